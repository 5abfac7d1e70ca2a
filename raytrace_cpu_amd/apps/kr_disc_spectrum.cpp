// apps/kr_disc_spectrum.cpp -- the continuum spectrum of the disc seen on an image plane, resident on the MI355X from start to finish: a multicolour
// blackbody with the Novikov-Thorne temperature profile (what kerrbb computes), or any tabulated rest-frame spectrum (a reflection table, a cut-off
// power law) smeared by the rays, relconv-style.  The rays are generated, traced, redshifted and summed into every output energy in HBM and only the
// Nen + 4 doubles of the spectrum come back (3 Nen + 4 with Stokes sums; include/kr_trace.h, kr_spectrum_model, has the per-ray rule).
//
// Reads the plane and disc keys of imageplane_app.h and the emissivity and limb keys of kr_line_profile (--parfile, outfile, dist, incl, plane_phi0, spin, r_disc,
// x0, xmax, Nx, y0, ymax, Ny, q1, rb1, q2, rb2, q3, emis_file, limb, limb_coeff, precision, integrator, rk45_tol; --arithmetic, --device, --timing), and
//   e_min = 0.1, e_max = 10   energy range of the Nen = 100 bins; the spectrum is sampled at the CENTRE of each bin
//   log_e = 1                 logarithmic bins (geometric centres)
//   model = thermal           thermal | table
//   thermal:  mass = 10       black-hole mass in solar masses
//             mdot = 1e18     accretion rate in g / s
//             f_col = 1.7     colour-correction factor: I = f_col^-4 B(E, f_col kT_eff)
//             kt_bins = 400   radial bins of the kT table, log-spaced over [r_isco, r_disc); kT in keV at each bin's centre, so E is in keV
//   table:    spec_file, Nzones, spec_bins = 512: the rest-frame spectrum per radial zone and the log grid it is resampled onto (rest_spectrum.h)
//   pol_law, pol_coeff        optional, the keys of kr_imageplane_polarisation (pol_law = 1, pol_coeff = 0.1171 when only one of them is given): the
//                             Stokes spectra Q(E), U(E) of the continuum (kr_post_spectrum_stokes_dev_f64) on the plane's own x and y axes; not with
//                             plunge = 1 (the polarisation frame has no plunging form)
//   disc_slope, disc_scale    (and disc_rin = ISCO; imageplane_app.h, DiscSurfaceKeys) with either key the disc has the surface of KR_STOP_THICKDISC and the
//                             spectrum is that of the rays that landed on it, every radius the cylindrical rho (kr_post_spectrum_surface_dev_f64); not
//                             with plunge = 1 or pol_law.  The file opens with the rows "# DISCSLOP", "# DISCSCAL", "# DISCRIN"; without the keys it is
//                             byte for byte what it was
// Every key may also be given as --key=value, which takes precedence over the file.  Nx and Ny are read as int, as kr_imageplane_disc_image reads
// them (before imageplane_app.h: as double, then cast; the same for a key written as a plain integer).
// Output: TextOutput (width 20, precision 8): three comment rows "# ON_DISC", "# USED", "# BAD_ANGLE" with their counts, then one row per energy:
// E flux.  The flux is per image-plane pixel: multiply by dx dy / dist^2 for a flux density.
// With pol_law or pol_coeff: the third comment row is "# BAD_POL" (disc records without a polarisation angle, which add to nothing) and every row is
// E I Q U.  Without them the file is byte for byte what it was before the keys existed.
#include <cmath>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/text_output.h"
#include "emissivity_table.h"
#include "imageplane_app.h"
#include "rest_spectrum.h"

namespace {

// CODATA 2018 / IAU 2015, cgs (api.py carries the same values)
const double kBoltzmannKeV = 8.617333262e-8, kSigmaSB = 5.670374419e-5, kG = 6.67430e-8, kC = 2.99792458e10, kMsun = 1.98841e33;

// the prograde ISCO in double (kerr_isco() keeps the reference's float-rounded intermediates)
double isco_radius(double a)
{
    const double z1 = 1 + cbrt((1 - a) * (1 + a)) * (cbrt(1 + a) + cbrt(1 - a));
    const double z2 = sqrt(3 * a * a + z1 * z1);
    return 3 + z2 - sqrt((3 - z1) * (3 + z1 + 2 * z2));
}

// Page & Thorne (1974): the flux of one face for Mdot = M = 1, in x = sqrt(r); exactly 0 at the ISCO, NaN inside (api.novikov_thorne_flux)
double novikov_thorne_flux(double r, double a)
{
    const double x0 = sqrt(isco_radius(a)), x = sqrt(r), ac = acos(a);
    if (!(x >= x0)) return NAN;
    const double roots[3] = {2 * cos((ac - M_PI) / 3), 2 * cos((ac + M_PI) / 3), -2 * cos(ac / 3)};
    double bracket = x - x0 - 1.5 * a * log(x / x0);
    for (int k = 0; k < 3; ++k) {
        const double xk = roots[k], xa = roots[k == 0 ? 1 : 0], xb = roots[k == 2 ? 1 : 2];        // the other two, in order
        bracket = bracket - 3 * (xk - a) * (xk - a) / (xk * (xk - xa) * (xk - xb)) * log((x - xk) / (x0 - xk));
    }
    return 3 / (8 * M_PI) * bracket / (x * x * x * x * (x * x * x - 3 * x + 2 * a));
}

}  // namespace

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt, true);
    const string emis_file = opt.str("emis_file", "");
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) opt.num("limb", 0);
    limb.coeff = opt.num("limb_coeff", 2.06);
    const bool stokes = opt.has("pol_law") || opt.has("pol_coeff");
    const kr_pol_law pol = krapp::pol_law_of(opt);
    if (stokes && s.flow.plunge) throw invalid_argument("pol_law / pol_coeff: the Stokes spectra do not take the plunging disc flow (plunge = 1)");
    const krapp::DiscSurfaceKeys disc(opt, s.r_isco, s.r_disc);
    disc.refuse_with(s.flow.plunge, stokes);

    const double e_min = opt.num("e_min", 0.1), e_max = opt.num("e_max", 10);
    const int ne = (int) opt.num("Nen", 100);
    const bool log_e = opt.num("log_e", 1) != 0;
    if (ne < 1) throw invalid_argument("Nen: at least one energy");
    const double de = log_e ? exp(log(e_max / e_min) / ne) : (e_max - e_min) / ne;
    const string model_name = opt.str("model", "thermal");
    if (model_name != "thermal" && model_name != "table") throw invalid_argument("model: expected thermal or table, got '" + model_name + "'");
    s.print_isco();

    const kr_imageplane plane = s.plane();
    kr_spectrum_model sm;
    memset(&sm, 0, sizeof sm);
    sm.e_min = e_min; sm.de = de; sm.ne = ne; sm.log_e = log_e ? 1 : 0;
    s.fill_disc(sm);
    sm.f_col = 1;
    vector<double> kt;
    krapp::RestSpectrum rest;
    krapp::EmisTable table;
    if (model_name == "thermal") {
        const double mass = opt.num("mass", 10), mdot = opt.num("mdot", 1e18);
        const int kt_bins = (int) opt.num("kt_bins", 400);
        if (kt_bins < 1) throw invalid_argument("kt_bins: at least one radial bin");
        sm.model = 0;
        sm.f_col = opt.num("f_col", 1.7);
        sm.table_r_min = s.r_isco;
        sm.table_dr = pow(s.r_disc / s.r_isco, 1.0 / kt_bins);
        sm.table_logbin = 1;
        sm.table_nr = kt_bins;
        const double scale = mdot * pow(kC, 6) / (kG * kG * (mass * kMsun) * (mass * kMsun));
        kt.resize((size_t) kt_bins);
        double kt_max = 0;
        for (int i = 0; i < kt_bins; ++i) {
            kt[(size_t) i] = kBoltzmannKeV * pow(novikov_thorne_flux(sm.table_r_min * pow(sm.table_dr, i + 0.5), s.spin) * scale / kSigmaSB, 0.25);
            if (kt[(size_t) i] > kt_max) kt_max = kt[(size_t) i];
        }
        sm.table_kt = kt.data();
        cout << "Novikov-Thorne disc: " << mass << " Msun, " << mdot << " g/s, f_col " << sm.f_col << ", peak kT_eff " << kt_max << " keV" << endl;
    } else {
        rest = krapp::read_rest_spectrum(opt);
        rest.fill(sm);
        if (!emis_file.empty()) {
            table = krapp::read_emis_table(emis_file);
            sm.table_r_min = table.r_min; sm.table_dr = table.dr; sm.table_logbin = 1;
            sm.table_nr = (int32_t) table.emis.size();
            sm.table_emis = table.emis.data();
            cout << "emissivity table " << emis_file << ": " << sm.table_nr << " bins from r = " << table.r_min << ", ratio " << table.dr << endl;
        }
        rest.print();
    }
    kr_params p = s.params(KR_RK45);
    disc.stop_on(p);

    // ---- device pipeline: init_emit -> trace -> redshift + range_phi + spectrum ---------------------------------------------------------
    krapp::DiscPlaneRun run(s, plane);
    const int64_t words = (int64_t) (stokes ? 3 : 1) * ne + 4;
    run.trace(plane, p, words);
    if (disc.thick)
        krapp::check(kr_post_spectrum_surface_dev_f64(&disc.surface, -s.spin, 1, -1 * M_PI, M_PI, &sm, &limb, run.rays->get(), run.n, run.acc->get(), nullptr),
                     "redshift + range_phi + spectrum of the surface");
    else if (stokes)
        krapp::check(kr_post_spectrum_stokes_dev_f64(-s.spin, s.flow.V(), 1, 0, 0, -1 * M_PI, M_PI, s.incl, &sm, &limb, &pol, run.rays->get(), run.n, run.acc->get(), nullptr),
                     "redshift + range_phi + spectrum with Stokes sums");
    else
        krapp::check(kr_post_spectrum_dev_f64(-s.spin, s.flow.V(), 1, 0, 0, -1 * M_PI, M_PI, &sm, &limb, run.rays->get(), run.n, run.acc->get(), nullptr), "redshift + range_phi + spectrum");
    vector<double> h((size_t) words);
    krapp::check(kr_memcpy_d2h(h.data(), run.acc->get(), words * (int64_t) sizeof(double)), "d2h");
    const double ms_post = run.clock.lap_ms();

    const double* tallies = h.data() + (size_t) (stokes ? 3 : 1) * ne;
    cout << static_cast<long>(tallies[0]) << " rays on the disc, " << static_cast<long>(tallies[1]) << " used, " << static_cast<long>(tallies[2])
         << (stokes ? " without a polarisation angle (bad-pol)" : " without an emission angle (bad-angle)") << endl;
    {
        TextOutput outfile(s.out_name);
        s.flow.write_rows(outfile);
        disc.write_rows(outfile);
        outfile << "# ON_DISC" << static_cast<long>(tallies[0]) << endl;
        outfile << "# USED" << static_cast<long>(tallies[1]) << endl;
        outfile << (stokes ? "# BAD_POL" : "# BAD_ANGLE") << static_cast<long>(tallies[2]) << endl;
        for (int i = 0; i < ne; ++i) {
            outfile << (log_e ? e_min * pow(de, i + 0.5) : e_min + (i + 0.5) * de) << h[(size_t) i];
            if (stokes) outfile << h[(size_t) ne + i] << h[(size_t) 2 * ne + i];
            outfile << endl;
        }
    }
    const double ms_out = run.clock.lap_ms();

    if (s.timing) run.print_timing() << "redshift+range_phi+spectrum+readback " << ms_post << " ms | text file " << ms_out << " ms" << endl;
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "../par/disc_spectrum.par", program); }
