// apps/kr_reverb_response.cpp -- the reverberation response of the disc seen on an image plane, resident on the MI355X from start to finish: the
// energy-time impulse response of a whole tabulated rest-frame reflection spectrum (one file per ionisation zone), each disc ray adding to every output
// energy of the time row its arrival falls in.  The rays are generated, traced, redshifted and summed in HBM and only the Nt x Nen + 4 doubles of the
// response come back (include/kr_trace.h, kr_response_model, has the per-ray rule).
//
// Reads the plane and disc keys of imageplane_app.h and the limb keys of kr_line_profile (--parfile, outfile, dist, incl, plane_phi0, spin, r_disc, x0, xmax,
// Nx, y0, ymax, Ny, q1, rb1, q2, rb2, q3, limb, limb_coeff, precision, integrator, rk45_tol; --arithmetic, --device, --timing), and
//   e_min = 0.1, e_max = 10, Nen = 100, log_e = 1    the output energies, as kr_disc_spectrum reads them: the response is sampled at the CENTRE of each bin
//   spec_file, Nzones, spec_bins = 512               the rest-frame spectrum per radial zone and the log grid it is resampled onto (rest_spectrum.h)
//   emis_file                 a 7-column emissivity table (kr_emissivity): its emis column is the emissivity and its time column the source -> disc
//                             delay by radius; without it the program uses the powerlaw3 emissivity and no source delay
//   t0 = dist, dt = 1, Nt = 100   the time rows: row j holds t0 + j dt <= t + delay < t0 + (j + 1) dt, in GM / c^3.  t0 is the caller's choice of the
//                             instant the direct continuum arrives.
//   disc_slope, disc_scale    (and disc_rin = ISCO; imageplane_app.h, DiscSurfaceKeys) with either key the disc has the surface of KR_STOP_THICKDISC and the
//                             response is that of the rays that landed on it (kr_post_response_surface_dev_f64; no plunge); the header gains DISCSLOP,
//                             DISCSCAL and DISCRIN.  Without the keys the program and its file are what they were.
// Every key may also be given as --key=value, which takes precedence over the file.
// Output: a FITS file (host/include/fits_output.h).  The primary HDU holds the response, Nen pixels along axis 1 and Nt along axis 2, with the tallies
// ON_DISC, USED, BADANGLE and OUTSIDE and the axes' parameters as header keys; the HDUs ENERGY (Nen x 1) and TIME (Nt x 1) hold the sampling energies and
// the centres (j + 0.5) dt of the rows, counted from t0.  The response is per image-plane pixel: multiply by dx dy / dist^2 for a flux density.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/fits_output.h"
#include "emissivity_table.h"
#include "imageplane_app.h"
#include "rest_spectrum.h"

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt, true);
    const string emis_file = opt.str("emis_file", "");
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) opt.num("limb", 0);
    limb.coeff = opt.num("limb_coeff", 2.06);

    const double e_min = opt.num("e_min", 0.1), e_max = opt.num("e_max", 10);
    const int ne = (int) opt.num("Nen", 100);
    const bool log_e = opt.num("log_e", 1) != 0;
    if (ne < 1) throw invalid_argument("Nen: at least one energy");
    const double de = log_e ? exp(log(e_max / e_min) / ne) : (e_max - e_min) / ne;
    const double t0 = opt.num("t0", s.dist), dt = opt.num("dt", 1);
    const int nt = (int) opt.num("Nt", 100);
    if (nt < 1) throw invalid_argument("Nt: at least one time row");
    const krapp::DiscSurfaceKeys disc(opt, s.r_isco, s.r_disc);
    disc.refuse_with(s.flow.plunge, opt.has("pol_law") || opt.has("pol_coeff"));
    s.print_isco();

    const kr_imageplane plane = s.plane();
    kr_response_model rm;
    memset(&rm, 0, sizeof rm);
    kr_spectrum_model& sm = rm.spec;
    sm.e_min = e_min; sm.de = de; sm.ne = ne; sm.log_e = log_e ? 1 : 0;
    s.fill_disc(sm);
    sm.f_col = 1;
    rm.t0 = t0; rm.dt = dt; rm.nt = nt;
    const krapp::RestSpectrum rest = krapp::read_rest_spectrum(opt, "kr_reverb_response needs spec_file");
    rest.fill(sm);
    krapp::EmisTable table;
    if (!emis_file.empty()) {
        table = krapp::read_emis_table(emis_file);
        sm.table_r_min = table.r_min; sm.table_dr = table.dr; sm.table_logbin = 1;
        sm.table_nr = (int32_t) table.emis.size();
        sm.table_emis = table.emis.data();
        rm.table_time = table.time.data();
        cout << "emissivity and delay table " << emis_file << ": " << sm.table_nr << " bins from r = " << table.r_min << ", ratio " << table.dr << endl;
    }
    rest.print();
    kr_params p = s.params(KR_RK45);
    disc.stop_on(p);

    // ---- device pipeline: init_emit -> trace -> redshift + range_phi + response ---------------------------------------------------------
    krapp::DiscPlaneRun run(s, plane);
    const int64_t cells = (int64_t) nt * ne, words = cells + 4;
    run.trace(plane, p, words);
    if (disc.thick)
        krapp::check(kr_post_response_surface_dev_f64(&disc.surface, -s.spin, 1, -1 * M_PI, M_PI, &rm, &limb, run.rays->get(), run.n, run.acc->get(), nullptr),
                     "redshift + range_phi + response of the surface");
    else
        krapp::check(kr_post_response_dev_f64(-s.spin, s.flow.V(), 1, 0, 0, -1 * M_PI, M_PI, &rm, &limb, run.rays->get(), run.n, run.acc->get(), nullptr), "redshift + range_phi + response");
    vector<double> h((size_t) words);
    krapp::check(kr_memcpy_d2h(h.data(), run.acc->get(), words * (int64_t) sizeof(double)), "d2h");
    const double ms_post = run.clock.lap_ms();

    const long on_disc = static_cast<long>(h[(size_t) cells]), used = static_cast<long>(h[(size_t) cells + 1]), bad_angle = static_cast<long>(h[(size_t) cells + 2]),
               outside = static_cast<long>(h[(size_t) cells + 3]);
    cout << on_disc << " rays on the disc, " << used << " used, " << bad_angle << " without an emission angle (bad-angle), " << outside << " outside the time window" << endl;
    {
        vector<double> energy((size_t) ne), time((size_t) nt);
        for (int i = 0; i < ne; ++i) energy[(size_t) i] = log_e ? e_min * pow(de, i + 0.5) : e_min + (i + 0.5) * de;
        for (int j = 0; j < nt; ++j) time[(size_t) j] = (j + 0.5) * dt;
        FITSOutput<double> fits(s.out_name);
        fits.write_image_array(h.data(), ne, nt);
        fits.write_comment("Energy-time response of the accretion disc: axis 1 energy, axis 2 time");
        fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "kr_reverb_response");
        fits.write_keyword("DIST", "Distance to image plane", s.dist);
        fits.write_keyword("INCL", "Inclination of line of sight", s.incl);
        fits.write_keyword("SPIN", "Black hole spin", s.spin);
        fits.write_keyword("ISCO", "Innermost stable circular orbit", s.r_isco);
        fits.write_keyword("RDISC", "Maximum radius of disc", s.r_disc);
        s.flow.write_keywords(fits);
        disc.write_keywords(fits);
        fits.write_keyword("NRAYS", "Number of rays", static_cast<long>(run.n));
        fits.write_keyword("ON_DISC", "Rays hitting disc", on_disc);
        fits.write_keyword("USED", "Rays with an emissivity and a delay", used);
        fits.write_keyword("BADANGLE", "Rays on the disc without an emission angle", bad_angle);
        fits.write_keyword("OUTSIDE", "Used rays outside the time window", outside);
        fits.write_keyword("T0", "Start of the first time row (GM/c^3)", t0);
        fits.write_keyword("DT", "Width of a time row (GM/c^3)", dt);
        fits.write_keyword("NT", "Number of time rows", nt);
        fits.write_keyword("E_MIN", "Lower edge of the first energy bin", e_min);
        fits.write_keyword("DE", log_e ? "Ratio between energy bin edges" : "Width of an energy bin", de);
        fits.write_keyword("NEN", "Number of energies", ne);
        fits.write_keyword("LOG_E", "Logarithmic energy bins", log_e);
        fits.write_image_array(energy.data(), ne, 1);
        fits.set_ext_name("ENERGY");
        fits.write_comment("Energies at which the response is sampled: the bin centres");
        fits.write_image_array(time.data(), nt, 1);
        fits.set_ext_name("TIME");
        fits.write_comment("Centres of the time rows, counted from T0");
        fits.close();
    }
    const double ms_out = run.clock.lap_ms();

    if (s.timing) run.print_timing() << "redshift+range_phi+response+readback " << ms_post << " ms | FITS file " << ms_out << " ms" << endl;
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "../par/reverb_response.par", program); }
