// apps/kr_hotspot_lightcurve.cpp -- an orbiting hot spot on the disc seen on an image plane, resident on the MI355X from start to finish: the light
// curve of the flare with its Doppler and lensing peaks, the track of the image centroid, and the energy-time spectrogram of a line emitted by the spot.
// The rays are generated, traced, redshifted and summed into every observer time in HBM and only the Nt (3 + Nen) + 4 doubles come back (Nt (5 + Nen) + 4 with Stokes sums)
// (include/kr_trace.h, kr_hotspot, has the per-ray rule).  The spot is a pattern of enhanced emission on the disc, good for spot_sigma << spot_r; the gas
// under it keeps its Keplerian orbits.  It is not a body with a four-velocity of its own.
//
// Reads the plane and disc keys of imageplane_app.h (--parfile, outfile, dist, incl, plane_phi0, spin, r_disc, x0, xmax,
// Nx, y0, ymax, Ny, precision, integrator, rk45_tol; --arithmetic, --device, --timing), and
//   spot_r                    radius of the spot's centre (required)
//   spot_sigma                its Gaussian width (required)
//   spot_cut = 3              the cut-off in units of spot_sigma: the shifted Gaussian reaches 0 there
//   spot_phi0 = 0             azimuth of the centre at coordinate time 0
//   spot_omega                pattern speed; absent: Keplerian at spot_r, 1 / (spin + spot_r^1.5)
//   spot_shear = 0            1: every radius at its own Keplerian rate (the spot winds into an arc)
//   nt = 64                   observer times T_k = t0 + k dt
//   t0 = dist                 the first observer time (a ray's own travel time is about dist)
//   dt  or  periods = 1       the step, or the number of periods P = 2 pi / |omega| the nt samples span: dt = periods P / nt
//   g_index = 4               weight exponent g^-g_index: 4 bolometric, 3 the specific intensity of a line
//   limb = 0, limb_coeff = 2.06   limb law of kr_limb_law
//   line_en = 6.4, e_min = 1, e_max = 10, ne = 0, log_e = 0   the spectrogram's line energy and its ne energy bins (ne = 0: none)
//   pol_law, pol_coeff        optional, the keys of kr_imageplane_polarisation (pol_law = 1, pol_coeff = 0.1171 when only one of them is given): the
//                             Stokes light curves Q, U of the spot's emission (kr_post_hotspot_stokes_dev_f64) on the plane's own x and y axes
// Every key may also be given as --key=value, which takes precedence over the file.  Nx and Ny are read as int, as kr_imageplane_disc_image reads
// them (before imageplane_app.h: as double, then cast; the same for a key written as a plain integer).
// Output: TextOutput (width 20, precision 8): three comment rows "# ON_DISC", "# USED", "# BAD_ANGLE" with their counts, one row per observer time:
// T flux x_c y_c (nan where flux is 0), and with ne > 0 one block per observer time, each after a blank line: a row T E_mid value per energy bin.
// With pol_law or pol_coeff: the third comment row is "# BAD_POL" (ring records without a polarisation angle, which add to nothing) and every row is
// T flux x_c y_c Q U.  Without them the file is byte for byte what it was before the keys existed.
// The sums are per image-plane pixel: multiply by dx dy / dist^2 for a flux.
#include <cmath>
#include <iostream>
#include <limits>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/text_output.h"
#include "imageplane_app.h"

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt);
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) opt.num("limb", 0);
    limb.coeff = opt.num("limb_coeff", 2.06);
    const bool stokes = opt.has("pol_law") || opt.has("pol_coeff");
    const kr_pol_law pol = krapp::pol_law_of(opt);
    s.print_isco();

    kr_hotspot h;
    memset(&h, 0, sizeof h);
    h.r_spot = opt.req("spot_r");
    h.sigma = opt.req("spot_sigma");
    h.cut = opt.num("spot_cut", 3);
    h.phi0 = opt.num("spot_phi0", 0);
    h.a_orbit = s.spin;
    h.omega = opt.has("spot_omega") ? opt.req("spot_omega") : 1 / (s.spin + h.r_spot * sqrt(h.r_spot));
    h.shear = (int32_t) opt.num("spot_shear", 0);
    h.nt = (int32_t) opt.num("nt", 64);
    if (h.nt < 1) throw invalid_argument("nt: at least one observer time");
    h.t0 = opt.num("t0", s.dist);
    if (opt.has("dt")) {
        h.dt = opt.req("dt");
    } else {
        if (h.omega == 0) throw invalid_argument("periods: a static spot (spot_omega = 0) has no period; give dt");
        h.dt = opt.num("periods", 1) * (2 * M_PI / fabs(h.omega)) / h.nt;
    }
    h.g_index = opt.num("g_index", 4);
    h.line_energy = opt.num("line_en", 6.4);
    h.ne = (int32_t) opt.num("ne", 0);
    h.log_e = opt.num("log_e", 0) != 0 ? 1 : 0;
    h.e_min = opt.num("e_min", 1);
    const double e_max = opt.num("e_max", 10);
    h.de = h.ne > 0 ? (h.log_e ? exp(log(e_max / h.e_min) / h.ne) : (e_max - h.e_min) / h.ne) : 1;
    h.r_isco = s.r_isco;
    h.r_disc = s.r_disc;
    cout << "hot spot at r = " << h.r_spot << ", sigma " << h.sigma << ", pattern speed " << h.omega << (h.shear ? " (sheared)" : "") << "; " << h.nt
         << " observer times from " << h.t0 << " in steps of " << h.dt << endl;

    const kr_imageplane plane = s.plane();
    const kr_params p = s.params(KR_RK45);

    // ---- device pipeline: init_emit -> trace -> redshift + range_phi + hot spot ---------------------------------------------------------
    krapp::DiscPlaneRun run(s, plane);
    const int nt = h.nt, ne = h.ne;
    if (ne < 0 || ne > 4096 || nt > 4096) throw invalid_argument("nt and ne: at most 4096 each, ne not negative");
    const int curves = stokes ? 5 : 3;
    const int64_t words = (int64_t) nt * (curves + ne) + 4;
    run.trace(plane, p, words);
    if (stokes)
        krapp::check(kr_post_hotspot_stokes_dev_f64(-s.spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, s.incl, &h, &limb, &pol, run.rays->get(), run.n, run.acc->get(), nullptr),
                     "redshift + range_phi + hot spot with Stokes sums");
    else
        krapp::check(kr_post_hotspot_dev_f64(-s.spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, &h, &limb, run.rays->get(), run.n, run.acc->get(), nullptr), "redshift + range_phi + hot spot");
    vector<double> w((size_t) words);
    krapp::check(kr_memcpy_d2h(w.data(), run.acc->get(), words * (int64_t) sizeof(double)), "d2h");
    const double ms_post = run.clock.lap_ms();

    const double* flux = w.data();
    const double* sx = flux + nt;
    const double* sy = sx + nt;
    const double* sq = sy + nt;                      // (Stokes only)
    const double* su = sq + nt;
    const double* spec = flux + (size_t) curves * nt;
    const double* tallies = spec + (size_t) nt * ne;
    cout << static_cast<long>(tallies[0]) << " rays on the disc, " << static_cast<long>(tallies[1]) << " in the spot's ring, " << static_cast<long>(tallies[2])
         << (stokes ? " ring records without a polarisation angle (bad-pol)" : " without an emission angle (bad-angle)") << endl;
    {
        TextOutput outfile(s.out_name);
        outfile << "# ON_DISC" << static_cast<long>(tallies[0]) << endl;
        outfile << "# USED" << static_cast<long>(tallies[1]) << endl;
        outfile << (stokes ? "# BAD_POL" : "# BAD_ANGLE") << static_cast<long>(tallies[2]) << endl;
        const double nan = numeric_limits<double>::quiet_NaN();
        for (int k = 0; k < nt; ++k) {
            const bool lit = flux[k] != 0;
            outfile << h.t0 + k * h.dt << flux[k] << (lit ? sx[k] / flux[k] : nan) << (lit ? sy[k] / flux[k] : nan);
            if (stokes) outfile << sq[k] << su[k];
            outfile << endl;
        }
        for (int k = 0; k < nt && ne > 0; ++k) {
            outfile.newline();
            for (int i = 0; i < ne; ++i)
                outfile << h.t0 + k * h.dt << (h.log_e ? h.e_min * pow(h.de, i + 0.5) : h.e_min + (i + 0.5) * h.de) << spec[(size_t) k * ne + i] << endl;
        }
    }
    const double ms_out = run.clock.lap_ms();

    if (s.timing) run.print_timing() << "redshift+range_phi+hot spot+readback " << ms_post << " ms | text file " << ms_out << " ms" << endl;
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "../par/hotspot_lightcurve.par", program); }
