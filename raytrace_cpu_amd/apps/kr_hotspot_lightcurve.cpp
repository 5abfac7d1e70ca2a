// apps/kr_hotspot_lightcurve.cpp -- an orbiting hot spot on the disc seen on an image plane, resident on the MI355X from start to finish: the light
// curve of the flare with its Doppler and lensing peaks, the track of the image centroid, and the energy-time spectrogram of a line emitted by the spot.
// The rays are generated, traced, redshifted and summed into every observer time in HBM and only the Nt (3 + Nen) + 4 doubles come back
// (include/kr_trace.h, kr_hotspot, has the per-ray rule).  The spot is a pattern of enhanced emission on the disc, good for spot_sigma << spot_r; the gas
// under it keeps its Keplerian orbits.  It is not a body with a four-velocity of its own.
//
// Reads the parameter file and the plane and disc keys of kr_imageplane_disc_image (--parfile, outfile, dist, incl, plane_phi0, spin, r_disc, x0, xmax,
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
// Every key may also be given as --key=value, which takes precedence over the file.
// Output: TextOutput (width 20, precision 8): three comment rows "# ON_DISC", "# USED", "# BAD_ANGLE" with their counts, one row per observer time:
// T flux x_c y_c (nan where flux is 0), and with ne > 0 one block per observer time, each after a blank line: a row T E_mid value per energy bin.
// The sums are per image-plane pixel: multiply by dx dy / dist^2 for a flux.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "../host/include/text_output.h"
#include "app_common.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process (include/kr_trace.h)
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/hotspot_lightcurve.par");
    ParameterFile par(par_name);
    // --key=value first, then the parameter file, then the default
    auto num = [&](const string& key, double dflt) { return args.key_exists("--" + key) ? args.get_parameter<double>("--" + key) : par.get_parameter<double>(key, dflt); };
    auto req = [&](const string& key) { return args.key_exists("--" + key) ? args.get_parameter<double>("--" + key) : par.get_parameter<double>(key); };
    auto has = [&](const string& key) { return args.key_exists("--" + key) || par.key_exists(key); };
    auto str = [&](const string& key, const string& dflt) { return args.key_exists("--" + key) ? args.get_parameter<string>("--" + key) : par.get_parameter<string>(key, dflt); };

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    const double dist = req("dist"), incl = req("incl"), plane_phi0 = num("plane_phi0", 0), spin = req("spin"), r_disc = req("r_disc");
    const double x0 = num("x0", -1 * r_disc), xmax = num("xmax", r_disc);
    const int Nx = (int) req("Nx");
    const double y0 = num("y0", x0), ymax = num("ymax", xmax);
    const int Ny = (int) num("Ny", Nx);
    const double precision = num("precision", 100);
    const string integ = str("integrator", "rk45");
    const double rk45_tol = num("rk45_tol", 1e-8);
    const string arith = args.key_exists("--arithmetic") ? args.get_parameter<string>("--arithmetic") : krapp::arithmetic_from_env();
    const bool timing = args.key_exists("--timing");
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) num("limb", 0);
    limb.coeff = num("limb_coeff", 2.06);

    const double dx = (xmax - x0) / Nx, dy = (ymax - y0) / Ny;
    const double r_isco = kerr_isco<double>(spin, +1);
    cout << "ISCO at " << r_isco << endl;

    kr_hotspot h;
    memset(&h, 0, sizeof h);
    h.r_spot = req("spot_r");
    h.sigma = req("spot_sigma");
    h.cut = num("spot_cut", 3);
    h.phi0 = num("spot_phi0", 0);
    h.a_orbit = spin;
    h.omega = has("spot_omega") ? req("spot_omega") : 1 / (spin + h.r_spot * sqrt(h.r_spot));
    h.shear = (int32_t) num("spot_shear", 0);
    h.nt = (int32_t) num("nt", 64);
    if (h.nt < 1) throw invalid_argument("nt: at least one observer time");
    h.t0 = num("t0", dist);
    if (has("dt")) {
        h.dt = req("dt");
    } else {
        if (h.omega == 0) throw invalid_argument("periods: a static spot (spot_omega = 0) has no period; give dt");
        h.dt = num("periods", 1) * (2 * M_PI / fabs(h.omega)) / h.nt;
    }
    h.g_index = num("g_index", 4);
    h.line_energy = num("line_en", 6.4);
    h.ne = (int32_t) num("ne", 0);
    h.log_e = num("log_e", 0) != 0 ? 1 : 0;
    h.e_min = num("e_min", 1);
    const double e_max = num("e_max", 10);
    h.de = h.ne > 0 ? (h.log_e ? exp(log(e_max / h.e_min) / h.ne) : (e_max - h.e_min) / h.ne) : 1;
    h.r_isco = r_isco;
    h.r_disc = r_disc;
    cout << "hot spot at r = " << h.r_spot << ", sigma " << h.sigma << ", pattern speed " << h.omega << (h.shear ? " (sheared)" : "") << "; " << h.nt
         << " observer times from " << h.t0 << " in steps of " << h.dt << endl;

    kr_imageplane plane;
    memset(&plane, 0, sizeof plane);
    plane.dist = dist;
    plane.inc_deg = incl;
    plane.x0 = x0; plane.xmax = xmax; plane.dx = dx;
    plane.y0 = y0; plane.ymax = ymax; plane.dy = dy;
    plane.spin = spin;
    plane.phi0 = plane_phi0;
    plane.precision = precision;

    kr_params p;
    kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane.cpp:12)
    p.precision = precision;
    p.integrator = krapp::integrator_code(integ, KR_RK45);
    if (p.integrator == KR_RK45) p.rk45_tol = rk45_tol;
    p.theta_max = M_PI_2;
    p.r_max = 1.1 * dist;
    p.stop_kind = KR_STOP_THETA;
    p.flags = krapp::arithmetic_flags(arith, p.integrator);

    // ---- device pipeline: init_emit -> trace -> redshift + range_phi + hot spot ---------------------------------------------------------
    krapp::check(kr_set_device((int) num("device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t n = kr_imageplane_count(&plane, nullptr, nullptr);
    if (n <= 0) throw runtime_error("empty ray grid");
    const int nt = h.nt, ne = h.ne;
    if (ne < 0 || ne > 4096 || nt > 4096) throw invalid_argument("nt and ne: at most 4096 each, ne not negative");
    const int64_t words = (int64_t) nt * (3 + ne) + 4;
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::DeviceBuffer acc(words * (int64_t) sizeof(double));
    acc.zero();
    krapp::check(kr_imageplane_init_emit_dev_f64(&plane, 0, 1, 0.0, 1, 0, rays.get(), n, nullptr), "imageplane_init + redshift_start");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_init = clock.lap_ms();
    kr_stats st;
    krapp::check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &st), "trace");
    const double ms_trace = clock.lap_ms();
    krapp::check(kr_post_hotspot_dev_f64(-spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, &h, &limb, rays.get(), n, acc.get(), nullptr), "redshift + range_phi + hot spot");
    vector<double> w((size_t) words);
    krapp::check(kr_memcpy_d2h(w.data(), acc.get(), words * (int64_t) sizeof(double)), "d2h");
    const double ms_post = clock.lap_ms();

    const double* flux = w.data();
    const double* sx = flux + nt;
    const double* sy = sx + nt;
    const double* spec = sy + nt;
    const double* tallies = spec + (size_t) nt * ne;
    cout << static_cast<long>(tallies[0]) << " rays on the disc, " << static_cast<long>(tallies[1]) << " in the spot's ring, " << static_cast<long>(tallies[2])
         << " without an emission angle (bad-angle)" << endl;
    {
        TextOutput outfile(out_name);
        outfile << "# ON_DISC" << static_cast<long>(tallies[0]) << endl;
        outfile << "# USED" << static_cast<long>(tallies[1]) << endl;
        outfile << "# BAD_ANGLE" << static_cast<long>(tallies[2]) << endl;
        const double nan = numeric_limits<double>::quiet_NaN();
        for (int k = 0; k < nt; ++k) {
            const bool lit = flux[k] != 0;
            outfile << h.t0 + k * h.dt << flux[k] << (lit ? sx[k] / flux[k] : nan) << (lit ? sy[k] / flux[k] : nan) << endl;
        }
        for (int k = 0; k < nt && ne > 0; ++k) {
            outfile.newline();
            for (int i = 0; i < ne; ++i)
                outfile << h.t0 + k * h.dt << (h.log_e ? h.e_min * pow(h.de, i + 0.5) : h.e_min + (i + 0.5) * h.de) << spec[(size_t) k * ne + i] << endl;
        }
    }
    const double ms_out = clock.lap_ms();

    if (timing)
        cout << "timing: rays " << st.rays_traced << " steps " << st.steps_total << " | init+redshift_start " << ms_init << " ms | trace " << ms_trace
             << " ms (kernel " << st.kernel_ms << ") | redshift+range_phi+hot spot+readback " << ms_post << " ms | text file " << ms_out << " ms" << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
