// apps/kr_healpix_to_disc.cpp -- the reference's healpix_to_disc program (src/healpix/healpix_to_disc.cpp) resident on the MI355X: the sky of a point
// source in HEALPix pixels (RING order), every pixel's centre ray traced to the disc, and per pixel where it lands, with which energy shift and
// emissivity weight.  The rays are built, traced, redshifted and classified on the device (healpix_app.h); only the fate map comes back.
//
// Reads (healpix_to_disc.cpp:43-60): --parfile (default ../par/healpix_to_disc.par), --outfile | outfile, source (4 values), V, --spin | spin, order,
// motion = 0, basis = 1, rmax = 1000, r_disc = 500, show_progress = 1, q_in = 7, rb1 = 4, q_mid = 0, rb2 = 10, q_out = 3.
// Extensions: integrator = euler (the reference hard-codes Euler, :67), reverse = 0 (the reference's literal calls pass `true` to redshift_start and
// redshift, :66-69; that program is stale -- its class no longer compiles -- so neither choice is pinned to a build of it), rays_per_pixel = 1 (5: the
// reference's layout; the table is the same, it reads the centres only), unit_center = 0, --arithmetic | KRTRACE_ARITHMETIC, --device = 0, --timing.
// Motion 1 takes the emitted energy in the frame of the moving source (include/kr_trace.h, kr_healpix_source), not in the orbital frame.
//
// outfile: the reference's five columns `pix r phi redshift emis` (:74-83), emis = powerlaw3(r) redshift^-3; a pixel whose ray does not end on the disc
// (theta >= pi/2 - 1e-2, r_isco <= r < r_disc; the reference: r > r_isco) is `pix nan nan nan 0`.
#include <cmath>
#include <iostream>
#include <string>
using namespace std;

#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "../host/include/text_output.h"
#include "healpix_app.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/healpix_to_disc.par");
    ParameterFile par(par_name);

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    kr_healpix_source s;
    memset(&s, 0, sizeof s);
    par.get_parameter_array("source", s.pos, 4);
    s.V = par.get_parameter<double>("V");
    s.spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
    s.E = 1;
    s.order = par.get_parameter<int>("order");
    s.motion = par.get_parameter<int>("motion", 0);
    s.basis = par.get_parameter<int>("basis", 1);
    s.rays_per_pixel = par.get_parameter<int>("rays_per_pixel", 1);
    s.unit_center = par.get_parameter<int>("unit_center", 0);
    const double rmax = par.get_parameter<double>("rmax", 1000);
    const int show_progress = par.get_parameter<int>("show_progress", 1);
    const int reverse = par.get_parameter<int>("reverse", 0);
    const string integ = par.get_parameter<string>("integrator", "euler");
    const string arith = args.key_exists("--arithmetic") ? args.get_parameter<string>("--arithmetic") : krapp::arithmetic_from_env();
    const bool timing = args.key_exists("--timing");

    kr_healpix_map m;
    memset(&m, 0, sizeof m);
    m.r_isco = kerr_isco<double>(s.spin, +1);
    m.r_disc = par.get_parameter<double>("r_disc", 500);
    m.r_esc = rmax;
    m.theta_tol = 1E-2;
    m.q1 = par.get_parameter<double>("q_in", 7);
    m.rb1 = par.get_parameter<double>("rb1", 4);
    m.q2 = par.get_parameter<double>("q_mid", 0);
    m.rb2 = par.get_parameter<double>("rb2", 10);
    m.q3 = par.get_parameter<double>("q_out", 3);

    kr_params p;
    kr_params_default(&p, s.spin);
    p.integrator = krapp::integrator_code(integ, KR_EULER);
    p.theta_max = M_PI_2;
    p.r_max = rmax;
    p.stop_kind = KR_STOP_THETA;
    p.flags = krapp::arithmetic_flags(arith, p.integrator);

    krapp::require_device();             // before the output file is created
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch wall;
    const krapp::HealpixRun run = krapp::healpix_run(s, p, m, reverse, show_progress, timing);
    const double ms_device = wall.lap_ms();

    {
        TextOutput outfile(out_name.c_str());
        const double *cls = run.plane(0), *r = run.plane(1), *phi = run.plane(3), *g = run.plane(4), *emis = run.plane(6);
        for (int64_t pix = 0; pix < run.npix; ++pix) {
            if (cls[pix] == 1)
                outfile << pix << r[pix] << phi[pix] << g[pix] << emis[pix] << endl;
            else
                outfile << pix << "nan" << "nan" << "nan" << 0 << endl;
        }
        outfile.close();
    }
    if (timing)
        cout << "timing: pixels " << run.npix << " rays " << run.stats.rays_traced << " steps " << run.stats.steps_total << " | source+redshift_start " << run.ms_init
             << " ms | trace " << run.ms_trace << " ms (kernels " << run.stats.kernel_ms << ") | range_phi+redshift+fate map " << run.ms_post << " ms | device total "
             << ms_device << " ms | file " << wall.lap_ms() << " ms" << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
