// apps/kr_healpix_photonfrac.cpp -- the reference's healpix_disc_source_photonfrac program (src/healpix/healpix_disc_source_photonfrac.cpp) resident
// on the MI355X: which fraction of the sky of a source ON the disc returns to the disc, escapes or is lost to the hole, as pixel counts of an
// equal-area HEALPix sampling (healpix_app.h: the rays never leave the device).
//
// Reads (:37-49): --parfile (default ../par/healpix_disc_source_photonfrac.par), --source_r | source_r, source_phi = 1.5707, V = -1 (negative: the
// disc's velocity at source_r, :58), --spin | spin, order, show_progress = 1, r_esc = 1000, r_disc := the r_esc key with default 500 (sic, :49).
// The source sits at (0, source_r, pi/2 - 1e-6, source_phi), basis 1, as a disc source (set_disc_source(), :77: the rays that start into the disc
// under it are unused slots and in no count), and is traced with Euler to theta = pi/2 or 1.1 r_esc (:75-80); rays that land within 0.1 source_r
// and 0.1 rad of the source itself are in none of the three counts but in the ray count they are divided by (:89-97).
// Extensions: integrator = euler, rays_per_pixel = 1, --arithmetic | KRTRACE_ARITHMETIC, --device = 0, --timing.
//
// Prints the reference's three lines (:111-113): Escape, Return, Lost, each over the count of live rays.
#include <cmath>
#include <iostream>
#include <string>
using namespace std;

#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "healpix_app.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/healpix_disc_source_photonfrac.par");
    ParameterFile par(par_name);

    const double source_r = args.key_exists("--source_r") ? args.get_parameter<double>("--source_r") : par.get_parameter<double>("source_r");
    const double source_phi = par.get_parameter<double>("source_phi", 1.5707);
    double V = par.get_parameter<double>("V", -1);
    const double spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
    const int order = (int) par.get_parameter<double>("order");
    const int show_progress = par.get_parameter<int>("show_progress", 1);
    const double r_esc = par.get_parameter<double>("r_esc", 1000);
    const double r_disc = par.get_parameter<double>("r_esc", 500);
    const string integ = par.get_parameter<string>("integrator", "euler");
    const string arith = args.key_exists("--arithmetic") ? args.get_parameter<string>("--arithmetic") : krapp::arithmetic_from_env();
    const bool timing = args.key_exists("--timing");
    if (V < 0) V = disc_velocity<double>(source_r, spin, +1);

    kr_healpix_source s;
    memset(&s, 0, sizeof s);
    s.pos[0] = 0; s.pos[1] = source_r; s.pos[2] = M_PI_2 - 1E-6; s.pos[3] = source_phi;
    s.V = V; s.spin = spin; s.E = 1;
    s.order = order; s.motion = 0; s.basis = 1;
    s.rays_per_pixel = par.get_parameter<int>("rays_per_pixel", 1);
    s.disc_source = 1;

    kr_healpix_map m;
    memset(&m, 0, sizeof m);
    m.r_isco = kerr_isco<double>(spin, +1);
    m.r_disc = r_disc; m.r_esc = r_esc; m.theta_tol = 0;
    m.source_r = source_r; m.source_phi = source_phi; m.self_zone = 1;
    m.q1 = 3; m.rb1 = 4; m.q2 = 3; m.rb2 = 10; m.q3 = 3;

    kr_params p;
    kr_params_default(&p, spin);
    p.integrator = krapp::integrator_code(integ, KR_EULER);
    p.theta_max = M_PI_2;
    p.r_max = 1.1 * r_esc;
    p.stop_kind = KR_STOP_THETA;
    p.flags = krapp::arithmetic_flags(arith, p.integrator);

    krapp::require_device();
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch wall;
    const krapp::HealpixRun run = krapp::healpix_run(s, p, m, 0, show_progress, timing);
    const double ray_count = run.tally(0), return_count = run.tally(1), escape_count = run.tally(2), lost_count = run.tally(3);

    cout << endl << "Escape: " << escape_count / ray_count << endl;
    cout << "Return: " << return_count / ray_count << endl;
    cout << "Lost:   " << lost_count / ray_count << endl << endl;
    if (timing)
        cout << "timing: pixels " << run.npix << " rays " << run.stats.rays_traced << " steps " << run.stats.steps_total << " | source+redshift_start " << run.ms_init
             << " ms | trace " << run.ms_trace << " ms (kernels " << run.stats.kernel_ms << ") | range_phi+fate map " << run.ms_post << " ms | device total "
             << wall.lap_ms() << " ms" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
