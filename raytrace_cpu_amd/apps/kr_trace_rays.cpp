// apps/kr_trace_rays.cpp -- the reference's `trace_rays` program (src/ray_paths/trace_rays.cpp) with the rays resident on the MI355X: the
// PointSource rays are generated on the device, their paths are counted and recorded there (kr_trace_paths_*_dev_f64), the rows come back
// once and are written as the same text file (t x y z, or t r theta phi with write_cartesian = 0; two blank lines after each ray).
//
// Reads (trace_rays.cpp:22-56): --parfile (default ../par/trace_rays.par), --outfile | outfile, source[4], V = -1 (-> the disc velocity at
// source[1], :58), --spin | spin, cosalpha0 = -0.995, cosalphamax = 0.995, dcosalpha, beta0 = -pi, betamax = pi, dbeta, r_max = 100,
// theta_max = pi / 2, show_progress (read, unused here), write_step = 10, write_rmin = -1, write_rmax = -1, write_cartesian = 1 (read as a
// double, :56).  The integrator is Euler, as the reference hard-wires it (:71); no redshift_start, which the reference does not call.
// Extensions: --device = 0, --timing.
#include <cmath>
#include <iostream>
#include <string>
using namespace std;

#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "path_recording.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/trace_rays.par");
    ParameterFile par(par_name);

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    double source[4];
    par.get_parameter_array("source", source, 4);
    double V = par.get_parameter<double>("V", -1);
    const double spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
    kr_pointsource src;
    memset(&src, 0, sizeof src);
    src.cosalpha0 = par.get_parameter<double>("cosalpha0", -0.995);
    src.cosalphamax = par.get_parameter<double>("cosalphamax", 0.995);
    src.dcosalpha = par.get_parameter<double>("dcosalpha");
    src.beta0 = par.get_parameter<double>("beta0", -1 * M_PI);
    src.betamax = par.get_parameter<double>("betamax", M_PI);
    src.dbeta = par.get_parameter<double>("dbeta");
    const double r_max = par.get_parameter<double>("r_max", 100);
    const double theta_max = par.get_parameter<double>("theta_max", M_PI_2);
    (void) par.get_parameter<int>("show_progress", 1);
    const double write_step = par.get_parameter<double>("write_step", 10);
    const double write_rmin = par.get_parameter<double>("write_rmin", -1);
    const double write_rmax = par.get_parameter<double>("write_rmax", -1);
    const bool write_cartesian = par.get_parameter<double>("write_cartesian", true);
    const bool timing = args.key_exists("--timing");

    if (V < 0) V = disc_velocity(source[1], spin, +1);

    cout << "*****" << endl;
    cout << "Source r = [" << source[0] << " , " << source[1] << " , " << source[2] << " , " << source[3] << "] mu" << endl;
    cout << "Source angular velocity V = " << V << " mu*c" << endl;
    cout << "Spin a = " << spin << endl;
    cout << "*****" << endl << endl;

    for (int i = 0; i < 4; ++i) src.pos[i] = source[i];
    src.V = V;
    src.spin = spin;
    src.tol = 100;   // TOL, raytracer.h
    src.E = 1;

    kr_params p;
    kr_params_default(&p, spin);
    p.integrator = KR_EULER;
    p.theta_max = theta_max;
    p.r_max = r_max;
    p.stop_kind = KR_STOP_THETA;
    p.flags = 0;                         // paths carry the reference's arithmetic

    kr_path_spec w;
    memset(&w, 0, sizeof w);
    w.write_step = static_cast<int>(write_step);      // (a double handed to an int parameter, :53 / :71)
    w.write_rmin = write_rmin;
    w.write_rmax = write_rmax;

    // ---- device pipeline ------------------------------------------------------------------------------------------
    krapp::require_device();
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t n = kr_pointsource_count(&src, nullptr, nullptr);
    if (n <= 0) throw runtime_error("empty ray grid");
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::check(kr_pointsource_init_dev_f64(&src, rays.get(), n, nullptr), "pointsource_init");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_init = clock.lap_ms();
    cout << "Running raytracer..." << endl;
    const krapp::PathTimes tm = krapp::record_paths_to_text(p, w, write_cartesian, spin, rays.get(), n, out_name);
    if (timing) krapp::print_path_times(tm, ms_init);
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
