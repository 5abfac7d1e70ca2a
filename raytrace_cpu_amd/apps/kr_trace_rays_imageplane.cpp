// apps/kr_trace_rays_imageplane.cpp -- the reference's `trace_rays_imageplane` program (src/ray_paths/trace_rays_imageplane.cpp) with the rays
// resident on the MI355X: ImagePlane rays generated on the device, paths counted and recorded there, one read-back, the same text file.
//
// Reads (trace_rays_imageplane.cpp:19-47): argv[1] = the parameter file (default ../par/trace_rays_imageplane.par), outfile, dist, incl,
// plane_phi0 = 0, spin, x0, xmax, Nx, y0, ymax, Ny, tol = TOL, write_step = 10, write_rmin = -1, write_rmax = -1, write_cartesian = 1,
// thetamax = 0 (no theta limit); dx = (xmax - x0) / (Nx - 1).  Euler, rlim = 1.5 dist (:61).
// Reproduced, not fixed: the constructor call (:59) hands `tol` to the parameter that is the plane's azimuth phi and
// `plane_phi0` to the one that is the Raytracer's precision (imageplane.h:26) -- so with plane_phi0 left at 0 the precision is 0 and every
// ray ends on its first step, as in the reference.
// Extensions: --device = 0, --timing (options; the first argument without "--" is the parameter file).
#include <cmath>
#include <iostream>
#include <string>
using namespace std;

#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "imageplane_app.h"
#include "path_recording.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();
    ParameterArgs args(argc, argv);
    const string par_name = args.num_positional() >= 1 ? args[0] : string("../par/trace_rays_imageplane.par");
    ParameterFile par(par_name);

    const string out_name = par.get_parameter<string>("outfile");
    const double dist = par.get_parameter<double>("dist");
    const double incl = par.get_parameter<double>("incl");
    const double plane_phi0 = par.get_parameter<double>("plane_phi0", 0);
    const double spin = par.get_parameter<double>("spin");
    const double x0 = par.get_parameter<double>("x0");
    const double xmax = par.get_parameter<double>("xmax");
    const int Nx = par.get_parameter<int>("Nx");
    const double y0 = par.get_parameter<double>("y0");
    const double ymax = par.get_parameter<double>("ymax");
    const int Ny = par.get_parameter<int>("Ny");
    const double tol = par.get_parameter<double>("tol", 100);      // TOL, raytracer.h
    const double write_step = par.get_parameter<double>("write_step", 10);
    const double write_rmin = par.get_parameter<double>("write_rmin", -1);
    const double write_rmax = par.get_parameter<double>("write_rmax", -1);
    const bool write_cartesian = par.get_parameter<double>("write_cartesian", true);
    const double theta_max = par.get_parameter<double>("thetamax", 0);
    const bool timing = args.key_exists("--timing");

    const double dx = (xmax - x0) / (Nx - 1);
    const double dy = (ymax - y0) / (Ny - 1);

    cout << "*****" << endl;
    cout << "Image plane at  d = " << dist << " , incl = " << incl << endl;
    cout << "Spin a = " << spin << endl;
    cout << "*****" << endl << endl;

    // ImagePlane<double>(dist, incl, x0, xmax, dx, y0, ymax, dy, spin, tol, plane_phi0): the last two land in `phi` and `precision` (:59)
    const kr_imageplane plane = krapp::imageplane(dist, incl, x0, xmax, dx, y0, ymax, dy, spin, tol, plane_phi0);

    kr_params p;
    kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane.cpp:12)
    p.precision = plane_phi0;
    p.integrator = KR_EULER;
    p.theta_max = theta_max;
    p.r_max = 1.5 * dist;
    p.stop_kind = KR_STOP_THETA;
    p.flags = 0;                             // paths carry the reference's arithmetic

    kr_path_spec w;
    memset(&w, 0, sizeof w);
    w.write_step = static_cast<int>(write_step);
    w.write_rmin = write_rmin;
    w.write_rmax = write_rmax;

    // ---- device pipeline ------------------------------------------------------------------------------------------
    krapp::require_device();
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t n = kr_imageplane_count(&plane, nullptr, nullptr);
    if (n <= 0) throw runtime_error("empty ray grid");
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::check(kr_imageplane_init_dev_f64(&plane, rays.get(), n, nullptr), "imageplane_init");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_init = clock.lap_ms();
    cout << "Running raytracer..." << endl;
    const krapp::PathTimes tm = krapp::record_paths_to_text(p, w, write_cartesian, -spin, rays.get(), n, out_name);
    if (timing) krapp::print_path_times(tm, ms_init);
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
