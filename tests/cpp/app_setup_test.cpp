// tests/cpp/app_setup_test.cpp -- what raytrace_cpu_amd/apps/imageplane_app.h makes of a parameter file and --key=value arguments, for
// tests/test_app_setup.py: every field of the kr_imageplane, of the kr_params of params(KR_RK45), of the kr_image_bins and of the AxisInfo as
// `name value` lines at 17 significant digits.  No device is needed: kr_params_default and kr_imageplane_count are host code.
//   app_setup_test --parfile=FILE [--key=value ...]
#include <iomanip>
#include <iostream>
using namespace std;

#include "../../raytrace_cpu_amd/apps/imageplane_app.h"

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt);
    const kr_imageplane plane = s.plane();
    const kr_params p = s.params(KR_RK45);
    const kr_image_bins b = s.image_bins();
    const krapp::AxisInfo& ax = s.ax;
    cout << setprecision(17);
#define SHOW(obj, field) cout << #obj "." #field " " << obj.field << "\n"
    SHOW(plane, dist); SHOW(plane, inc_deg); SHOW(plane, x0); SHOW(plane, xmax); SHOW(plane, dx); SHOW(plane, y0); SHOW(plane, ymax); SHOW(plane, dy);
    SHOW(plane, spin); SHOW(plane, phi0); SHOW(plane, precision);
    SHOW(p, spin); SHOW(p, horizon); SHOW(p, precision); SHOW(p, theta_precision); SHOW(p, max_tstep); SHOW(p, maxtstep_rlim); SHOW(p, max_phistep);
    SHOW(p, rk45_tol); SHOW(p, r_max); SHOW(p, theta_max);
    for (int i = 0; i < 4; ++i) cout << "p.stop_params" << i << " " << p.stop_params[i] << "\n";
    SHOW(p, integrator); SHOW(p, stop_kind); SHOW(p, steplim); SHOW(p, flags);
    SHOW(b, x0); SHOW(b, y0); SHOW(b, img_dx); SHOW(b, img_dy); SHOW(b, r_isco); SHOW(b, r_disc); SHOW(b, q1); SHOW(b, rb1); SHOW(b, q2); SHOW(b, rb2); SHOW(b, q3);
    SHOW(b, img_nx); SHOW(b, img_ny); SHOW(b, flip_image); SHOW(b, pad);
    SHOW(ax, x0); SHOW(ax, xmax); SHOW(ax, dx); SHOW(ax, y0); SHOW(ax, ymax); SHOW(ax, dy); SHOW(ax, img_nx); SHOW(ax, img_ny);
#undef SHOW
    cout << "rays " << kr_imageplane_count(&plane, nullptr, nullptr) << "\n";
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "app_setup.par", program); }
