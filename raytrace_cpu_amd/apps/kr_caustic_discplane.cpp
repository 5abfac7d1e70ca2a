// apps/kr_caustic_discplane.cpp -- the reference's `caustic_discplane` program (src/caustic/caustic_discplane.cpp: critical curves of the
// lens map image plane -> disc, det J of d(x_disc, y_disc) / d(x_img, y_img) per pixel) with the ray pipeline resident on the MI355X: the 5-ray
// bundles (or, with bundle_eps_frac = 0, the plain ray grid) are built, traced to the disc, redshifted, gathered into the nine maps and filtered in
// HBM; only the maps come back.  Same parameter file and overrides, same stdout lines, same 10-HDU FITS file (primary + DET_J, SIGN_J, ORDER,
// HIT, RADIUS, PHI, X_DISC, Y_DISC, REDSHIFT), written by include/fits_output.h without cfitsio.
//
// Reads (caustic_discplane.cpp:73-110): --parfile (default ../par/caustic_discplane.par), --outfile | outfile, dist, --incl | incl, plane_phi0 = 0,
// --spin | spin, r_disc, x0 = -r_disc, xmax = r_disc, Nx, y0 = x0, ymax = xmax, Ny = Nx, integrator = rk45 (euler: a warning, then rk45),
// rk45_tol = 1e-8, precision = 100, --show_progress | show_progress (accepted; the trace is one launch, there is no progress line),
// bundle_eps_frac = 0.01 (0: grid-neighbour Jacobian).
// Extensions: --arithmetic | KRTRACE_ARITHMETIC = strict (default, for every integrator: det J amplifies end-point differences by 1e2-1e3) | hybrid |
// fast; --steplim | steplim = 0 (the reference's limit: 1e7 steps, 1e5 under RK45): a DiscWithISCODestination does not stop a photon trapped inside
// the ISCO, and one such ray holds the launch until the limit; --device; --timing.
// Difference: under RK45 a grid pixel exactly at (0, 0) never returns in the reference; here it ends with KR_STATUS_NAN and is no hit.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/fits_output.h"
#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "../host/raytracer/ray_destination.h"
#include "app_common.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process (include/kr_trace.h)
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/caustic_discplane.par");
    ParameterFile par(par_name);

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    const double dist = par.get_parameter<double>("dist");
    const double incl = args.key_exists("--incl") ? args.get_parameter<double>("--incl") : par.get_parameter<double>("incl");
    const double plane_phi0 = par.get_parameter<double>("plane_phi0", 0);
    const double spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
    const double r_disc = par.get_parameter<double>("r_disc");
    const double x0 = par.get_parameter<double>("x0", -1 * r_disc), xmax = par.get_parameter<double>("xmax", r_disc);
    const int Nx = par.get_parameter<int>("Nx");
    const double y0 = par.get_parameter<double>("y0", x0), ymax = par.get_parameter<double>("ymax", xmax);
    const int Ny = par.get_parameter<int>("Ny", Nx);
    const string integ = par.get_parameter<string>("integrator", "rk45");
    const double rk45_tol = par.get_parameter<double>("rk45_tol", 1e-8);
    const double precision = par.get_parameter<double>("precision", 100);
    (void) (args.key_exists("--show_progress") ? args.get_parameter<int>("--show_progress") : par.get_parameter<int>("show_progress", 1));
    const double bundle_eps_frac = par.get_parameter<double>("bundle_eps_frac", 0.01);
    const int steplim = args.key_exists("--steplim") ? args.get_parameter<int>("--steplim") : par.get_parameter<int>("steplim", 0);
    const string arith = args.key_exists("--arithmetic") ? args.get_parameter<string>("--arithmetic") : krapp::arithmetic_from_env();
    const bool timing = args.key_exists("--timing");

    int integrator = KR_RK45;
    if (integ == "euler") cerr << "Warning: Euler integrator does not support RayDestination; using RK45" << endl;
    else if (integ == "rk4") integrator = KR_RK4;

    const double dx = (xmax - x0) / Nx, dy = (ymax - y0) / Ny;
    const int img_nx = Nx + 1, img_ny = Ny + 1;             // fencepost: the ray grid has one more point per axis than steps
    const double r_isco = kerr_isco<double>(spin, +1);
    cout << "ISCO at r = " << r_isco << endl;
    cout << "Image plane: " << img_nx << " x " << img_ny << " = " << img_nx * img_ny << " rays" << endl;
    const bool use_bundles = bundle_eps_frac > 0.0;
    if (use_bundles)
        cout << "Bundle Jacobian mode: eps_frac=" << bundle_eps_frac << "  (eps_x=" << bundle_eps_frac * dx << " eps_y=" << bundle_eps_frac * dy << " rg)" << endl;
    else
        cout << "Grid-neighbour Jacobian mode" << endl;

    kr_imageplane plane;
    memset(&plane, 0, sizeof plane);
    plane.dist = dist;
    plane.inc_deg = incl;
    plane.x0 = x0; plane.xmax = xmax; plane.dx = dx;
    plane.y0 = y0; plane.ymax = ymax; plane.dy = dy;
    plane.spin = spin;
    plane.phi0 = plane_phi0;
    plane.precision = precision;

    int32_t nx = 0, ny = 0;
    const int64_t n = use_bundles ? kr_bundles_count(&plane, &nx, &ny) : kr_imageplane_count(&plane, &nx, &ny);
    if (n <= 0) throw runtime_error("empty ray grid");
    // the reference indexes its (Nx + 1) x (Ny + 1) maps with the ray source's own counts; where the two disagree it writes out of bounds
    if (nx != img_nx || ny != img_ny) throw runtime_error("the ray source's grid (" + to_string(nx) + " x " + to_string(ny) + ") is not (Nx + 1) x (Ny + 1)");

    kr_caustic_map cm;
    memset(&cm, 0, sizeof cm);
    cm.r_isco = r_isco; cm.r_disc = r_disc;
    cm.eps_x = use_bundles ? bundle_eps_frac * dx : dx;
    cm.eps_y = use_bundles ? bundle_eps_frac * dy : dy;
    cm.nx = nx; cm.ny = ny;
    cm.bundles = use_bundles ? 1 : 0;

    kr_params p;
    kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane_bundles.h:151)
    p.precision = precision;
    p.integrator = integrator;
    if (integrator == KR_RK45) p.rk45_tol = rk45_tol;
    p.r_max = 1.1 * dist;
    p.steplim = steplim;
    bool default_velocity = false;
    DiscWithISCODestination<double>(r_isco, r_disc).describe(p.stop_kind, p.stop_params, default_velocity);
    p.flags = arith.empty() ? 0 : krapp::arithmetic_flags(arith, integrator);

    // ---- device pipeline ------------------------------------------------------------------------------------------
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t npix = (int64_t) nx * ny, words = 9 * npix + 7;
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::DeviceBuffer maps(words * (int64_t) sizeof(double));
    if (use_bundles)
        krapp::check(kr_bundles_init_emit_dev_f64(&plane, bundle_eps_frac, 0.0, 1, 0, rays.get(), n, nullptr), "bundles_init + redshift_start");
    else
        krapp::check(kr_imageplane_init_emit_dev_f64(&plane, 0, 1, 0.0, 1, 0, rays.get(), n, nullptr), "imageplane_init + redshift_start");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_init = clock.lap_ms();
    static const char* names[] = {"", "Running raytracer (RK4)...", "Running raytracer (RK45/DOPRI5)..."};
    cout << names[integrator] << endl;
    kr_stats st;
    krapp::check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &st), "trace");
    const double ms_trace = clock.lap_ms();
    krapp::check(kr_post_caustic_disc_dev_f64(-spin, 1, &cm, rays.get(), n, maps.get(), nullptr), "redshift + maps");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_post = clock.lap_ms();
    krapp::check(kr_caustic_suppress_dev_f64(&cm, maps.get(), nullptr), "suppression");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_suppress = clock.lap_ms();
    krapp::PinnedDoubles h(words);
    krapp::check(kr_memcpy_d2h(h.data(), maps.get(), words * (int64_t) sizeof(double)), "d2h");
    const double ms_d2h = clock.lap_ms();

    const double* counts = h.data() + 9 * npix;
    const long disc_count = static_cast<long>(counts[0]);
    cout << disc_count << " rays hit the disc" << endl;
    cout << "  -> horizon=" << static_cast<long>(counts[1]) << " rlim=" << static_cast<long>(counts[2]) << " steplim=" << static_cast<long>(counts[3])
         << " out-of-range=" << static_cast<long>(counts[4]) << " other=" << static_cast<long>(counts[5]) << endl;
    cout << static_cast<long>(counts[6]) << " alternating-sign pixels suppressed (branch boundary)" << endl;

    // ---- FITS (caustic_discplane.cpp:497-598) -------------------------------------------------------------------------
    const double SENTINEL = 1e30;
    vector<vector<double*>> rows(9, vector<double*>(static_cast<size_t>(nx)));
    for (int k = 0; k < 9; ++k)
        for (int ix = 0; ix < nx; ++ix) rows[k][ix] = h.data() + k * npix + static_cast<int64_t>(ix) * ny;

    FITSOutput<double> fits(out_name);
    fits.create_primary();
    fits.write_comment("Kerr spacetime caustic / critical curve mapping (image plane)");
    fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "caustic_discplane");
    fits.write_keyword("DIST", "Distance to image plane (rg)", dist);
    fits.write_keyword("INCL", "Inclination (degrees)", incl);
    fits.write_keyword("SPIN", "Black hole spin parameter a/M", spin);
    fits.write_keyword("ISCO", "Innermost stable circular orbit (rg)", r_isco);
    fits.write_keyword("RDISC", "Outer disc radius (rg)", r_disc);
    fits.write_keyword("NRAYS", "Total number of rays", img_nx * img_ny);
    fits.write_keyword("DISC_N", "Rays that hit the disc", disc_count);
    fits.write_keyword("EPSFRAC", "Bundle satellite offset fraction (0=grid-neighbour)", bundle_eps_frac);

    auto write_plane = [&](int k, const char* extname, const char* what, const char* pixval, const char* pixunit) {
        fits.write_image(rows[k].data(), img_nx, img_ny, false);
        fits.set_ext_name(extname);
        fits.write_comment(what);
        fits.write_keyword("AXIS1", "Quantity along X axis", "Image plane X (rg)");
        fits.write_keyword("AXIS2", "Quantity along Y axis", "Image plane Y (rg)");
        fits.write_keyword("X0", "Start of X axis (rg)", x0);
        fits.write_keyword("XMAX", "End of X axis (rg)", xmax);
        fits.write_keyword("DX", "X step (rg)", dx);
        fits.write_keyword("NX", "Number of pixels in X", img_nx);
        fits.write_keyword("Y0", "Start of Y axis (rg)", y0);
        fits.write_keyword("YMAX", "End of Y axis (rg)", ymax);
        fits.write_keyword("DY", "Y step (rg)", dy);
        fits.write_keyword("NY", "Number of pixels in Y", img_ny);
        if (k == 0) fits.write_keyword("SENTINL", "Value used at image-order boundaries (also critical curves)", SENTINEL);
        if (pixval) {
            fits.write_keyword("PIXVAL", "Pixel value quantity", pixval);
            fits.write_keyword("PIXUNIT", "Pixel value unit", pixunit);
        }
    };
    write_plane(0, "DET_J", "Jacobian determinant det(d(x_disc,y_disc)/d(x,y)); zero-crossings = critical curves", nullptr, nullptr);
    write_plane(1, "SIGN_J", "Sign of Jacobian determinant (+1/-1/0); parity flips at critical curves", nullptr, nullptr);
    write_plane(2, "ORDER", "Image order (rdot_flips): 0=direct, 1=first photon ring, -1=no hit", nullptr, nullptr);
    write_plane(3, "HIT", "1 if ray hit disc, 0 otherwise", nullptr, nullptr);
    write_plane(4, "RADIUS", "Disc emission radius (rg); 0 if no disc hit", "RADIUS", "RG");
    write_plane(5, "PHI", "Disc azimuthal angle (radians, range [-pi,pi]); 0 if no disc hit", "PHI", "RAD");
    write_plane(6, "X_DISC", "Disc Cartesian x coordinate (rg) = r*cos(phi); 0 if no disc hit", "X_DISC", "RG");
    write_plane(7, "Y_DISC", "Disc Cartesian y coordinate (rg) = r*sin(phi); 0 if no disc hit", "Y_DISC", "RG");
    write_plane(8, "REDSHIFT", "Photon energy ratio E_obs/E_emit (gravitational + Doppler); 0 if no disc hit", "REDSHIFT", "E_OBS/E_EMIT");
    fits.close();
    const double ms_fits = clock.lap_ms();

    if (timing)
        cout << "timing: rays " << st.rays_traced << " steps " << st.steps_total << " | init+redshift_start " << ms_init << " ms | trace " << ms_trace
             << " ms (kernel " << st.kernel_ms << ") | redshift+maps " << ms_post << " ms | suppress " << ms_suppress << " ms | readback " << ms_d2h
             << " ms | FITS file " << ms_fits << " ms" << endl;
    cout << "Done. Output: " << out_name << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
