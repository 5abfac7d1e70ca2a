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

#include "../host/include/kerr.h"
#include "../host/raytracer/ray_destination.h"
#include "caustic_app.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process (include/kr_trace.h)
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/caustic_discplane.par");
    ParameterFile par(par_name);
    double r_disc = 0;
    const krapp::CausticSetup s(args, par, [&] { return r_disc = par.get_parameter<double>("r_disc"); }, 0, [](const string& name) {
        if (name == "euler") cerr << "Warning: Euler integrator does not support RayDestination; using RK45" << endl;
    });
    const double bundle_eps_frac = par.get_parameter<double>("bundle_eps_frac", 0.01);

    const double r_isco = kerr_isco<double>(s.spin, +1);
    cout << "ISCO at r = " << r_isco << endl;
    cout << "Image plane: " << s.img_nx << " x " << s.img_ny << " = " << s.img_nx * s.img_ny << " rays" << endl;
    const bool use_bundles = bundle_eps_frac > 0.0;
    if (use_bundles)
        cout << "Bundle Jacobian mode: eps_frac=" << bundle_eps_frac << "  (eps_x=" << bundle_eps_frac * s.dx << " eps_y=" << bundle_eps_frac * s.dy << " rg)" << endl;
    else
        cout << "Grid-neighbour Jacobian mode" << endl;

    kr_caustic_map cm;
    memset(&cm, 0, sizeof cm);
    cm.r_isco = r_isco; cm.r_disc = r_disc;
    cm.eps_x = use_bundles ? bundle_eps_frac * s.dx : s.dx;
    cm.eps_y = use_bundles ? bundle_eps_frac * s.dy : s.dy;
    cm.bundles = use_bundles ? 1 : 0;
    const int64_t n = s.rays(bundle_eps_frac, cm.nx, cm.ny);
    const int64_t npix = static_cast<int64_t>(cm.nx) * cm.ny;

    kr_params p = s.params();
    p.r_max = 1.1 * s.dist;
    bool default_velocity = false;
    DiscWithISCODestination<double>(r_isco, r_disc).describe(p.stop_kind, p.stop_params, default_velocity);

    const kr_imageplane plane = s.plane();
    krapp::CausticTimes t;
    const unique_ptr<krapp::PinnedDoubles> h = krapp::run_caustic(
        s, p, bundle_eps_frac, n, 9 * npix + 7,
        {"imageplane_init + redshift_start", [&](void* rays, int64_t m, void*) { return kr_imageplane_init_emit_dev_f64(&plane, 0, 1, 0.0, 1, 0, rays, m, nullptr); }},
        {"bundles_init + redshift_start", [&](void* rays, int64_t m, void*) { return kr_bundles_init_emit_dev_f64(&plane, bundle_eps_frac, 0.0, 1, 0, rays, m, nullptr); }},
        {{"redshift + maps", [&](void* rays, int64_t m, void* maps) { return kr_post_caustic_disc_dev_f64(-s.spin, 1, &cm, rays, m, maps, nullptr); }},
         {"suppression", [&](void*, int64_t, void* maps) { return kr_caustic_suppress_dev_f64(&cm, maps, nullptr); }}},
        t);

    const double* counts = h->data() + 9 * npix;
    const long disc_count = static_cast<long>(counts[0]);
    cout << disc_count << " rays hit the disc" << endl;
    cout << "  -> horizon=" << static_cast<long>(counts[1]) << " rlim=" << static_cast<long>(counts[2]) << " steplim=" << static_cast<long>(counts[3])
         << " out-of-range=" << static_cast<long>(counts[4]) << " other=" << static_cast<long>(counts[5]) << endl;
    cout << static_cast<long>(counts[6]) << " alternating-sign pixels suppressed (branch boundary)" << endl;

    // ---- FITS (caustic_discplane.cpp:497-598) -------------------------------------------------------------------------
    krapp::Stopwatch clock;
    const double SENTINEL = 1e30;
    vector<vector<double*>> rows = krapp::plane_rows(h->data(), 9, cm.nx, cm.ny);
    FITSOutput<double> fits(s.out_name);
    fits.create_primary();
    fits.write_comment("Kerr spacetime caustic / critical curve mapping (image plane)");
    fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "caustic_discplane");
    fits.write_keyword("DIST", "Distance to image plane (rg)", s.dist);
    fits.write_keyword("INCL", "Inclination (degrees)", s.incl);
    fits.write_keyword("SPIN", "Black hole spin parameter a/M", s.spin);
    fits.write_keyword("ISCO", "Innermost stable circular orbit (rg)", r_isco);
    fits.write_keyword("RDISC", "Outer disc radius (rg)", r_disc);
    fits.write_keyword("NRAYS", "Total number of rays", s.img_nx * s.img_ny);
    fits.write_keyword("DISC_N", "Rays that hit the disc", disc_count);
    fits.write_keyword("EPSFRAC", "Bundle satellite offset fraction (0=grid-neighbour)", bundle_eps_frac);

    auto write_plane = [&](int k, const char* extname, const char* what, const char* pixval, const char* pixunit) {
        fits.write_image(rows[k].data(), s.img_nx, s.img_ny, false);
        fits.set_ext_name(extname);
        fits.write_comment(what);
        fits.write_keyword("AXIS1", "Quantity along X axis", "Image plane X (rg)");
        fits.write_keyword("AXIS2", "Quantity along Y axis", "Image plane Y (rg)");
        krapp::write_axis_keywords(fits, s);
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

    if (s.timing)
        cout << "timing: rays " << t.stats.rays_traced << " steps " << t.stats.steps_total << " | init+redshift_start " << t.init << " ms | trace " << t.trace
             << " ms (kernel " << t.stats.kernel_ms << ") | redshift+maps " << t.steps[0] << " ms | suppress " << t.steps[1] << " ms | readback " << t.readback
             << " ms | FITS file " << ms_fits << " ms" << endl;
    cout << "Done. Output: " << s.out_name << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
