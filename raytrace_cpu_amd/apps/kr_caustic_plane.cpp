// apps/kr_caustic_plane.cpp -- the reference's `caustic_plane` program (src/caustic/caustic_plane.cpp: caustics of the lens map image plane -> a flat
// source plane z_s behind the hole, det J of d(x_s, y_s) / d(x_img, y_img) per pixel) with the ray pipeline resident on the MI355X: the 5-ray bundles
// (or, with bundle_eps_frac = 0, the plain ray grid) are built, traced to a FlatPlaneDestination, gathered into the eight maps and differenced in HBM;
// only the maps come back.  Same parameter file and overrides, same stdout lines, same 9-HDU FITS file (primary + DET_J, SIGN_J, ORDER, HIT_PLANE,
// X_S, Y_S, RDOT_FLIPS, EQUAT_CROSS), written by include/fits_output.h without cfitsio.
//
// Reads (caustic_plane.cpp:68-118): --parfile (default ../par/caustic_plane.par), --outfile | outfile, dist, --incl | incl, plane_phi0 = 0, --spin | spin,
// --z_s | z_s = dist, --r_max | r_max = 4 z_s, x0 = -20, xmax = 20, Nx, y0 = x0, ymax = xmax, Ny = Nx, integrator = rk45 (anything but rk4: a warning,
// then rk45), rk45_tol = 1e-8, --steplim | steplim = -1 (<= 0: the reference's limit, 1e7 steps, 1e5 under RK45), precision = 100,
// --show_progress | show_progress (accepted; the trace is one launch, there is no progress line), bundle_eps_frac = 0.01 (0: grid-neighbour Jacobian).
// Extensions: --arithmetic | KRTRACE_ARITHMETIC = strict (default) | hybrid | fast; --device; --timing.
// Difference: under RK45 a grid pixel exactly at (0, 0) never returns in the reference; here it ends with KR_STATUS_NAN and is no hit.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/raytracer/ray_destination.h"
#include "caustic_app.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process (include/kr_trace.h)
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/caustic_plane.par");
    ParameterFile par(par_name);
    const krapp::CausticSetup s(args, par, [] { return 20.0; }, -1,
                                [](const string& name) { cerr << "Warning: unknown integrator '" << name << "'; using RK45" << endl; });
    const double z_s = args.key_exists("--z_s") ? args.get_parameter<double>("--z_s") : par.get_parameter<double>("z_s", s.dist);
    const double r_max = args.key_exists("--r_max") ? args.get_parameter<double>("--r_max") : par.get_parameter<double>("r_max", 4.0 * z_s);
    const double bundle_eps_frac = par.get_parameter<double>("bundle_eps_frac", 0.01);
    const double incl_rad = s.incl * M_PI / 180.0;

    cout << "Image plane: " << s.img_nx << " x " << s.img_ny << " = " << s.img_nx * s.img_ny << " rays" << endl;
    cout << "Source plane z_s = " << z_s << " rg, r_max = " << r_max << " rg" << endl;
    const bool use_bundles = bundle_eps_frac > 0.0;
    if (use_bundles)
        cout << "Bundle Jacobian mode: eps_frac=" << bundle_eps_frac << "  (eps_x=" << bundle_eps_frac * s.dx << " eps_y=" << bundle_eps_frac * s.dy << " rg)" << endl;
    else
        cout << "Grid-neighbour Jacobian mode" << endl;

    kr_params p = s.params();
    p.r_max = r_max;
    bool default_velocity = false;
    FlatPlaneDestination<double>(incl_rad, s.plane_phi0, z_s).describe(p.stop_kind, p.stop_params, default_velocity);

    kr_source_map sm;
    memset(&sm, 0, sizeof sm);
    sm.kind = 1;
    sm.eps_x = use_bundles ? bundle_eps_frac * s.dx : s.dx;
    sm.eps_y = use_bundles ? bundle_eps_frac * s.dy : s.dy;
    sm.sin_incl = sin(incl_rad); sm.cos_incl = cos(incl_rad);        // the C library's, as source_coords evaluates them (ray_destination.h)
    sm.sin_phi0 = sin(s.plane_phi0); sm.cos_phi0 = cos(s.plane_phi0);

    sm.bundles = use_bundles ? 1 : 0;
    const int64_t n = s.rays(bundle_eps_frac, sm.nx, sm.ny);
    const int64_t npix = static_cast<int64_t>(sm.nx) * sm.ny;
    const kr_imageplane plane = s.plane();
    krapp::require_device();
    krapp::CausticTimes t;
    const unique_ptr<krapp::PinnedDoubles> h = krapp::run_caustic(
        s, p, bundle_eps_frac, n, 8 * npix + 3, {"imageplane_init", [&](void* rays, int64_t m, void*) { return kr_imageplane_init_dev_f64(&plane, rays, m, nullptr); }},
        {"bundles_init", [&](void* rays, int64_t m, void*) { return kr_bundles_init_emit_dev_f64(&plane, bundle_eps_frac, 0.0, 1, 0, rays, m, nullptr); }},
        {{"maps", [&](void* rays, int64_t m, void* maps) { return kr_post_caustic_source_dev_f64(&sm, rays, m, maps, nullptr); }}}, t);
    const double* counts = h->data() + 8 * npix;
    const long hit_count = static_cast<long>(counts[0]), captured_count = static_cast<long>(counts[1]), steplim_count = static_cast<long>(counts[2]);
    cout << hit_count << " rays hit source plane" << endl;
    cout << captured_count << " rays captured by BH" << endl;
    if (steplim_count > 0) cerr << "Warning: " << steplim_count << " rays hit step limit" << endl;

    // ---- FITS (caustic_plane.cpp:397-483) -------------------------------------------------------------------------------------
    krapp::Stopwatch clock;
    const double SENTINEL = 1e30;
    vector<vector<double*>> rows = krapp::plane_rows(h->data(), 8, sm.nx, sm.ny);
    FITSOutput<double> fits(s.out_name);
    fits.create_primary();
    fits.write_comment("Kerr BH caustic / critical curve mapping \xe2\x80\x94 flat source plane");
    fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "caustic_plane");
    fits.write_keyword("DIST", "Observer distance (rg)", s.dist);
    fits.write_keyword("INCL", "Observer inclination (degrees)", s.incl);
    fits.write_keyword("PHI0", "Observer azimuth (radians)", s.plane_phi0);
    fits.write_keyword("SPIN", "Black hole spin parameter a/M", s.spin);
    fits.write_keyword("ZS", "Source plane distance behind BH (rg)", z_s);
    fits.write_keyword("RMAX", "Maximum ray propagation radius (rg)", r_max);
    fits.write_keyword("NRAYS", "Total number of rays", s.img_nx * s.img_ny);
    fits.write_keyword("N_HIT", "Rays that hit source plane", hit_count);
    fits.write_keyword("N_CAP", "Rays captured by BH", captured_count);
    fits.write_keyword("N_SLIM", "Rays that hit step limit", steplim_count);
    fits.write_keyword("EPSFRAC", "Bundle satellite offset fraction (0=grid-neighbour)", bundle_eps_frac);

    auto write_plane = [&](int k, const char* extname, std::initializer_list<const char*> comments) {
        fits.write_image(rows[k].data(), s.img_nx, s.img_ny, false);
        fits.set_ext_name(extname);
        for (const char* c : comments) fits.write_comment(c);
        if (k == 0) fits.write_keyword("SENTINL", "Value at image-order boundaries (also critical curves)", SENTINEL);
        krapp::write_axis_keywords(fits, s);
    };
    write_plane(0, "DET_J", {"det(J) of image-plane->source-plane map; zero-crossings = critical curves", "NaN: ray did not hit plane; SENTINL: image-order boundary"});
    write_plane(1, "SIGN_J", {"Sign of det(J): +1 or -1; 0 at order boundaries or undefined"});
    write_plane(2, "ORDER", {"Image order: 0=direct, 1=first photon ring; -1=did not hit plane"});
    write_plane(3, "HIT_PLANE", {"1 = ray reached source plane; 0 = captured or near-side escape"});
    write_plane(4, "X_S", {"East coordinate on source plane (rg); NaN if ray did not hit plane"});
    write_plane(5, "Y_S", {"North coordinate on source plane (rg); NaN if ray did not hit plane"});
    write_plane(6, "RDOT_FLIPS", {"Radial turning-point count during propagation"});
    write_plane(7, "EQUAT_CROSS", {"Equatorial-plane (theta=pi/2) crossing count during propagation"});
    fits.close();

    if (s.timing) krapp::print_source_timing(t, clock.lap_ms());
    cout << "Written to " << s.out_name << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
