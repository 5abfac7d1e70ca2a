// apps/kr_volume_spectrum.cpp -- from corona geometry to the observed spectrum and reverberation response of the volume it illuminates, without leaving
// the device: the rays of a grid of point sources are traced and binned into an (r, theta, phi) grid as they step (kr_trace_volume_dev_f64, as
// kr_volume_map does); the map becomes a volume emissivity and a flash delay per cell (the expression source_tracer.cpp:257-258 comments out; O(cells),
// on the host); an image plane is built on the device with redshift_start(0, reverse = 1) and its rays are marched back through the volume, gathering
// j l E^3 exp(-tau) into an energy spectrum, an energy-time response and a per-pixel image (kr_trace_observe_dev_f64; include/kr_trace.h has the rule).
// This is SourceTracer::propagate_source driven as sourcetracer_imageplane.cpp / src/outflow/outflow_ent.cpp drive it, restated against the live trace
// loop, with the mapper's grid in place of the hard-wired shell.
//
// Reads: --parfile (default ../par/volume_spectrum.par), --outfile | outfile, --spin | spin, --timing, --device = 0, and
//   the source grid, as kr_volume_map reads it: source[4] (--source_h overrides source[1]), source_h_max = source[1] and Nsource = 1 (Nsource point
//     sources at heights from source[1] to source_h_max, all adding into one map), V = 0, cosalpha0 = -0.995, cosalphamax = 0.995, dcosalpha, beta0 = -pi,
//     betamax = pi, dbeta, r0, rmax, Nr, Ntheta, Nphi = 1, logbin_r = false, theta_max = pi / 2, r_esc = 1000, mode = 0, --integrator | integrator = rk4;
//   the plane, as outflow_ent.cpp:31-41 names it: dist, incl (degrees), plane_phi0 = 0, x0, xmax, Nx, y0, ymax, Ny (dx = (xmax - x0) / (Nx - 1)); its
//     rays run to 1.5 dist (run_source_trace(1.5 * dist));
//   the bins (:42-48): en0, enmax, Nen, logbin_en = false, t0 = 0, tmax = 0, Nt = 0 (no response);
//   gamma = 2 (the emissivity's power of the mean energy shift), kappa = 0 (a uniform absorption per unit proper length; 0: optically thin).
// The emitters are the mapper's observers: orbits of V = 1 / (a + r sin(theta) sqrt(r sin(theta))).
//
// outfile: FITS, HDUs PRIMARY, ENERGY (Nen bin centres), SPECTRUM (Nen), HITS (Nen), RESPONSE (NAXIS1 = Nt by NAXIS2 = Nen; 1 x Nen zeros when
// Nt = 0), IMAGE (NAXIS1 = Ny by NAXIS2 = Nx, pixel [ix][iy]: the ray's total).  The primary header carries every parameter, the number of source rays
// and the six tallies rows / in_grid / lit / contributions / bad_g / degenerate.
#include <algorithm>
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/fits_output.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "app_common.h"
#include "imageplane_app.h"
#include "volume_app.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/volume_spectrum.par");
    ParameterFile par(par_name);

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    const double spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
    const bool timing = args.key_exists("--timing");
    // the source grid
    const double V = par.get_parameter<double>("V", 0);
    kr_pointsource src0 = krapp::read_point_source(par, spin, V);
    if (args.key_exists("--source_h")) src0.pos[1] = args.get_parameter<double>("--source_h");
    const double* source = src0.pos;
    const double source_h_max = par.get_parameter<double>("source_h_max", source[1]);
    const int Nsource = par.get_parameter<int>("Nsource", 1);
    const krapp::VolumeGridPar grid(args, par);
    const int Nr = grid.Nr, Ntheta = grid.Ntheta, Nphi = grid.Nphi;
    // the plane
    const double dist = par.get_parameter<double>("dist");
    const double incl = par.get_parameter<double>("incl");
    const double plane_phi0 = par.get_parameter<double>("plane_phi0", 0);
    const double x0 = par.get_parameter<double>("x0");
    const double xmax = par.get_parameter<double>("xmax");
    const int Nx = par.get_parameter<int>("Nx");
    const double y0 = par.get_parameter<double>("y0");
    const double ymax = par.get_parameter<double>("ymax");
    const int Ny = par.get_parameter<int>("Ny");
    // the bins
    const double en0 = par.get_parameter<double>("en0");
    const double enmax = par.get_parameter<double>("enmax");
    const int Nen = par.get_parameter<int>("Nen");
    const bool logbin_en = par.get_parameter<bool>("logbin_en", false);
    const double t0 = par.get_parameter<double>("t0", 0);
    const double tmax = par.get_parameter<double>("tmax", 0);
    const int Nt = par.get_parameter<int>("Nt", 0);
    const double gamma = par.get_parameter<double>("gamma", 2);
    const double kappa = par.get_parameter<double>("kappa", 0);
    if (Nx < 2 || Ny < 2) throw runtime_error("Nx and Ny must be at least 2");
    if (Nen < 1 || Nt < 0 || Nsource < 1) throw runtime_error("Nen and Nsource must be at least 1, Nt must not be negative");

    const kr_volume_map m = grid.map();

    kr_observe_bins b;
    memset(&b, 0, sizeof b);
    b.en0 = en0; b.den = logbin_en ? exp(log(enmax / en0) / Nen) : (enmax - en0) / Nen;
    b.t0 = t0; b.dt = Nt > 0 ? (tmax - t0) / Nt : 0;
    b.nen = Nen; b.nt = Nt; b.logbin_en = logbin_en ? 1 : 0;

    const kr_params p_source = grid.params(spin);      // both traces ride the strict recording loop
    kr_params p_plane;
    kr_params_default(&p_plane, -1 * spin);      // as stored by the Raytracer of an ImagePlane (imageplane.cpp:12)
    p_plane.integrator = p_source.integrator;
    p_plane.r_max = 1.5 * dist;
    p_plane.stop_kind = KR_STOP_THETA;
    p_plane.flags = 0;

    const kr_imageplane plane = krapp::imageplane(dist, incl, x0, xmax, (xmax - x0) / (Nx - 1), y0, ymax, (ymax - y0) / (Ny - 1), spin, plane_phi0, 100);

    krapp::require_device();             // before the output file is created
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch clock;

    // 1. the map: every source adds into it
    const int64_t ncell = (int64_t) Nr * Ntheta * Nphi, map_words = 3 * ncell + 4;
    krapp::DeviceBuffer map(map_words * (int64_t) sizeof(double));
    map.zero();
    int64_t num_rays = 0;
    double ms_map = 0;
    for (int is = 0; is < Nsource; ++is) {
        kr_pointsource src = src0;
        if (Nsource > 1) src.pos[1] = source[1] + is * (source_h_max - source[1]) / (Nsource - 1);
        const int64_t n = kr_pointsource_count(&src, nullptr, nullptr);
        if (n <= 0) throw runtime_error("empty source ray grid");
        krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
        krapp::check(kr_pointsource_init_emit_dev_f64(&src, 0, 1, V, 0, 0, rays.get(), n, nullptr), "pointsource_init + redshift_start");
        kr_stats st;
        krapp::check(kr_trace_volume_dev_f64(&p_source, &m, rays.get(), n, map.get(), nullptr, &st), "volume map");
        num_rays += st.rays_traced;
        ms_map += st.kernel_ms;
    }
    vector<double> h(static_cast<size_t>(map_words));
    krapp::check(kr_memcpy_d2h(h.data(), map.get(), map_words * (int64_t) sizeof(double)), "d2h");
    const double ms_sources = clock.lap_ms();

    // 2. emissivity and delay per cell: count / (num_rays volume) mean_g^-gamma and mean_time (source_tracer.cpp:257-258; calculate_volume, mapper.cpp:311-338)
    vector<double> emis(static_cast<size_t>(ncell), 0.0), delay(static_cast<size_t>(ncell), 0.0), kap(static_cast<size_t>(ncell), kappa);
    for (int ir = 0; ir < Nr; ++ir) {
        for (int itheta = 0; itheta < Ntheta; ++itheta) {
            const double volume = krapp::cell_volume(m, spin, ir, itheta);
            for (int iphi = 0; iphi < Nphi; ++iphi) {
                const size_t c = ((size_t) ir * Ntheta + itheta) * Nphi + iphi;
                const double count = h[c];
                if (!(count > 0)) continue;
                delay[c] = h[ncell + c] / count;
                if (volume > 0 && std::isfinite(volume)) emis[c] = count / ((double) num_rays * volume) * pow(h[2 * ncell + c] / count, -1 * gamma);
            }
        }
    }

    // 3. + 4. the plane, observed
    const int64_t n = kr_imageplane_count(&plane, nullptr, nullptr);
    if (n != (int64_t) Nx * Ny) throw runtime_error("the image plane does not have Nx * Ny rays (choose x0, xmax, Nx so that (xmax - x0) / dx is whole)");
    const int64_t out_words = 2 * (int64_t) Nen + (int64_t) Nen * Nt + 6;
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64)), d_out(out_words * (int64_t) sizeof(double)), d_image(n * (int64_t) sizeof(double));
    krapp::DeviceBuffer d_emis(ncell * (int64_t) sizeof(double)), d_delay(ncell * (int64_t) sizeof(double)), d_kappa(ncell * (int64_t) sizeof(double));
    d_out.zero();
    krapp::check(kr_memcpy_h2d(d_emis.get(), emis.data(), ncell * (int64_t) sizeof(double)), "h2d");
    krapp::check(kr_memcpy_h2d(d_delay.get(), delay.data(), ncell * (int64_t) sizeof(double)), "h2d");
    krapp::check(kr_memcpy_h2d(d_kappa.get(), kap.data(), ncell * (int64_t) sizeof(double)), "h2d");
    krapp::check(kr_imageplane_init_emit_dev_f64(&plane, 0, 1, 0.0, 1, 0, rays.get(), n, nullptr), "ImagePlane + redshift_start");
    kr_volume_map mo = m;
    mo.reverse = 1;                      // the camera's rays run backwards
    kr_stats st;
    krapp::check(kr_trace_observe_dev_f64(&p_plane, &mo, &b, d_emis.get(), kappa > 0 ? d_kappa.get() : nullptr, d_delay.get(), rays.get(), n, d_out.get(), d_image.get(),
                                          nullptr, &st), "observe");
    vector<double> out(static_cast<size_t>(out_words)), image(static_cast<size_t>(n));
    krapp::check(kr_memcpy_d2h(out.data(), d_out.get(), out_words * (int64_t) sizeof(double)), "d2h");
    krapp::check(kr_memcpy_d2h(image.data(), d_image.get(), n * (int64_t) sizeof(double)), "d2h");
    const double ms_observe = clock.lap_ms();

    vector<double> energy(static_cast<size_t>(Nen));
    for (int i = 0; i < Nen; ++i) energy[i] = logbin_en ? en0 * pow(b.den, i + 0.5) : en0 + b.den * (i + 0.5);
    vector<double> no_response(static_cast<size_t>(Nen), 0.0);
    const double* tally = out.data() + 2 * (size_t) Nen + (size_t) Nen * Nt;

    FITSOutput<double> fits(out_name);
    fits.create_primary();
    fits.write_comment("Kerr BH: spectrum, response and image of an illuminated volume along camera rays");
    fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "kr_volume_spectrum");
    fits.write_keyword("SPIN", "Black hole spin parameter a/M", spin);
    fits.write_keyword("SOURCE_H", "Height of the (first) point source (rg)", source[1]);
    fits.write_keyword("SRC_HMAX", "Height of the last point source (rg)", Nsource > 1 ? source_h_max : source[1]);
    fits.write_keyword("NSOURCE", "Point sources", Nsource);
    fits.write_keyword("SOURCE_T", "Source polar angle", source[2]);
    fits.write_keyword("SOURCE_P", "Source azimuth", source[3]);
    fits.write_keyword("V", "Source angular velocity", V);
    krapp::write_grid_keywords(fits, grid, m);
    fits.write_keyword("THETAMAX", "Polar angle at which the source trace stops", grid.theta_max);
    fits.write_keyword("NTHETA", "Polar cells, from theta = 0", Ntheta);
    fits.write_keyword("NPHI", "Azimuthal cells, from phi = -pi", Nphi);
    fits.write_keyword("R_ESC", "Radius at which the source trace stops (rg)", grid.r_esc);
    fits.write_keyword("MODE", "0 = one deposit per passage of a cell, 1 = per step", grid.mode);
    fits.write_keyword("INTEGRAT", "Integrator of both traces", grid.integ);
    fits.write_keyword("DIST", "Distance of the image plane (rg)", dist);
    fits.write_keyword("INCL", "Inclination of the image plane (degrees)", incl);
    fits.write_keyword("PHI0", "Azimuth of the image plane", plane_phi0);
    fits.write_keyword("X0", "Image plane x0", x0);
    fits.write_keyword("XMAX", "Image plane xmax", xmax);
    fits.write_keyword("NX", "Image plane pixels in x", Nx);
    fits.write_keyword("Y0", "Image plane y0", y0);
    fits.write_keyword("YMAX", "Image plane ymax", ymax);
    fits.write_keyword("NY", "Image plane pixels in y", Ny);
    fits.write_keyword("EN0", "First energy edge", en0);
    fits.write_keyword("ENMAX", "Last energy edge", enmax);
    fits.write_keyword("NEN", "Energy bins", Nen);
    fits.write_keyword("DEN", "Energy bin width, or ratio between edges with LOGBIN_E", b.den);
    fits.write_keyword("LOGBIN_E", "1 = logarithmic energy bins", logbin_en ? 1 : 0);
    fits.write_keyword("T0", "First time edge", t0);
    fits.write_keyword("TMAX", "Last time edge", tmax);
    fits.write_keyword("NT", "Time bins (0 = no response)", Nt);
    fits.write_keyword("GAMMA", "Emissivity = count / (rays volume) mean_g^-GAMMA", gamma);
    fits.write_keyword("KAPPA", "Uniform absorption per unit proper length (0 = thin)", kappa);
    fits.write_keyword("NUM_RAYS", "Source rays traced", (long) num_rays);
    fits.write_keyword("PIX_RAYS", "Camera rays traced", (long) st.rays_traced);
    fits.write_keyword("ROWS", "Camera ray steps that could contribute", (long) llround(tally[0]));
    fits.write_keyword("IN_GRID", "... of them inside the grid", (long) llround(tally[1]));
    fits.write_keyword("LIT", "... in a cell that emits or absorbs", (long) llround(tally[2]));
    fits.write_keyword("CONTRIB", "Contributions: steps that added to a ray's total", (long) llround(tally[3]));
    fits.write_keyword("BAD_G", "Emitting steps dropped for an energy shift <= 0 or not finite", (long) llround(tally[4]));
    fits.write_keyword("DEGENER", "Steps dropped for a degenerate length (polar reflection)", (long) llround(tally[5]));
    struct Plane { const char* name; const char* what; double* data; int n1, n2; };
    const Plane planes[5] = {
        {"ENERGY", "Centre of the energy bin (E observed / E emitted)", energy.data(), Nen, 1},
        {"SPECTRUM", "Sum of j l E^3 exp(-tau) per energy bin", out.data(), Nen, 1},
        {"HITS", "Contributions per energy bin", out.data() + Nen, Nen, 1},
        {"RESPONSE", "Sum of j l E^3 exp(-tau) per (energy, time) bin, pixel [ien][it]", Nt > 0 ? out.data() + 2 * (size_t) Nen : no_response.data(), Nt > 0 ? Nt : 1, Nen},
        {"IMAGE", "Total of j l E^3 exp(-tau) along the ray of pixel [ix][iy]", image.data(), Ny, Nx}};
    for (const Plane& pl : planes) {
        fits.write_image_array(pl.data, pl.n1, pl.n2);
        fits.set_ext_name(pl.name);
        fits.write_comment(pl.what);
    }
    fits.close();

    if (timing)
        cout << "timing: source rays " << num_rays << " cells " << ncell << " | sources + map " << ms_sources << " ms (map launches " << ms_map << ") | camera rays "
             << st.rays_traced << " steps " << st.steps_total << " | emissivity + plane + observe " << ms_observe << " ms (observe launch " << st.kernel_ms << ") | files "
             << clock.lap_ms() << " ms" << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
