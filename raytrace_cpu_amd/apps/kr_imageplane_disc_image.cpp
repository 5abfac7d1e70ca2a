// apps/kr_imageplane_disc_image.cpp -- the reference's `imageplane_disc_image` program
// (src/imageplane/imageplane_disc_image.cpp) with the ray pipeline resident on the MI355X: the image-plane rays are
// generated, traced to the disc, redshifted and accumulated into the seven image planes in HBM; only the planes come
// back.  Same parameter file and overrides, same 7-HDU FITS file (primary + FLUX, RADIUS, PHI, ENSHIFT, TIME, EMIS),
// written by include/fits_output.h without cfitsio.
//
// Reads (imageplane_disc_image.cpp:30-66): --parfile (default ../par/imageplane_disc_image.par), --outfile | outfile, dist,
// --incl | incl, plane_phi0 = 0, --spin | spin, r_disc, x0 = -r_disc, xmax = r_disc, Nx, y0 = x0, ymax = xmax, Ny = Nx,
// img_Nx = Nx, img_Ny = img_Nx, q1 = 3, rb1 = 4, q2 = 3, rb2 = 10, q3 = 3, precision = 100, flip_image = true,
// integrator = rk45, rk45_tol = 1e-8.  (max_tstep is read and ignored by the reference, :63, :109.)
// Extensions: --integrator, --arithmetic | KRTRACE_ARITHMETIC, --device, --timing.  These are the plane and disc keys of imageplane_app.h, which reads
// them: every key, disc_slope, disc_scale and disc_rin included, may also be given as --key=value, which takes precedence over the file (before
// imageplane_app.h only outfile, incl, spin and integrator could; the other arguments were ignored), and `device` may stand in the file.
// disc_slope, disc_scale (and disc_rin = ISCO): with either key the disc has a surface, z = +-H(rho), H = disc_slope rho + disc_scale (1 - sqrt(disc_rin / rho))
// between disc_rin and r_disc (KR_STOP_THICKDISC, include/kr_trace.h): the rays stop on it (RK4 / RK45), the gas orbits at the cylindrical radius rho, the
// emissivity is taken at rho and the RADIUS plane holds rho (kr_post_image_surface_dev_f64).  Without the keys the program and its output are what they were.
// Difference: under RK45 a pixel exactly at (0, 0) never returns in the reference; here it ends with KR_STATUS_NAN.
#include <cmath>
#include <iostream>
#include <string>
using namespace std;

#include "imageplane_app.h"

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt, true);
    const bool thick = opt.has("disc_slope") || opt.has("disc_scale");
    const double disc_slope = opt.num("disc_slope", 0), disc_scale = opt.num("disc_scale", 0);
    if (thick && s.flow.plunge) throw invalid_argument("plunge: the surface of a thick disc keeps the Keplerian flow (no disc_slope / disc_scale)");
    s.print_isco();

    const kr_imageplane plane = s.plane();
    const kr_image_bins bins = s.image_bins();
    kr_params p = s.params(KR_RK45);
    if (thick) {
        p.stop_kind = KR_STOP_THICKDISC;
        p.stop_params[0] = opt.num("disc_rin", s.r_isco); p.stop_params[1] = s.r_disc; p.stop_params[2] = disc_slope; p.stop_params[3] = disc_scale;
    }

    // ---- device pipeline ------------------------------------------------------------------------------------------
    krapp::DiscPlaneRun run(s, plane);
    const int64_t npix = (int64_t) s.ax.img_nx * s.ax.img_ny;
    run.trace(plane, p, 7 * npix + 1);
    void *rays = run.rays->get(), *planes = run.acc->get();
    if (thick)
        krapp::check(kr_post_image_surface_dev_f64(-s.spin, 1, -1 * M_PI, M_PI, &bins, rays, run.n, planes, nullptr), "redshift + range_phi + image planes of the surface");
    else
        krapp::check(kr_post_image_dev_f64(-s.spin, s.flow.V(), 1, 0, 0, -1 * M_PI, M_PI, &bins, rays, run.n, planes, nullptr), "redshift + range_phi + image planes");
    krapp::PinnedDoubles h(7 * npix + 1);     // 0.94 GB at 4096^2: page-locked, or the read-back runs at a tenth of the PCIe rate
    krapp::check(kr_memcpy_d2h(h.data(), planes, h.size() * (int64_t) sizeof(double)), "d2h");
    const double ms_post = run.clock.lap_ms();

    const long disc_count = static_cast<long>(h[7 * npix]);
    cout << disc_count << " rays hit the disc" << endl;
    krapp::DiscImageMeans means = krapp::disc_image_means(h.data(), npix, s.ax.img_nx, s.ax.img_ny);
    const double ms_means = run.clock.lap_ms();

    // ---- FITS (imageplane_disc_image.cpp:176-304) ----------------------------------------------------------------------
    krapp::write_disc_image_fits(s.out_name, s.image_info(disc_count), means.planes.data());
    const double ms_fits = run.clock.lap_ms();

    if (s.timing)
        run.print_timing() << "redshift+range_phi+planes+readback " << ms_post << " ms | per-pixel means " << ms_means << " ms | FITS file " << ms_fits << " ms" << endl;
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "../par/imageplane_disc_image.par", program); }
