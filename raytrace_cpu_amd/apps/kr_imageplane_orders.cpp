// apps/kr_imageplane_orders.cpp -- the order-resolved images of an equatorial disc: the image plane of kr_imageplane_disc_image, but its rays
// run on THROUGH the plane theta = pi/2 (theta_max = 0) and every meeting with it is recorded on the device (kr_trace_crossings_dev_f64,
// include/kr_trace.h has the rule).  Crossing number k of a camera ray is the image of order k: the direct image (0), the underside of the disc
// seen over the top of the hole (1), the photon ring (>= 2).  A ray ends with its (max_order + 1)-th crossing (stop_when_full), which also
// removes the rays that whirl at the photon sphere.
//
// Reads the plane and disc keys of imageplane_app.h plus
//   max_order = 2      orders 0 .. max_order are recorded (max_order + 1 <= 16 crossings per ray)
//   steplim            the step limit of a ray (default: the trace's)
//   opaque = 1         also write the image of an opaque disc: every ray's FIRST crossing inside [r_isco, r_disc)
//   integrator = rk4   euler or rk4, strict arithmetic (the crossings carry the reference's arithmetic; RK45 is not recorded)
// Writes <outfile stem>_n<k>.fits for k = 0 .. max_order and, with opaque, <stem>_opaque.fits: each the 7-HDU file of
// kr_imageplane_disc_image (primary + FLUX, RADIUS, PHI, ENSHIFT, TIME, EMIS; apps/disc_image_fits.h) with two more cards in the primary header,
// ORDER (-1: the opaque disc) and MAXORD.  Extensions: --integrator, --device, --timing.
// Every key may also be given as --key=value, which takes precedence over the file (before imageplane_app.h only outfile, incl, spin and integrator could;
// the other arguments were ignored), and `device` may stand in the file.  --arithmetic is checked like the other programs' and then not used.
// Without a device: exits 1 with the library's message and writes nothing.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "imageplane_app.h"

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt);
    const int max_order = opt.integer("max_order", 2);
    const int steplim = opt.integer("steplim", -1);
    const bool opaque = opt.integer("opaque", 1) != 0;
    if (max_order < 0 || max_order > 15) throw invalid_argument("max_order: expected 0 .. 15");
    s.print_isco();

    const kr_imageplane plane = s.plane();
    const kr_image_bins bins = s.image_bins();
    kr_params p = s.params(KR_RK4);
    p.theta_max = 0;                         // no theta limit: the rays run on through the plane
    p.flags = 0;                             // the crossings carry the reference's arithmetic
    if (steplim > 0) p.steplim = steplim;

    kr_crossing_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.V = -1.0;                           // the Keplerian flow at the crossing, as the image app's redshift(-1, reverse = 1)
    spec.max_crossings = max_order + 1;
    spec.stop_when_full = 1;
    spec.reverse = 1;

    // ---- device pipeline ------------------------------------------------------------------------------------------
    krapp::require_device();
    krapp::DiscPlaneRun run(s, plane);
    const int64_t n = run.n, npix = (int64_t) s.ax.img_nx * s.ax.img_ny;
    krapp::DeviceBuffer rows(n * spec.max_crossings * 4 * (int64_t) sizeof(double));
    krapp::DeviceBuffer seen(n * (int64_t) sizeof(int32_t));
    run.trace(plane, p, 7 * npix + 1, false, "trace + crossings", [&](const kr_params* q, void* rays, int64_t m, kr_stats* st) {
        return kr_trace_crossings_dev_f64(q, &spec, rays, m, rows.get(), seen.get(), nullptr, st);
    });
    krapp::DeviceBuffer& planes = *run.acc;

    const string& out_name = s.out_name;
    const string stem = out_name.size() > 5 && out_name.compare(out_name.size() - 5, 5, ".fits") == 0 ? out_name.substr(0, out_name.size() - 5) : out_name;
    krapp::PinnedDoubles h(7 * npix + 1);
    double ms_images = 0, ms_fits = 0;
    vector<int> orders;
    for (int k = 0; k <= max_order; ++k) orders.push_back(k);
    if (opaque) orders.push_back(-1);
    for (int order : orders) {
        planes.zero();
        krapp::check(kr_reduce_crossing_image_dev_f64(&bins, spec.max_crossings, order, -1 * M_PI, M_PI, run.rays->get(), rows.get(), seen.get(), n, planes.get(), nullptr),
                     "image planes of one order");
        krapp::check(kr_memcpy_d2h(h.data(), planes.get(), h.size() * (int64_t) sizeof(double)), "d2h");
        // per-pixel means as kr_imageplane_disc_image takes them
        const long disc_count = static_cast<long>(h[7 * npix]);
        krapp::DiscImageMeans means = krapp::disc_image_means(h.data(), npix, s.ax.img_nx, s.ax.img_ny);
        ms_images += run.clock.lap_ms();
        const string name = order < 0 ? stem + "_opaque.fits" : stem + "_n" + to_string(order) + ".fits";
        cout << (order < 0 ? string("opaque disc") : "order " + to_string(order)) << ": " << disc_count << " rays -> " << name << endl;
        const int cards[2] = {order, max_order};
        krapp::write_disc_image_fits(name, s.image_info(disc_count), means.planes.data(), cards);
        ms_fits += run.clock.lap_ms();
    }

    if (s.timing)
        run.print_timing(" longest " + to_string(run.st.longest_ray_steps), "trace+crossings")
            << "planes+readback+means of " << orders.size() << " images " << ms_images << " ms | FITS files " << ms_fits << " ms" << endl;
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "../par/imageplane_disc_image.par", program); }
