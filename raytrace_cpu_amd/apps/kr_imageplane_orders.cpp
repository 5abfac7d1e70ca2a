// apps/kr_imageplane_orders.cpp -- the order-resolved images of an equatorial disc: the image plane of kr_imageplane_disc_image, but its rays
// run on THROUGH the plane theta = pi/2 (theta_max = 0) and every meeting with it is recorded on the device (kr_trace_crossings_dev_f64,
// include/kr_trace.h has the rule).  Crossing number k of a camera ray is the image of order k: the direct image (0), the underside of the disc
// seen over the top of the hole (1), the photon ring (>= 2).  A ray ends with its (max_order + 1)-th crossing (stop_when_full), which also
// removes the rays that whirl at the photon sphere.
//
// Reads the parameter file of kr_imageplane_disc_image (same keys, same overrides) plus
//   max_order = 2      orders 0 .. max_order are recorded (max_order + 1 <= 16 crossings per ray)
//   steplim            the step limit of a ray (default: the trace's)
//   opaque = 1         also write the image of an opaque disc: every ray's FIRST crossing inside [r_isco, r_disc)
//   integrator = rk4   euler or rk4, strict arithmetic (the crossings carry the reference's arithmetic; RK45 is not recorded)
// Writes <outfile stem>_n<k>.fits for k = 0 .. max_order and, with opaque, <stem>_opaque.fits: each the 7-HDU file of
// kr_imageplane_disc_image (primary + FLUX, RADIUS, PHI, ENSHIFT, TIME, EMIS; apps/disc_image_fits.h) with two more cards in the primary header,
// ORDER (-1: the opaque disc) and MAXORD.  Extensions: --integrator, --device, --timing.
// Without a device: exits 1 with the library's message and writes nothing.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "app_common.h"
#include "disc_image_fits.h"

using krapp::AxisInfo;

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process: hardware queues for overlapping launches (include/kr_trace.h)
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/imageplane_disc_image.par");
    ParameterFile par(par_name);

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    const double dist = par.get_parameter<double>("dist");
    const double incl = args.key_exists("--incl") ? args.get_parameter<double>("--incl") : par.get_parameter<double>("incl");
    const double plane_phi0 = par.get_parameter<double>("plane_phi0", 0);
    const double spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
    const double r_disc = par.get_parameter<double>("r_disc");
    AxisInfo ax;
    ax.x0 = par.get_parameter<double>("x0", -1 * r_disc);
    ax.xmax = par.get_parameter<double>("xmax", r_disc);
    const int Nx = par.get_parameter<int>("Nx");
    ax.y0 = par.get_parameter<double>("y0", ax.x0);
    ax.ymax = par.get_parameter<double>("ymax", ax.xmax);
    const int Ny = par.get_parameter<int>("Ny", Nx);
    ax.img_nx = par.get_parameter<int>("img_Nx", Nx);
    ax.img_ny = par.get_parameter<int>("img_Ny", ax.img_nx);
    const double q1 = par.get_parameter<double>("q1", 3), rb1 = par.get_parameter<double>("rb1", 4), q2 = par.get_parameter<double>("q2", 3),
                 rb2 = par.get_parameter<double>("rb2", 10), q3 = par.get_parameter<double>("q3", 3);
    const double precision = par.get_parameter<double>("precision", 100);
    const bool flip_image = par.get_parameter<bool>("flip_image", true);
    const string integ = args.key_exists("--integrator") ? args.get_parameter<string>("--integrator") : par.get_parameter<string>("integrator", "rk4");
    const int max_order = par.get_parameter<int>("max_order", 2);
    const int steplim = par.get_parameter<int>("steplim", -1);
    const bool opaque = par.get_parameter<int>("opaque", 1) != 0;
    const bool timing = args.key_exists("--timing");
    if (max_order < 0 || max_order > 15) throw invalid_argument("max_order: expected 0 .. 15");

    ax.dx = (ax.xmax - ax.x0) / Nx;
    ax.dy = (ax.ymax - ax.y0) / Ny;
    const double r_isco = kerr_isco<double>(spin, +1);
    cout << "ISCO at " << r_isco << endl;

    kr_imageplane plane;
    memset(&plane, 0, sizeof plane);
    plane.dist = dist;
    plane.inc_deg = incl;
    plane.x0 = ax.x0; plane.xmax = ax.xmax; plane.dx = ax.dx;
    plane.y0 = ax.y0; plane.ymax = ax.ymax; plane.dy = ax.dy;
    plane.spin = spin;
    plane.phi0 = plane_phi0;
    plane.precision = precision;

    kr_image_bins bins;
    memset(&bins, 0, sizeof bins);
    bins.x0 = ax.x0; bins.y0 = ax.y0;
    bins.img_dx = (ax.xmax - ax.x0) / ax.img_nx;
    bins.img_dy = (ax.ymax - ax.y0) / ax.img_ny;
    bins.r_isco = r_isco; bins.r_disc = r_disc;
    bins.q1 = q1; bins.rb1 = rb1; bins.q2 = q2; bins.rb2 = rb2; bins.q3 = q3;
    bins.img_nx = ax.img_nx; bins.img_ny = ax.img_ny;
    bins.flip_image = flip_image ? 1 : 0;

    kr_params p;
    kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane.cpp:12)
    p.precision = precision;
    p.integrator = krapp::integrator_code(integ, KR_RK4);
    p.theta_max = 0;                         // no theta limit: the rays run on through the plane
    p.r_max = 1.1 * dist;
    p.stop_kind = KR_STOP_THETA;
    p.flags = 0;
    if (steplim > 0) p.steplim = steplim;

    kr_crossing_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.V = -1.0;                           // the Keplerian flow at the crossing, as the image app's redshift(-1, reverse = 1)
    spec.max_crossings = max_order + 1;
    spec.stop_when_full = 1;
    spec.reverse = 1;

    // ---- device pipeline ------------------------------------------------------------------------------------------
    krapp::require_device();
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t n = kr_imageplane_count(&plane, nullptr, nullptr);
    if (n <= 0) throw runtime_error("empty ray grid");
    const int64_t npix = (int64_t) ax.img_nx * ax.img_ny;
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::DeviceBuffer rows(n * spec.max_crossings * 4 * (int64_t) sizeof(double));
    krapp::DeviceBuffer seen(n * (int64_t) sizeof(int32_t));
    krapp::DeviceBuffer planes((7 * npix + 1) * (int64_t) sizeof(double));
    krapp::check(kr_imageplane_init_emit_dev_f64(&plane, 0, 1, 0.0, 1, 0, rays.get(), n, nullptr), "imageplane_init + redshift_start");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_init = clock.lap_ms();
    kr_stats st;
    krapp::check(kr_trace_crossings_dev_f64(&p, &spec, rays.get(), n, rows.get(), seen.get(), nullptr, &st), "trace + crossings");
    const double ms_trace = clock.lap_ms();

    const string stem = out_name.size() > 5 && out_name.compare(out_name.size() - 5, 5, ".fits") == 0 ? out_name.substr(0, out_name.size() - 5) : out_name;
    krapp::PinnedDoubles h(7 * npix + 1);
    double ms_images = 0, ms_fits = 0;
    vector<int> orders;
    for (int k = 0; k <= max_order; ++k) orders.push_back(k);
    if (opaque) orders.push_back(-1);
    for (int order : orders) {
        planes.zero();
        krapp::check(kr_reduce_crossing_image_dev_f64(&bins, spec.max_crossings, order, -1 * M_PI, M_PI, rays.get(), rows.get(), seen.get(), n, planes.get(), nullptr),
                     "image planes of one order");
        krapp::check(kr_memcpy_d2h(h.data(), planes.get(), h.size() * (int64_t) sizeof(double)), "d2h");
        // per-pixel means as kr_imageplane_disc_image takes them: flux only where rays arrived, the rest 0/0 -> NaN
        const long disc_count = static_cast<long>(h[7 * npix]);
        double* hp = h.data();
        krapp::parallel_for(npix, [=](int64_t a, int64_t b) {
            for (int64_t i = a; i < b; ++i) {
                const int hits = static_cast<int>(hp[i]);
                if (hits > 0) hp[npix + i] /= hits;
                for (int k = 2; k <= 6; ++k) hp[k * npix + i] /= hits;
            }
        });
        vector<vector<double*>> prows(6, vector<double*>(static_cast<size_t>(ax.img_nx)));
        double** sums[6];
        for (int k = 0; k < 6; ++k) {
            for (int ix = 0; ix < ax.img_nx; ++ix) prows[k][ix] = hp + (k + 1) * npix + static_cast<int64_t>(ix) * ax.img_ny;
            sums[k] = prows[k].data();
        }
        ms_images += clock.lap_ms();
        const string name = order < 0 ? stem + "_opaque.fits" : stem + "_n" + to_string(order) + ".fits";
        cout << (order < 0 ? string("opaque disc") : "order " + to_string(order)) << ": " << disc_count << " rays -> " << name << endl;
        krapp::DiscImageInfo info = {dist, incl, spin, r_isco, r_disc, q1, rb1, q2, rb2, q3, Nx * Ny, disc_count, ax};
        const int cards[2] = {order, max_order};
        krapp::write_disc_image_fits(name, info, sums, cards);
        ms_fits += clock.lap_ms();
    }

    if (timing)
        cout << "timing: rays " << st.rays_traced << " steps " << st.steps_total << " longest " << st.longest_ray_steps << " | init+redshift_start " << ms_init
             << " ms | trace+crossings " << ms_trace << " ms (kernel " << st.kernel_ms << ") | planes+readback+means of " << orders.size() << " images " << ms_images
             << " ms | FITS files " << ms_fits << " ms" << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
