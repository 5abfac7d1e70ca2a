// apps/imageplane_app.h -- what the programs that look at the disc from an image plane share (kr_imageplane_disc_image, kr_imageplane_orders,
// kr_line_profile, kr_imageplane_polarisation, kr_disc_spectrum, kr_hotspot_lightcurve): the plane and disc keys they read, the structs filled from
// them, the front of the resident pipeline (device, ray grid, buffers, rays with their emit, trace) and the front of the timing line.  The post pass,
// the read-back and the output stay in each program.  Where the programs differ on purpose, the difference is an argument.
//
// The plane and disc keys, in the order they are read (imageplane_disc_image.cpp:30-66), each as --key=value first, then from the parameter file:
// outfile, dist, incl, plane_phi0 = 0, spin, r_disc, x0 = -r_disc, xmax = r_disc, Nx, y0 = x0, ymax = xmax, Ny = Nx, img_Nx = Nx, img_Ny = img_Nx,
// q1 = 3, rb1 = 4, q2 = 3, rb2 = 10, q3 = 3, precision = 100, flip_image = true, integrator (the program's default), rk45_tol = 1e-8, device = 0,
// plunge = 0, r_in (app_common.h, DiscFlowKeys);
// --arithmetic | KRTRACE_ARITHMETIC and --timing come from the command line only.  Nx, Ny, img_Nx, img_Ny and device are read as int.
#ifndef KR_APP_IMAGEPLANE_APP_H_
#define KR_APP_IMAGEPLANE_APP_H_

#include <cmath>
#include <functional>
#include <iostream>
#include <memory>
#include <string>

#include "../host/include/kerr.h"
#include "app_common.h"
#include "disc_image_fits.h"

namespace krapp {

// ImagePlane<T>(dist, incl, x0, xmax, dx, y0, ymax, dy, spin, phi0, precision) as the struct of the C ABI: the one place that fills it
inline kr_imageplane imageplane(double dist, double incl, double x0, double xmax, double dx, double y0, double ymax, double dy, double spin, double phi0,
                                double precision)
{
    kr_imageplane plane;
    memset(&plane, 0, sizeof plane);
    plane.dist = dist;
    plane.inc_deg = incl;
    plane.x0 = x0; plane.xmax = xmax; plane.dx = dx;
    plane.y0 = y0; plane.ymax = ymax; plane.dy = dy;
    plane.spin = spin;
    plane.phi0 = phi0;
    plane.precision = precision;
    return plane;
}

// the degree law of kr_pol_law from the keys pol_law = 1 and pol_coeff = 0.1171 (kr_imageplane_polarisation, kr_hotspot_lightcurve)
inline kr_pol_law pol_law_of(const Options& opt)
{
    kr_pol_law pol;
    memset(&pol, 0, sizeof pol);
    pol.law = (int32_t) opt.num("pol_law", 1);
    pol.coeff = opt.num("pol_coeff", 0.1171);
    return pol;
}

// The surface keys of the programs that bin a disc of finite thickness seen from an image plane (kr_line_profile, kr_disc_spectrum, kr_reverb_response),
// read as kr_imageplane_disc_image reads them: disc_slope and disc_scale, either of which gives the disc the surface z = +-H(rho),
// H = disc_slope rho + disc_scale (1 - sqrt(disc_rin / rho)), between disc_rin (default: the ISCO) and r_disc (KR_STOP_THICKDISC and kr_disc_surface,
// include/kr_trace.h).  The rays stop on the surface, the gas orbits at the cylindrical radius rho and the pass is the program's kr_post_*_surface_dev_f64.
// Without the keys: nothing, the program and its output files what they were.  With them a text file gains the rows "# DISCSLOP", "# DISCSCAL" and
// "# DISCRIN", a FITS header the keywords of those names.
struct DiscSurfaceKeys {
    bool thick = false;
    kr_disc_surface surface = {0, 0, 0, 0};

    DiscSurfaceKeys(const Options& opt, double r_isco, double r_disc)
    {
        thick = opt.has("disc_slope") || opt.has("disc_scale");
        surface.slope = opt.num("disc_slope", 0);
        surface.scale = opt.num("disc_scale", 0);
        surface.r_in = opt.num("disc_rin", r_isco);
        surface.r_out = r_disc;
    }
    // the refusals: the surface keeps the Keplerian flow and carries no polarisation
    void refuse_with(bool plunge, bool stokes) const
    {
        if (thick && plunge) throw std::invalid_argument("plunge: the surface of a thick disc keeps the Keplerian flow (no disc_slope / disc_scale)");
        if (thick && stokes) throw std::invalid_argument("pol_law / pol_coeff: the Stokes passes know no disc surface (no disc_slope / disc_scale)");
    }
    // the trace stops on the surface
    void stop_on(kr_params& p) const
    {
        if (!thick) return;
        p.stop_kind = KR_STOP_THICKDISC;
        p.stop_params[0] = surface.r_in; p.stop_params[1] = surface.r_out; p.stop_params[2] = surface.slope; p.stop_params[3] = surface.scale;
    }
    template <class Text>
    void write_rows(Text& out) const
    {
        if (!thick) return;
        out << "# DISCSLOP" << surface.slope << std::endl;
        out << "# DISCSCAL" << surface.scale << std::endl;
        out << "# DISCRIN" << surface.r_in << std::endl;
    }
    template <class Fits>
    void write_keywords(Fits& fits) const
    {
        if (!thick) return;
        fits.write_keyword("DISCSLOP", "Disc surface: slope of H(rho)", surface.slope);
        fits.write_keyword("DISCSCAL", "Disc surface: scale of H(rho)", surface.scale);
        fits.write_keyword("DISCRIN", "Disc surface: inner radius", surface.r_in);
    }
};

struct DiscPlaneSetup {
    std::string out_name, integ, arith;
    double dist, incl, plane_phi0, spin, r_disc, r_isco, q1, rb1, q2, rb2, q3, precision, rk45_tol;
    AxisInfo ax;
    int Nx, Ny, device;
    bool flip_image, timing;
    DiscFlowKeys flow;                       // plunge, r_in: kr_imageplane_disc_image, kr_line_profile, kr_disc_spectrum, kr_reverb_response; the rest refuse plunge = 1

    explicit DiscPlaneSetup(const Options& opt, bool takes_plunge = false)
    {
        out_name = opt.str("outfile");
        dist = opt.req("dist");
        incl = opt.req("incl");
        plane_phi0 = opt.num("plane_phi0", 0);
        spin = opt.req("spin");
        r_disc = opt.req("r_disc");
        ax.x0 = opt.num("x0", -1 * r_disc);
        ax.xmax = opt.num("xmax", r_disc);
        Nx = opt.integer("Nx");
        ax.y0 = opt.num("y0", ax.x0);
        ax.ymax = opt.num("ymax", ax.xmax);
        Ny = opt.integer("Ny", Nx);
        ax.img_nx = opt.integer("img_Nx", Nx);
        ax.img_ny = opt.integer("img_Ny", ax.img_nx);
        q1 = opt.num("q1", 3); rb1 = opt.num("rb1", 4); q2 = opt.num("q2", 3); rb2 = opt.num("rb2", 10); q3 = opt.num("q3", 3);
        precision = opt.num("precision", 100);
        flip_image = opt.flag("flip_image", true);
        integ = opt.str("integrator", "");         // "" and every unknown name: the program's default, params()
        rk45_tol = opt.num("rk45_tol", 1e-8);
        arith = arithmetic_choice(opt);
        timing = opt.on_command_line("timing");
        device = opt.integer("device", 0);
        ax.dx = (ax.xmax - ax.x0) / Nx;
        ax.dy = (ax.ymax - ax.y0) / Ny;
        r_isco = kerr_isco<double>(spin, +1);
        flow = disc_flow_keys(opt, spin);
        if (flow.plunge && !takes_plunge) throw std::invalid_argument("plunge: this program does not take the plunging disc flow");
    }

    // a program says this once its own keys are read and checked
    void print_isco() const { std::cout << "ISCO at " << r_isco << std::endl; }

    kr_imageplane plane() const { return imageplane(dist, incl, ax.x0, ax.xmax, ax.dx, ax.y0, ax.ymax, ax.dy, spin, plane_phi0, precision); }

    // the trace to the equatorial plane within 1.1 dist
    kr_params params(int default_integrator) const
    {
        kr_params p;
        kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane.cpp:12)
        p.precision = precision;
        p.integrator = integrator_code(integ, default_integrator);
        if (p.integrator == KR_RK45) p.rk45_tol = rk45_tol;
        p.theta_max = M_PI_2;
        p.r_max = 1.1 * dist;
        p.stop_kind = KR_STOP_THETA;
        p.flags = arithmetic_flags(arith, p.integrator);
        return p;
    }

    // r_isco, r_disc and the powerlaw3 emissivity into any struct that carries them (kr_image_bins, kr_line_bins, kr_spectrum_model)
    template <class Bins>
    void fill_disc(Bins& b) const
    {
        b.r_isco = flow.inner_edge(r_isco); b.r_disc = r_disc;
        b.q1 = q1; b.rb1 = rb1; b.q2 = q2; b.rb2 = rb2; b.q3 = q3;
    }

    kr_image_bins image_bins() const
    {
        kr_image_bins bins;
        memset(&bins, 0, sizeof bins);
        bins.x0 = ax.x0; bins.y0 = ax.y0;
        bins.img_dx = (ax.xmax - ax.x0) / ax.img_nx;
        bins.img_dy = (ax.ymax - ax.y0) / ax.img_ny;
        fill_disc(bins);
        bins.img_nx = ax.img_nx; bins.img_ny = ax.img_ny;
        bins.flip_image = flip_image ? 1 : 0;
        return bins;
    }

    // the primary header of the disc-image file
    DiscImageInfo image_info(long disc_count) const { return {dist, incl, spin, r_isco, r_disc, q1, rb1, q2, rb2, q3, Nx * Ny, disc_count, ax, flow.plunge, flow.r_in}; }
};

// The front of the resident pipeline.  The constructor: kr_set_device, the ray count, the ray buffer.  trace(): the accumulator of `words` doubles
// (zeroed here, unless the program zeroes it before each of several images), the rays with their emit (init lap), the program's trace step (trace lap).
struct DiscPlaneRun {
    using Step = std::function<int(const kr_params* p, void* rays, int64_t n, kr_stats* st)>;

    Stopwatch clock;
    int64_t n;
    std::unique_ptr<DeviceBuffer> rays, acc;
    double ms_init = 0, ms_trace = 0;
    kr_stats st;

    DiscPlaneRun(const DiscPlaneSetup& s, const kr_imageplane& plane)
    {
        check(kr_set_device(s.device), "kr_set_device");
        clock = Stopwatch();
        n = kr_imageplane_count(&plane, nullptr, nullptr);
        if (n <= 0) throw std::runtime_error("empty ray grid");
        rays.reset(new DeviceBuffer(n * (int64_t) sizeof(kr_ray_f64)));
    }

    void trace(const kr_imageplane& plane, const kr_params& p, int64_t words, bool zeroed, const char* what, const Step& step)
    {
        acc.reset(new DeviceBuffer(words * (int64_t) sizeof(double)));
        if (zeroed) acc->zero();
        check(kr_imageplane_init_emit_dev_f64(&plane, 0, 1, 0.0, 1, 0, rays->get(), n, nullptr), "imageplane_init + redshift_start");
        check(kr_synchronize(nullptr), "sync");
        ms_init = clock.lap_ms();
        check(step(&p, rays->get(), n, &st), what);
        ms_trace = clock.lap_ms();
    }
    // the step of every program but kr_imageplane_orders
    void trace(const kr_imageplane& plane, const kr_params& p, int64_t words)
    {
        trace(plane, p, words, true, "trace", [](const kr_params* q, void* r, int64_t m, kr_stats* s) { return kr_trace_dev_f64(q, r, m, nullptr, s); });
    }

    // "timing: rays ... steps ...<after_steps> | init+redshift_start ... ms | <trace_name> ... ms (kernel ...) | ": the program appends its own laps
    std::ostream& print_timing(const std::string& after_steps = "", const char* trace_name = "trace") const
    {
        return std::cout << "timing: rays " << st.rays_traced << " steps " << st.steps_total << after_steps << " | init+redshift_start " << ms_init << " ms | " << trace_name
                         << " " << ms_trace << " ms (kernel " << st.kernel_ms << ") | ";
    }
};

}   // namespace krapp

#endif /* KR_APP_IMAGEPLANE_APP_H_ */
