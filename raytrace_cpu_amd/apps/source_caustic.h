// apps/source_caustic.h -- what kr_caustic_sourceplane and kr_caustic_plane share: the image-plane parameters both programs read, the resident
// pipeline (ray grid or 5-ray bundles -> trace -> kr_post_caustic_source_dev_f64 -> the maps read back) and the FITS pieces common to their files.
#ifndef KR_APP_SOURCE_CAUSTIC_H_
#define KR_APP_SOURCE_CAUSTIC_H_

#include <cmath>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../host/include/fits_output.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "app_common.h"

namespace krapp {

// caustic_sourceplane.cpp:84-137 / caustic_plane.cpp:74-135: the parameters the two programs have in common
struct SourceCausticSetup {
    std::string out_name, arith;
    double dist, incl, plane_phi0, spin, x0, xmax, y0, ymax, dx, dy, rk45_tol, precision;
    int Nx, Ny, img_nx, img_ny, steplim, integrator, device;
    bool timing;

    SourceCausticSetup(ParameterArgs& args, ParameterFile& par)
    {
        out_name = args.key_exists("--outfile") ? args.get_parameter<std::string>("--outfile") : par.get_parameter<std::string>("outfile");
        dist = par.get_parameter<double>("dist");
        incl = args.key_exists("--incl") ? args.get_parameter<double>("--incl") : par.get_parameter<double>("incl");
        plane_phi0 = par.get_parameter<double>("plane_phi0", 0);
        spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
        x0 = par.get_parameter<double>("x0", -20.0);
        xmax = par.get_parameter<double>("xmax", 20.0);
        Nx = par.get_parameter<int>("Nx");
        y0 = par.get_parameter<double>("y0", x0);
        ymax = par.get_parameter<double>("ymax", xmax);
        Ny = par.get_parameter<int>("Ny", Nx);
        const std::string integ = par.get_parameter<std::string>("integrator", "rk45");
        rk45_tol = par.get_parameter<double>("rk45_tol", 1e-8);
        steplim = args.key_exists("--steplim") ? args.get_parameter<int>("--steplim") : par.get_parameter<int>("steplim", -1);
        precision = par.get_parameter<double>("precision", 100);
        (void) (args.key_exists("--show_progress") ? args.get_parameter<int>("--show_progress") : par.get_parameter<int>("show_progress", 1));
        arith = args.key_exists("--arithmetic") ? args.get_parameter<std::string>("--arithmetic") : arithmetic_from_env();
        if (arith.empty()) arith = "strict";         // det J amplifies end-point differences by 1e2-1e3
        device = args.get_parameter<int>("--device", 0);
        timing = args.key_exists("--timing");
        integrator = KR_RK45;
        if (integ == "rk4") integrator = KR_RK4;
        else if (integ != "rk45") std::cerr << "Warning: unknown integrator '" << integ << "'; using RK45" << std::endl;
        dx = (xmax - x0) / Nx;
        dy = (ymax - y0) / Ny;
        img_nx = Nx + 1;            // fencepost: the ray grid has one more point per axis than steps
        img_ny = Ny + 1;
    }

    kr_imageplane plane() const
    {
        kr_imageplane s;
        memset(&s, 0, sizeof s);
        s.dist = dist; s.inc_deg = incl;
        s.x0 = x0; s.xmax = xmax; s.dx = dx;
        s.y0 = y0; s.ymax = ymax; s.dy = dy;
        s.spin = spin; s.phi0 = plane_phi0; s.precision = precision;
        return s;
    }

    // everything of kr_params that does not depend on the stop surface
    kr_params params() const
    {
        kr_params p;
        kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane.cpp:12)
        p.precision = precision;
        p.integrator = integrator;
        if (integrator == KR_RK45) p.rk45_tol = rk45_tol;
        p.steplim = steplim;                     // <= 0: the reference's limit (1e7 steps, 1e5 under RK45)
        p.flags = arithmetic_flags(arith, integrator);
        return p;
    }
};

struct SourceCausticTimes {
    double init = 0, trace = 0, maps = 0, readback = 0;
    kr_stats stats;
};

// The resident pipeline.  sm comes in with kind, the eps and the trig terms set; nx, ny and bundles are filled in here.  Returns the 8 nx ny + 3 words.
inline std::unique_ptr<PinnedDoubles> run_source_caustic(const SourceCausticSetup& s, const kr_params& p, kr_source_map& sm, double bundle_eps_frac, SourceCausticTimes& t)
{
    const kr_imageplane plane = s.plane();
    const bool bundles = sm.kind == 1 && bundle_eps_frac > 0.0;
    int32_t nx = 0, ny = 0;
    const int64_t n = bundles ? kr_bundles_count(&plane, &nx, &ny) : kr_imageplane_count(&plane, &nx, &ny);
    if (n <= 0) throw std::runtime_error("empty ray grid");
    // the reference indexes its (Nx + 1) x (Ny + 1) maps with the ray source's own counts; where the two disagree it writes out of bounds
    if (nx != s.img_nx || ny != s.img_ny)
        throw std::runtime_error("the ray source's grid (" + std::to_string(nx) + " x " + std::to_string(ny) + ") is not (Nx + 1) x (Ny + 1)");
    sm.nx = nx; sm.ny = ny;
    sm.bundles = bundles ? 1 : 0;

    require_device();
    check(kr_set_device(s.device), "kr_set_device");
    Stopwatch clock;
    const int64_t words = 8 * (int64_t) nx * ny + 3;
    DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    DeviceBuffer maps(words * (int64_t) sizeof(double));
    if (bundles) check(kr_bundles_init_emit_dev_f64(&plane, bundle_eps_frac, 0.0, 1, 0, rays.get(), n, nullptr), "bundles_init");
    else check(kr_imageplane_init_dev_f64(&plane, rays.get(), n, nullptr), "imageplane_init");
    check(kr_synchronize(nullptr), "sync");
    t.init = clock.lap_ms();
    std::cout << (p.integrator == KR_RK4 ? "Running raytracer (RK4)..." : "Running raytracer (RK45/DOPRI5)...") << std::endl;
    check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &t.stats), "trace");
    t.trace = clock.lap_ms();
    check(kr_post_caustic_source_dev_f64(&sm, rays.get(), n, maps.get(), nullptr), "maps");
    check(kr_synchronize(nullptr), "sync");
    t.maps = clock.lap_ms();
    std::unique_ptr<PinnedDoubles> h(new PinnedDoubles(words));
    check(kr_memcpy_d2h(h->data(), maps.get(), words * (int64_t) sizeof(double)), "d2h");
    t.readback = clock.lap_ms();
    return h;
}

// the per-extension axis keywords (caustic_sourceplane.cpp:324-334, caustic_plane.cpp:414-424)
inline void write_axis_keywords(FITSOutput<double>& fits, const SourceCausticSetup& s)
{
    fits.write_keyword("X0", "Start of X axis (rg)", s.x0);
    fits.write_keyword("XMAX", "End of X axis (rg)", s.xmax);
    fits.write_keyword("DX", "X step (rg)", s.dx);
    fits.write_keyword("NX", "Number of pixels in X", s.img_nx);
    fits.write_keyword("Y0", "Start of Y axis (rg)", s.y0);
    fits.write_keyword("YMAX", "End of Y axis (rg)", s.ymax);
    fits.write_keyword("DY", "Y step (rg)", s.dy);
    fits.write_keyword("NY", "Number of pixels in Y", s.img_ny);
}

// rows[k][ix]: plane k of the words as the double** that FITSOutput::write_image takes
inline std::vector<std::vector<double*>> plane_rows(double* words, int nx, int ny)
{
    std::vector<std::vector<double*>> rows(8, std::vector<double*>(static_cast<size_t>(nx)));
    for (int k = 0; k < 8; ++k)
        for (int ix = 0; ix < nx; ++ix) rows[k][ix] = words + (static_cast<int64_t>(k) * nx + ix) * ny;
    return rows;
}

inline void print_timing(const SourceCausticTimes& t, double ms_fits)
{
    std::cout << "timing: rays " << t.stats.rays_traced << " steps " << t.stats.steps_total << " | init " << t.init << " ms | trace " << t.trace << " ms (kernel "
              << t.stats.kernel_ms << ") | maps " << t.maps << " ms | readback " << t.readback << " ms | FITS file " << ms_fits << " ms" << std::endl;
}

}   // namespace krapp

#endif /* KR_APP_SOURCE_CAUSTIC_H_ */
