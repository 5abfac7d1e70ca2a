// apps/caustic_app.h -- what kr_caustic_discplane, kr_caustic_sourceplane and kr_caustic_plane share: the image-plane parameters the three programs
// read, the resident pipeline (ray grid or 5-ray bundles -> trace -> the program's map passes -> the maps read back) and the FITS pieces common to
// their files.  Where the programs differ on purpose, the difference is an argument.
#ifndef KR_APP_CAUSTIC_APP_H_
#define KR_APP_CAUSTIC_APP_H_

#include <cmath>
#include <functional>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../host/include/fits_output.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "app_common.h"
#include "imageplane_app.h"

namespace krapp {

// caustic_discplane.cpp:73-110 / caustic_sourceplane.cpp:84-137 / caustic_plane.cpp:74-135: the parameters the programs have in common
struct CausticSetup {
    std::string out_name, arith;
    double dist, incl, plane_phi0, spin, x0, xmax, y0, ymax, dx, dy, rk45_tol, precision;
    int Nx, Ny, img_nx, img_ny, steplim, integrator, device;
    bool timing;

    // half_width(): the default of -x0 and xmax, asked for where the reference reads it (after spin).  steplim_default: without --steplim | steplim.
    // other_integrator(name): called for a name that is neither rk4 nor rk45 (RK45 is used), to warn as the program's original does.
    // Arithmetic, when neither --arithmetic nor KRTRACE_ARITHMETIC names one: strict for every integrator (det J amplifies end-point differences by 1e2-1e3).
    CausticSetup(ParameterArgs& args, ParameterFile& par, const std::function<double()>& half_width, int steplim_default,
                 const std::function<void(const std::string&)>& other_integrator)
    {
        out_name = args.key_exists("--outfile") ? args.get_parameter<std::string>("--outfile") : par.get_parameter<std::string>("outfile");
        dist = par.get_parameter<double>("dist");
        incl = args.key_exists("--incl") ? args.get_parameter<double>("--incl") : par.get_parameter<double>("incl");
        plane_phi0 = par.get_parameter<double>("plane_phi0", 0);
        spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
        const double half = half_width();
        x0 = par.get_parameter<double>("x0", -1 * half);
        xmax = par.get_parameter<double>("xmax", half);
        Nx = par.get_parameter<int>("Nx");
        y0 = par.get_parameter<double>("y0", x0);
        ymax = par.get_parameter<double>("ymax", xmax);
        Ny = par.get_parameter<int>("Ny", Nx);
        const std::string integ = par.get_parameter<std::string>("integrator", "rk45");
        rk45_tol = par.get_parameter<double>("rk45_tol", 1e-8);
        steplim = args.key_exists("--steplim") ? args.get_parameter<int>("--steplim") : par.get_parameter<int>("steplim", steplim_default);
        precision = par.get_parameter<double>("precision", 100);
        (void) (args.key_exists("--show_progress") ? args.get_parameter<int>("--show_progress") : par.get_parameter<int>("show_progress", 1));
        arith = args.key_exists("--arithmetic") ? args.get_parameter<std::string>("--arithmetic") : arithmetic_from_env();
        if (arith.empty()) arith = "strict";
        device = args.get_parameter<int>("--device", 0);
        timing = args.key_exists("--timing");
        integrator = KR_RK45;
        if (integ == "rk4") integrator = KR_RK4;
        else if (integ != "rk45") other_integrator(integ);
        dx = (xmax - x0) / Nx;
        dy = (ymax - y0) / Ny;
        img_nx = Nx + 1;            // fencepost: the ray grid has one more point per axis than steps
        img_ny = Ny + 1;
    }

    kr_imageplane plane() const { return imageplane(dist, incl, x0, xmax, dx, y0, ymax, dy, spin, plane_phi0, precision); }

    // everything of kr_params that does not depend on the stop surface
    kr_params params() const
    {
        kr_params p;
        kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane.cpp:12, imageplane_bundles.h:151)
        p.precision = precision;
        p.integrator = integrator;
        if (integrator == KR_RK45) p.rk45_tol = rk45_tol;
        p.steplim = steplim;                     // <= 0: the reference's limit (1e7 steps, 1e5 under RK45)
        p.flags = arithmetic_flags(arith, integrator);
        return p;
    }

    // the rays of the grid (bundle_eps_frac = 0) or of its 5-ray bundles, and the pixel counts
    int64_t rays(double bundle_eps_frac, int32_t& nx, int32_t& ny) const
    {
        const kr_imageplane s = plane();
        const int64_t n = bundle_eps_frac > 0.0 ? kr_bundles_count(&s, &nx, &ny) : kr_imageplane_count(&s, &nx, &ny);
        if (n <= 0) throw std::runtime_error("empty ray grid");
        // the reference indexes its (Nx + 1) x (Ny + 1) maps with the ray source's own counts; where the two disagree it writes out of bounds
        if (nx != img_nx || ny != img_ny)
            throw std::runtime_error("the ray source's grid (" + std::to_string(nx) + " x " + std::to_string(ny) + ") is not (Nx + 1) x (Ny + 1)");
        return n;
    }
};

// one device call of a program on the n records and the map words, with the name it fails under
struct CausticStep {
    const char* what;
    std::function<int(void* rays, int64_t n, void* maps)> call;
};
struct CausticTimes {
    double init = 0, trace = 0, readback = 0;
    std::vector<double> steps;                   // one lap per map step
    kr_stats stats;
};

// The resident pipeline: grid_init (bundle_eps_frac = 0) or the bundles, the trace, the program's map steps, and the `words` map words read back.
inline std::unique_ptr<PinnedDoubles> run_caustic(const CausticSetup& s, const kr_params& p, double bundle_eps_frac, int64_t n, int64_t words, const CausticStep& grid_init,
                                                  const CausticStep& bundles_init, const std::vector<CausticStep>& steps, CausticTimes& t)
{
    check(kr_set_device(s.device), "kr_set_device");
    Stopwatch clock;
    DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    DeviceBuffer maps(words * (int64_t) sizeof(double));
    const CausticStep& init = bundle_eps_frac > 0.0 ? bundles_init : grid_init;
    check(init.call(rays.get(), n, nullptr), init.what);
    check(kr_synchronize(nullptr), "sync");
    t.init = clock.lap_ms();
    std::cout << (p.integrator == KR_RK4 ? "Running raytracer (RK4)..." : "Running raytracer (RK45/DOPRI5)...") << std::endl;
    check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &t.stats), "trace");
    t.trace = clock.lap_ms();
    for (const CausticStep& step : steps) {
        check(step.call(rays.get(), n, maps.get()), step.what);
        check(kr_synchronize(nullptr), "sync");
        t.steps.push_back(clock.lap_ms());
    }
    std::unique_ptr<PinnedDoubles> h(new PinnedDoubles(words));
    check(kr_memcpy_d2h(h->data(), maps.get(), words * (int64_t) sizeof(double)), "d2h");
    t.readback = clock.lap_ms();
    return h;
}

// the per-extension axis keywords (caustic_discplane.cpp:520-530, caustic_sourceplane.cpp:324-334, caustic_plane.cpp:414-424)
inline void write_axis_keywords(FITSOutput<double>& fits, const CausticSetup& s)
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
inline std::vector<std::vector<double*>> plane_rows(double* words, int planes, int nx, int ny)
{
    std::vector<std::vector<double*>> rows(static_cast<size_t>(planes), std::vector<double*>(static_cast<size_t>(nx)));
    for (int k = 0; k < planes; ++k)
        for (int ix = 0; ix < nx; ++ix) rows[k][ix] = words + (static_cast<int64_t>(k) * nx + ix) * ny;
    return rows;
}

// the timing line of the two source programs
inline void print_source_timing(const CausticTimes& t, double ms_fits)
{
    std::cout << "timing: rays " << t.stats.rays_traced << " steps " << t.stats.steps_total << " | init " << t.init << " ms | trace " << t.trace << " ms (kernel "
              << t.stats.kernel_ms << ") | maps " << t.steps[0] << " ms | readback " << t.readback << " ms | FITS file " << ms_fits << " ms" << std::endl;
}

}   // namespace krapp

#endif /* KR_APP_CAUSTIC_APP_H_ */
