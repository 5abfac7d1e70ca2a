// GPU test program for the host-side C++ mirror (raytrace_cpu_amd/host): exercises parts of the reference class API
// that the reference's own apps do not reach.  Built by tests/cpp/Makefile, run by tests/test_gpu_host_mirror.py.
// Exit code 0 = every check passed; each failed check prints a line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "kr_trace.h"
#include "raytracer/imageplane.h"
#include "raytracer/pointsource.h"
#include "raytracer/ray_destination.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a user-defined destination: the HIP path must refuse it in run_raytrace, but redshift(dest) must still work (host loop)
template <typename T>
class SlowDisc : public RayDestination<T> {
public:
    bool reached(T r, T theta, T phi) const override { return theta >= T(M_PI_2); }
    T velocity(T r, T theta, T phi) const override { return T(0.5) / (T(0.998) + r * std::sqrt(r)); }   // half Keplerian
};

int main(int argc, char** argv)
{
    const double spin = 0.998;
    double pos[4] = {0.0, 10.0, 1e-3, 1.5707};

    // `host_api_test steplim-env` with KRTRACE_STEPLIM=40 in the environment: the limit applies where the application passes none
    // (Euler / RK4 default STEPLIM = 1e7), marks the unfinished rays RAY_STATUS_STEPLIM with a negated count, and leaves an explicit steplim alone
    if (argc > 1 && std::string(argv[1]) == "steplim-env") {
        PointSource<double> a(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        PointSource<double> b(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        a.run_raytrace(Integrator::RK4, M_PI_2, 1000.0, 0);                                   // no steplim passed -> the environment's 40
        b.run_raytrace(Integrator::RK4, M_PI_2, 1000.0, 0, 0, 1, -1, -1, true, 100000);       // explicit -> untouched
        int capped = 0, live = 0;
        for (int i = 0; i < a.get_count(); i++) {
            if (b.rays[i].steps == -1) continue;
            ++live;
            if (b.rays[i].steps > 40) {
                ++capped;
                CHECK(a.rays[i].steps == -40 && (a.rays[i].status & RAY_STATUS_STEPLIM), "ray %d: steps %d status %d under KRTRACE_STEPLIM=40", i, a.rays[i].steps, a.rays[i].status);
            } else {
                CHECK(a.rays[i].steps == b.rays[i].steps, "ray %d finished early but differs: %d vs %d", i, a.rays[i].steps, b.rays[i].steps);
            }
        }
        CHECK(live > 100 && capped > 50, "too few rays: live %d capped %d", live, capped);
        std::printf(failures ? "FAIL\n" : "PASS\n");
        return failures ? 1 : 0;
    }

    if (argc > 1 && !std::strcmp(argv[1], "progress")) {
        // run_raytrace(show_progress = -250000) on 2e6 rays: plain report lines "Ray <done>/<total>" (negative: no bar), the integrator's banner first
        const double d = 1.99 / (std::sqrt(2.0e6) - 1.0);
        PointSource<double> a(pos, 0.0, spin, TOL, d, d * M_PI / 0.995, -0.995, 0.995, -M_PI, M_PI);
        a.run_raytrace(Integrator::RK4, M_PI_2, 1000.0, -250000);
        int traced = 0;
        for (int i = 0; i < a.get_count(); i++) traced += a.rays[i].steps > 0;
        CHECK(traced > 1900000, "traced %d", traced);
        std::printf(failures ? "FAIL\n" : "PASS\n");
        return failures ? 1 : 0;
    }

    // `host_api_test step-control`: the constructor's tol and the three setters reach the kernels as the kr_params fields of the C ABI.  A source run
    // through the class must leave, bit for bit, the records of kr_trace_f64 called with the same kr_params on the same initial rays -- under
    // tol = 7, set_max_tstep(0.3, 20), set_max_phistep(0.01), set_boundary(3.0), and again after set_boundary() has put the event horizon back.
    // set_precision(1, 1) changes nothing: the reference's setter assigns its parameters to themselves, and that no-op is part of the contract.
    if (argc > 1 && !std::strcmp(argv[1], "step-control")) {
        static_assert(sizeof(Ray<double>) == sizeof(kr_ray_f64), "Ray<double> is the C ABI's record");
        for (int pass = 0; pass < 2; pass++) {
            PointSource<double> a(pos, 0.0, spin, 7.0, 0.05, 0.05, -0.995, 0.995, -M_PI, M_PI);
            a.redshift_start();
            std::vector<kr_ray_f64> direct(a.get_count());
            std::memcpy(direct.data(), a.rays, sizeof(kr_ray_f64) * direct.size());
            a.set_max_tstep(0.3, 20.0);
            a.set_max_phistep(0.01);
            a.set_boundary(3.0);
            if (pass == 1) a.set_boundary();
            a.set_precision(1.0, 1.0);
            a.set_precision(1.0);
            a.run_raytrace(Integrator::RK4, M_PI_2, 1000.0, 0);

            kr_params p;
            std::memset(&p, 0, sizeof p);
            p.spin = spin;
            p.horizon = pass == 0 ? 3.0 : kr_kerr_horizon(spin);
            p.precision = 7.0;
            p.theta_precision = THETA_PRECISION;
            p.max_tstep = 0.3;
            p.maxtstep_rlim = 20.0;
            p.max_phistep = 0.01;
            p.rk45_tol = 1e-8;
            p.r_max = 1000.0;
            p.theta_max = M_PI_2;
            p.integrator = KR_RK4;
            p.stop_kind = KR_STOP_THETA;
            p.steplim = -1;
            p.flags = KR_FLAG_HYBRID;             // the class's arithmetic for the theta-limit overloads (KRTRACE_ARITHMETIC unset)
            CHECK(a.calculate_horizon() == kr_kerr_horizon(spin), "calculate_horizon() %.17g vs kr_kerr_horizon %.17g", a.calculate_horizon(), kr_kerr_horizon(spin));
            const int rc = kr_trace_f64(&p, direct.data(), (int64_t) direct.size(), nullptr);
            CHECK(rc == 0, "kr_trace_f64: %d (%s)", rc, kr_last_error());
            int live = 0, differ = 0, deep = 0;
            for (int i = 0; i < a.get_count(); i++) {
                if (direct[i].steps == -1) { CHECK(a.rays[i].steps == -1, "ray %d: unused slot was traced", i); continue; }
                ++live;
                // (a ray that ends with every coordinate NaN is the same ray whatever the NaN's sign bit)
                const double* x = &a.rays[i].t; const double* y = &direct[i].t;
                bool same = a.rays[i].steps == direct[i].steps && a.rays[i].status == direct[i].status && a.rays[i].rdot_sign == direct[i].rdot_sign &&
                            a.rays[i].thetadot_sign == direct[i].thetadot_sign && a.rays[i].rdot_flips == direct[i].rdot_flips &&
                            a.rays[i].equatorial_crossings == direct[i].equatorial_crossings;
                for (int f = 0; f < 13; f++) same = same && (!std::memcmp(x + f, y + f, sizeof(double)) || (std::isnan(x[f]) && std::isnan(y[f])));
                if (!same && differ++ < 5) std::printf("pass %d ray %d: class steps %d r %.17g, direct steps %d r %.17g\n", pass, i, a.rays[i].steps, a.rays[i].r, direct[i].steps, direct[i].r);
                if (direct[i].r < 2.9) ++deep;
            }
            CHECK(live == 5040, "pass %d: %d live rays", pass, live);
            CHECK(differ == 0, "pass %d: %d of %d records differ from kr_trace_f64 with the same kr_params", pass, differ, live);
            // the boundary is felt: while it is set a ray stops within a step of r = 3 (the MIN_STEP floor carries it just across), none goes on
            // towards the event horizon; once that is back, many do
            CHECK(pass == 0 ? deep == 0 : deep > 100, "pass %d: %d rays ended inside r = 2.9", pass, deep);
        }
        std::printf(failures ? "FAIL\n" : "PASS\n");
        return failures ? 1 : 0;
    }

    // 1. whole-array run_raytrace == per-ray propagate_rk4 (single-ray launches of the same kernel)
    {
        PointSource<double> a(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        PointSource<double> b(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        a.run_raytrace(Integrator::RK4, M_PI_2, 1000.0, 0);
        int moved = 0;
        for (int i = 0; i < b.get_count(); i += 7) {
            if (b.rays[i].steps < 0) continue;
            const int st = b.propagate_rk4(i, 1000.0, M_PI_2, STEPLIM);
            CHECK(st == a.rays[i].steps, "ray %d: propagate_rk4 returned %d steps, run_raytrace %d", i, st, a.rays[i].steps);
            CHECK(b.rays[i].r == a.rays[i].r && b.rays[i].t == a.rays[i].t && b.rays[i].status == a.rays[i].status, "ray %d state differs", i);
            ++moved;
        }
        CHECK(moved > 10, "too few rays compared");
        // the single-ray forms have no skip rule and take steplim verbatim (reference raytracer.cpp:129-340): a ray marked
        // unused (steps == -1) is traced all the same, and steplim <= 0 means zero iterations + RAY_STATUS_STEPLIM
        PointSource<double> c(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        int live = -1;
        for (int i = 0; i < c.get_count(); i++) if (c.rays[i].steps == 0 && a.rays[i].steps > 5) { live = i; break; }
        CHECK(live >= 0, "no live ray found");
        c.rays[live].steps = -1;
        const int st1 = c.propagate_rk4(live, 1000.0, M_PI_2, STEPLIM);
        CHECK(st1 == a.rays[live].steps && c.rays[live].steps == st1 - 1 && c.rays[live].r == a.rays[live].r, "steps == -1 ray: returned %d, record %d (run_raytrace took %d)", st1,
              c.rays[live].steps, a.rays[live].steps);
        PointSource<double> z(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        const double r_before = z.rays[live].r;
        z.rays[live].steps = 7;
        const int st0 = z.propagate_rk4(live, 1000.0, M_PI_2, 0);
        CHECK(st0 == 0 && z.rays[live].r == r_before && (z.rays[live].status & RAY_STATUS_STEPLIM) && z.rays[live].steps == -7, "steplim = 0: returned %d, steps %d status %d", st0,
              z.rays[live].steps, z.rays[live].status);
        // a bounded call followed by the rest equals the one-shot result
        PointSource<double> h2(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        const int part = h2.propagate_rk4(live, 1000.0, M_PI_2, 3);
        CHECK(part == 3 && h2.rays[live].steps == -3, "bounded call: returned %d, steps %d", part, h2.rays[live].steps);
    }

    // 2. the float instantiation traces on the GPU too and lands near the double result
    {
        float posf[4] = {0.f, 10.f, 1e-3f, 1.5707f};
        PointSource<float> f(posf, 0.f, 0.998f, TOL, 0.2f, 0.2f, -0.995f, 0.995f, (float) -M_PI, (float) M_PI);
        PointSource<double> d(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        f.redshift_start();
        d.redshift_start();
        f.run_raytrace(Integrator::RK4, (float) M_PI_2, 1000.f, 0, 0, 1, -1, -1, true, 20000);
        d.run_raytrace(Integrator::RK4, M_PI_2, 1000.0, 0, 0, 1, -1, -1, true, 20000);
        f.range_phi();
        f.redshift(-1.0f);
        d.range_phi();
        d.redshift(-1.0);
        int close = 0, live = 0;
        const int n = std::min(f.get_count(), d.get_count());
        for (int i = 0; i < n; i++) {
            if (d.rays[i].steps <= 0 || f.rays[i].steps <= 0 || d.rays[i].status != 1) continue;
            ++live;
            if (f.rays[i].status == 1 && std::fabs(f.rays[i].r - d.rays[i].r) < 2e-2 * d.rays[i].r && std::fabs(f.rays[i].redshift - d.rays[i].redshift) < 1e-2) ++close;
        }
        CHECK(live > 50 && close > 0.9 * live, "float vs double: %d of %d disc rays close", close, live);
    }

    // 3. RayDestination overloads: built-ins go to the kernel; Euler and user subclasses are refused loudly
    {
        PointSource<double> s(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        PointSource<double> ref(pos, 0.0, spin, TOL, 0.2, 0.2, -0.995, 0.995, -M_PI, M_PI);
        FlatDiscDestination<double> flat(M_PI_2);
        s.redshift_start();
        ref.redshift_start();
        s.run_raytrace(&flat, Integrator::RK4, 1000.0, 0);
        ref.run_raytrace(Integrator::RK4, M_PI_2, 1000.0, 0);
        int same = 0, live = 0;
        for (int i = 0; i < s.get_count(); i++) {
            if (ref.rays[i].steps <= 0 || ref.rays[i].status != 1) continue;
            ++live;
            if (s.rays[i].status == 1 && s.rays[i].theta >= M_PI_2 && std::fabs(s.rays[i].r - ref.rays[i].r) < 0.1 * ref.rays[i].r) ++same;   // no theta clip in the dest overload: it lands up to one step past the plane
        }
        CHECK(live > 50 && same > 0.9 * live, "FlatDiscDestination vs theta limit: %d of %d", same, live);

        bool threw = false;
        try { s.run_raytrace(&flat, Integrator::Euler, 1000.0, 0); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw, "Euler + RayDestination must throw (reference asserts)");
        SlowDisc<double> custom;
        threw = false;
        try { s.run_raytrace(&custom, Integrator::RK4, 1000.0, 0); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw, "user-defined RayDestination must be refused by run_raytrace");
        threw = false;
        try { s.run_raytrace(Integrator::RK4, M_PI_2, 1000.0, 0, (TextOutput*) 0x1); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw, "outfile != nullptr must be refused");

        // redshift(dest): built-in -> device kernel; custom velocity field -> host loop through the virtual call
        s.redshift(&flat);
        std::vector<double> g_kep(s.get_count());
        for (int i = 0; i < s.get_count(); i++) g_kep[i] = s.rays[i].redshift;
        s.redshift(-1.0);
        int agree = 0, n_disc = 0;
        for (int i = 0; i < s.get_count(); i++) {
            if (s.rays[i].steps <= 0 || s.rays[i].status != 1) continue;
            ++n_disc;
            if (std::fabs(s.rays[i].redshift - g_kep[i]) < 1e-12 * std::fabs(g_kep[i])) ++agree;   // Keplerian either way
        }
        CHECK(n_disc > 50 && agree == n_disc, "redshift(dest) vs redshift(-1): %d of %d", agree, n_disc);
        s.redshift(&custom);
        int differ = 0;
        for (int i = 0; i < s.get_count(); i++)
            if (s.rays[i].steps > 0 && s.rays[i].status == 1 && std::fabs(s.rays[i].redshift - g_kep[i]) > 1e-6) ++differ;
        CHECK(differ > n_disc / 2, "custom velocity field had no effect (%d)", differ);
    }

    // 4. ImagePlane helpers and the reverse redshift pair
    {
        ImagePlane<double> ip(10000.0, 80.0, -30.0, 30.0, 4.0, -30.0, 30.0, 4.0, spin, 0.0);
        CHECK(ip.get_count() == 256 && ip.get_x_index(17) == 1 && ip.get_y_index(17) == 1, "ImagePlane indexing");
        CHECK(ip.ray_x(16) == -26.0 && ip.ray_y(3) == -18.0, "ray_x/ray_y");
        ip.redshift_start();
        ip.run_raytrace(Integrator::RK4, M_PI_2, 11000.0, 0);
        ip.redshift(false);
        ip.range_phi();
        int hits = 0;
        for (int i = 0; i < ip.get_count(); i++)
            if (ip.rays[i].steps > 0 && ip.rays[i].status == 1 && ip.rays[i].redshift > 0.3 && ip.rays[i].redshift < 3) ++hits;
        CHECK(hits > 100, "image plane disc hits with sane redshift: %d", hits);
    }

    std::printf(failures ? "FAILED (%d)\n" : "PASS\n", failures);
    return failures ? 1 : 0;
}
