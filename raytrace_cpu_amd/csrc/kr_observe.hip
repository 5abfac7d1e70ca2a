// kr_observe.hip -- observing a volume map: camera rays are marched back through the emitting volume and, AS THEY STEP, gather the emissivity of the
// cells they cross into an energy spectrum, an energy-time response and a per-ray total (reference src/source_tracer/source_tracer.cpp,
// SourceTracer::propagate_source :102-310, stale there as Mapper was), as a third recorder on the trace's own persistent-wave loop.
//
// fp64, strict arithmetic, Euler and RK4 only.  ObserveRecorder below rides trace_body (kr_trace_loop.hpp) with the recorders' shared pieces
// (kr_recorder.hpp).  VolumeRecorder scatters into cells; this one is its mirror image: it gathers from cells and accumulates per ray, per energy bin
// and per (energy, time) bin.
//
// The rule (include/kr_trace.h states it in full).  ROWS, CELL and the energy shift are the shared ones.  The step that produced a row moved the lane
// from its state at before_step (the previous row, or the initial record) by (dr, dtheta, dphi); its proper length at the row is
//     l = sqrt((Sigma / Delta) dr^2 + Sigma dtheta^2 + (A sin^2 theta / Sigma) dphi^2)
// and a row in a cell with j = emis[cell] > 0 whose energy shift z = redshift_value is positive and finite adds w = j l E^3 exp(-tau), E = 1 / z, to the
// ray's total, to spectrum[(int) q_e] and to response[(int) q_e][(int) q_t]; then tau += l kappa[cell].  tau and the total are per ray, 0 at the claim.
//
// Accumulation.  Neighbouring pixels have neighbouring energies, so the lanes of a wave pile onto a few spectrum bins.  Two forms are built
// (KR_OBSERVE_ACC; figures in profiles/volume_observe_ab.txt):
//   1   per wave and step, the lanes that contribute to the same energy bin are summed in registers first and ONE lane adds the sum and the head count
//       (wave_step_end: at most kAggRounds bins per step, lanes left over add for themselves); those of them that share the leader's (energy, time) bin
//       are summed for the response the same way, the others add their own response term;
//   0   every lane does its own global f64 atomics (global_atomic_add_f64 under -munsafe-fp-atomics: no compare-and-swap loop).
// Measured on 6.6e4 / 2.6e5 / 1.05e6 camera rays (64 / 256 x 64 / 1024 x 256 bins): form 1 observes in 11-14 / 22-29 / 72-82 ms, form 0 in 49-53 / 94-108 /
// 250-265 ms -- the plain form is 3.2-4.4 x slower everywhere, so form 1 is the product and form 0 stays behind the macro.
// The ray's total lives in a register and is stored once, in leave().  add_tallies_kernel adds the launch's six tallies into the output's tail.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kr_recorder.hpp"

#ifndef KR_OBSERVE_ACC
#define KR_OBSERVE_ACC 1
#endif
#ifndef KR_OBSERVE_EULER_WAVES
#define KR_OBSERVE_EULER_WAVES 3     // resident waves per SIMD the Euler instance's register allocation must allow (as kr_volume.hip's)
#endif
#ifndef KR_OBSERVE_RK4_WAVES
#define KR_OBSERVE_RK4_WAVES 2       // ... and the RK4 instances': their launch holds 8 waves per CU anyway (launch_observe), and with the registers of 2 per
                                     // SIMD they spill 32-64 bytes instead of 256-400: 1.5-17 % faster at every size measured (the Euler instance at 2: 3-16 %
                                     // slower at the two larger sizes; profiles/volume_observe_ab.txt)
#endif

namespace kr {

namespace {

constexpr int kObserveTallies = 6;                               // rows, in_grid, lit, contributions, bad_g, degenerate
constexpr int kObserveWords = kRecorderWord + kObserveTallies;   // the trace's counter words, then the tallies
constexpr long long kMaxBins = 1ll << 27;

struct ObserveGrid {
    CellGrid cells;
    ObserverFrame frame;
    double en0, den, log_den, t0, dt;            // log_den: log(den) from the host's C library (logbin_en)
    const double* __restrict__ emis;
    const double* __restrict__ kappa;            // or null: optically thin
    const double* __restrict__ delay;            // or null: 0
    int32_t nen, nt, logbin_en;
};

// The recorder of trace_body (kr_trace_loop.hpp lists the hooks).  out: the caller's [spectrum | hits | response | tallies]; image: double[n] or null.
struct ObserveRecorder {
    static constexpr bool kActive = true, kStoresRays = true, kWaveHook = KR_OBSERVE_ACC == 1;
    ObserveGrid g;                                 // the launch
    const kr_ray_f64* __restrict__ records;        // rays[]: emit is read at the claim (the loop's Lane does not carry it, and no kernel writes it)
    double* __restrict__ out;
    double* __restrict__ image;
    // this lane's ray
    double emit = 0, tau = 0, image_ray = 0;
    double r0 = 0, theta0 = 0, phi0 = 0;                      // before_step: where the step starts
    RowGate gate;
    int32_t dep_e = -1, dep_et = -1; double dep_w = 0;        // after_step -> wave_step_end: this step's contribution (dep_e < 0: none; dep_et < 0: no response term)
    // this lane's tallies
    unsigned long long rows = 0, in_grid = 0, lit = 0, contributions = 0, bad_g = 0, degenerate = 0;

    KR_DEV void at_slot(long long slot, bool take) { if (!take && image) image[slot] = 0.0; }
    KR_DEV void claim(long long slot)
    {
        tau = 0; image_ray = 0;
        emit = records[slot].emit;
    }
    KR_DEV void before_step(Lane<double>& s)
    {
        gate.before_step(s);
        r0 = s.r; theta0 = s.theta; phi0 = s.phi;
    }

    KR_DEV void add_spectrum(int32_t e, double w, double heads) const
    {
        atomicAdd(out + e, w);
        atomicAdd(out + g.nen + e, heads);
    }
    KR_DEV void add_response(int32_t et, double w) const { atomicAdd(out + 2 * (long long) g.nen + et, w); }

    // All 64 lanes, after every step of the wave: the lanes that contribute to the energy bin of the first contributing lane are summed and lane 0 adds
    // the sum; then the next bin, kAggRounds times at most; a lane whose bin nobody shares, or that is left over, adds for itself.  Inside a group the
    // lanes that share its first lane's (energy, time) bin are summed for the response, the others add their own term.
    KR_DEV void wave_step_end()
    {
        for_lane_groups<kAggRounds>(dep_e, [&](int32_t e, bool same, int lanes) {
            const double sum_w = wave_sum(same ? dep_w : 0.0);
            if ((threadIdx.x & 63) == 0) add_spectrum(e, sum_w, (double) lanes);
            if (g.nt > 0) {
                const int leader = __ffsll((long long) __builtin_amdgcn_ballot_w64(same)) - 1;
                const int32_t et = __builtin_amdgcn_readlane(dep_et, leader);
                const bool same_et = same && dep_et == et;
                const double sum_et = wave_sum(same_et ? dep_w : 0.0);
                if (et >= 0 && (threadIdx.x & 63) == 0) add_response(et, sum_et);
                if (same && !same_et && dep_et >= 0) add_response(dep_et, dep_w);
            }
        });
        if (dep_e >= 0) {
            add_spectrum(dep_e, dep_w, 1.0);
            if (dep_et >= 0) add_response(dep_et, dep_w);
            dep_e = -1;
        }
    }

    template <bool USE_DEST> KR_DEV bool after_step(Lane<double>& s, bool fin)
    {
        if (!gate.template row<USE_DEST>(s)) return fin;
        ++rows;
        const int32_t cell = g.cells.cell_of(s.r, s.theta, s.phi);
        if (cell < 0) return fin;
        ++in_grid;
        const double j = g.emis[cell];
        const double kap = g.kappa ? g.kappa[cell] : 0.0;
        if (!(j > 0) && !(kap > 0)) return fin;
        ++lit;
        const double dr = s.r - r0, dth = s.theta - theta0, dph = s.phi - phi0;
        const double a = g.frame.spin, r = s.r;
        double sn, cs;
        kr_sincos_f64(s.theta, sn, cs);
        const double sigma = r * r + (a * cs) * (a * cs);
        const double delta = r * r - 2 * r + a * a;
        const double big_a = (r * r + a * a) * (r * r + a * a) - a * a * delta * sn * sn;
        const double len = kr_sqrt((sigma / delta) * dr * dr + sigma * dth * dth + (big_a * sn * sn / sigma) * dph * dph);
        if (!(len > 0 && len < __builtin_huge_val() && kr_abs(dph) < kPi / 2)) { ++degenerate; return fin; }
        if (j > 0) {
            const double z = g.frame.row_shift(s, emit);
            if (!(z > 0 && z < __builtin_huge_val())) {
                ++bad_g;
            } else {
                const double E = 1 / z;
                double w = j * len * E * E * E;
                if (g.kappa) w = w * ::exp(-tau);
                image_ray += w;
                ++contributions;
                const double q_e = g.logbin_en ? kr_log(E / g.en0) / g.log_den : (E - g.en0) / g.den;
                if (q_e >= 0 && q_e < g.nen) {
                    const int32_t e = (int32_t) q_e;
                    int32_t et = -1;
                    if (g.nt > 0) {
                        const double T = s.t + (g.delay ? g.delay[cell] : 0.0);
                        const double q_t = (T - g.t0) / g.dt;
                        if (q_t >= 0 && q_t < g.nt) et = e * g.nt + (int32_t) q_t;
                    }
#if KR_OBSERVE_ACC == 1
                    dep_e = e; dep_et = et; dep_w = w;
#else
                    add_spectrum(e, w, 1.0);
                    if (et >= 0) add_response(et, w);
#endif
                }
            }
        }
        tau += len * kap;
        return fin;
    }
    KR_DEV void leave(long long idx) { if (image) image[idx] = image_ray; }
    KR_DEV void at_exit(int lane, unsigned long long* __restrict__ counters)
    {
        const unsigned long long tally[kObserveTallies] = {rows, in_grid, lit, contributions, bad_g, degenerate};
        flush_tallies(tally, lane, counters);
    }
};

// resident waves per SIMD the register allocation must allow: KR_OBSERVE_RK4_WAVES / KR_OBSERVE_EULER_WAVES above
template <bool RK4, bool USE_DEST>
__global__ void __attribute__((amdgpu_flat_work_group_size(kTraceBlock, kTraceBlock))) __attribute__((amdgpu_waves_per_eu(RK4 ? KR_OBSERVE_RK4_WAVES : KR_OBSERVE_EULER_WAVES, 8)))
observe_kernel(kr_ray_f64* __restrict__ rays, long long n, TraceConsts<double> c, ObserveGrid g, double* __restrict__ out, double* __restrict__ image,
               unsigned long long* __restrict__ counters)
{
    int has_prio = 0;
    trace_body<double, RK4 ? KR_RK4 : KR_EULER, USE_DEST, false, false, KR_REFILL_MIN, false, ObserveRecorder>(
        rays, n, c, counters, nullptr, nullptr, 0, nullptr, 0, has_prio, -1, 0, ObserveRecorder{g, rays, out, image});
}

}  // namespace

// everything that can be refused without a device (include/kr_trace.h lists it): what volume_validate refuses, then the bins
int observe_validate(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const char* who)
{
    const int rc = volume_validate(p, m, who);
    if (rc != KR_OK) return rc;
    if (!b) return invalid_arg(who, "null argument (bins)");
    if (b->nen < 1) return invalid_arg(who, "nen must be at least 1");
    if (b->nt < 0) return invalid_arg(who, "nt must not be negative (0: no response)");
    if (2 * (long long) b->nen + (long long) b->nen * b->nt > kMaxBins) return invalid_arg(who, "2 nen + nen nt is more than 2^27 bins");
    if (!positive_finite(b->den)) return invalid_arg(who, "den must be positive and finite");
    if (!std::isfinite(b->en0)) return invalid_arg(who, "en0 must be finite");
    if (b->logbin_en && !(b->den > 1)) return invalid_arg(who, "a logarithmic energy grid needs den > 1 (the ratio of successive edges)");
    if (b->logbin_en && !(b->en0 > 0)) return invalid_arg(who, "a logarithmic energy grid needs en0 > 0");
    if (b->nt > 0 && !positive_finite(b->dt)) return invalid_arg(who, "dt must be positive and finite when nt > 0");
    if (!std::isfinite(b->t0)) return invalid_arg(who, "t0 must be finite");
    return KR_OK;
}

int trace_observe_dev(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const void* d_emis, const void* d_kappa, const void* d_delay, void* d_rays,
                      int64_t n, void* d_out, void* d_image, hipStream_t st, kr_stats* stats)
{
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->rays_total = n; }
    if (n == 0) return KR_OK;
    ObserveGrid g;
    g.cells = cell_grid_of(m); g.frame = observer_frame_of(p, m);
    g.en0 = b->en0; g.den = b->den; g.log_den = b->logbin_en ? std::log(b->den) : 0.0; g.t0 = b->t0; g.dt = b->dt;
    g.emis = (const double*) d_emis; g.kappa = (const double*) d_kappa; g.delay = (const double*) d_delay;
    g.nen = b->nen; g.nt = b->nt; g.logbin_en = b->logbin_en;
    const long long nbins = 2 * (long long) b->nen + (long long) b->nen * b->nt;
    const TraceConsts<double> c = make_consts<double>(p, effective_steplim(p));
    unsigned long long h[kObserveWords];
    return run_recorder(st, kObserveWords, stats, [&](unsigned long long* counters) -> int {
        const int rc = dispatch_instance(p, [&](auto rk4, auto dest) {
            constexpr bool RK4 = decltype(rk4)::value, USE_DEST = decltype(dest)::value;
            return launch_recorder(observe_kernel<RK4, USE_DEST>, RK4, n, st, (kr_ray_f64*) d_rays, n, c, g, (double*) d_out, (double*) d_image, counters);
        });
        if (rc != KR_OK) return rc;
        hipLaunchKernelGGL(add_tallies_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*) counters, kObserveTallies, (double*) d_out + nbins);
        KR_LAUNCH_CHECK();
        return KR_OK;
    }, h);
}

}  // namespace kr
