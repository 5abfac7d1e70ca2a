// kr_crossings.hip -- equatorial crossings: where and when a ray meets the plane theta = pi / 2, every time it does, with the energy shift of an
// emitter on the plane there -- the order-resolved images of a disc (the n-th crossing of a camera ray is the n-th-order image), as a fourth recorder
// on the trace's own persistent-wave loop.
//
// fp64, strict arithmetic, Euler and RK4 only -- the instances of kr_paths.hip.  CrossingRecorder below rides trace_body (kr_trace_loop.hpp) exactly as
// VolumeRecorder does: a recorded ray is claimed, reset, stepped and stored by the very code a flags = 0 trace runs, so a ray the recorder does not end
// finishes with that trace's record, bit for bit.  This file has no loop of its own.
//
// The rule (include/kr_trace.h states it in full).  An iteration CROSSED iff the trace's own counter equatorial_crossings moved in it (crossed_equator,
// kr_device.hpp): a theta-flip iteration never does; one that ends on the horizon or on dest->reached() does like any other -- the disc of a
// KR_STOP_DISC_ISCO trace is met in exactly such an iteration -- so this recorder does not use RowGate and never parks the lane's status.  With the
// lane's (t, r, theta, phi) before the iteration (0) and after it (1, after reflect_poles):
//     f = (pi/2 - theta0) / (theta1 - theta0)      r_c = r0 + f (r1 - r0)     phi_c = phi0 + f (phi1 - phi0)     t_c = t0 + f (t1 - t0)
// every operation a single IEEE one (-ffp-contract=off), and g = redshift_value (kr_post_device.hpp: the function the redshift pass applies) at
// (r_c, pi/2) with the ray's k, h, Q and emit and the lane's signs after the step.  Crossing number `seen` (from 0) of the ray in slot i goes to
// rows[(i M + seen) 4 ..] = {r_c, phi_c, t_c, g} while seen < M; g is stored as computed (NaN or <= 0 included: consumers filter); ++seen always.
//
// Ending a ray.  With stop_when_full the iteration that makes the M-th crossing returns fin = true: the ray ends with that iteration's state and
// its record is what the loop's epilogue (finish_status) makes of it -- the mechanism of a path recording that leaves its window.  The recorder adds no
// status bit of its own: the record carries the ERGO / NEG_ENERGY flags the steps raised, HORIZON or DEST if that very iteration ended on one (it
// would have ended anyway), and of the epilogue's bits those its state satisfies -- STEPLIM if it was the ray's steplim-th iteration, RLIM if
// r >= rlim, DEST (theta-limit instances) if theta left the limits -- in practice none: a ray cut short in mid-flight has status 0 and steps > 0.
//
// No atomics and no tallies: a lane stores only into the slab of the ray it holds and into seen[] of the slots it visited.  Rows m >= min(seen, M)
// of a ray are not written; seen[i] is written for every slot, 0 for a ray the skip rule passed over.
//
// Registers.  Per lane the recorder adds four doubles (the state before the step), eq_cross before the step, seen, emit and the slab pointer: 14
// vector registers that live across the step.  KR_CROSSINGS_RK4_WAVES / KR_CROSSINGS_EULER_WAVES below say what was chosen and why
// (profiles/crossings_ab.txt has the figures).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kr_recorder.hpp"

// Resident waves per SIMD the register allocation must allow (amdgpu_waves_per_eu's lower bound): 3 for every instance, by measurement
// (profiles/crossings_ab.txt; scripts/kernel_resources.sh for the allocations, scripts/crossings_ab.py for the times).
//   at 3 (168 VGPRs): scratch 48 bytes per lane (Euler), 64 (RK4 to the theta limit), 144 (RK4 to a destination) -- the path recorder's record
//     instances have 48 / 32 / 96, the volume recorder's 144 / 160 / 272;
//   Euler at 4 (128 VGPRs, the path recorder's choice): 160 bytes of scratch, and 3-6 % SLOWER on the two lamp posts (best of three 42.5 against
//     40.0 ms and 42.1 against 41.0 ms), the same on the image plane (145.7 against 145.2 ms): the volume recorder's finding (KR_VOLUME_EULER_WAVES);
//   RK4 at 2 (183 VGPRs, 32 bytes of scratch): 5 % and 20 % slower on the lamp posts when the rays run on (292.6 against 278.4 ms, 101.8 against
//     84.8 ms), within 4 % either way everywhere else.  (launch_recorder holds 2 RK4 waves per SIMD whatever this bound says: the bound only
//     decides the allocation, and the looser one did not buy a faster schedule.)
#ifndef KR_CROSSINGS_RK4_WAVES
#define KR_CROSSINGS_RK4_WAVES 3
#endif
#ifndef KR_CROSSINGS_EULER_WAVES
#define KR_CROSSINGS_EULER_WAVES 3
#endif

namespace kr {

namespace {

constexpr int kCrossingWords = kRecorderWord;      // the trace's counter words; the recorder has no tallies
constexpr int kMaxCrossings = 16;

// What the kernel is handed, doubles first (see VolumeArgs, kr_volume.hip).
struct CrossingArgs {
    double V, spin;
    int32_t max_crossings, stop_when_full, reverse, projradius, motion;
};

// The recorder of trace_body (kr_trace_loop.hpp lists the hooks).  rows: double[n][M][4]; seen: int32[n].
struct CrossingRecorder {
    static constexpr bool kActive = true, kStoresRays = true, kWaveHook = false;
    CrossingArgs a;                                // the launch
    const kr_ray_f64* __restrict__ records;        // rays[]: emit is read at the claim (the loop's Lane does not carry it, and no kernel writes it)
    double* __restrict__ rows;
    int32_t* __restrict__ seen_out;
    // this lane's ray
    double emit = 0;
    double* slab = nullptr;                        // rows of its slot
    int32_t seen = 0;
    double t0 = 0, r0 = 0, theta0 = 0, phi0 = 0; int32_t eq0 = 0;      // before_step -> after_step

    KR_DEV void at_slot(long long slot, bool take)
    {
        if (!take) seen_out[slot] = 0;
    }
    KR_DEV void claim(long long slot)
    {
        seen = 0;
        emit = records[slot].emit;
        slab = rows + slot * (long long) (4 * a.max_crossings);
    }
    KR_DEV void before_step(Lane<double>& s)
    {
        t0 = s.t; r0 = s.r; theta0 = s.theta; phi0 = s.phi; eq0 = s.eq_cross;
    }
    template <bool USE_DEST> KR_DEV bool after_step(Lane<double>& s, bool fin)
    {
        if (s.eq_cross != eq0) {
            if (seen < a.max_crossings) {
                const double f = (kPi2 - theta0) / (s.theta - theta0);
                const double r_c = r0 + f * (s.r - r0);
                const double phi_c = phi0 + f * (s.phi - phi0);
                const double t_c = t0 + f * (s.t - t0);
                kr_ray_f64 at;
                at.r = r_c; at.theta = kPi2; at.k = s.k; at.h = s.h; at.Q = s.Q; at.rdot_sign = s.rdot_sign; at.thetadot_sign = s.thetadot_sign; at.emit = emit;
                const double g = redshift_value<kr_ray_f64>(at, a.spin, a.V, a.reverse, a.projradius, a.motion);
                double2* q = reinterpret_cast<double2*>(slab + 4 * seen);      // (seen < M: inside the ray's slab)
                q[0] = make_double2(r_c, phi_c);
                q[1] = make_double2(t_c, g);
            }
            ++seen;
            if (a.stop_when_full && seen == a.max_crossings) fin = true;
        }
        return fin;
    }
    KR_DEV void leave(long long idx) { seen_out[idx] = seen; }
    KR_DEV void at_exit(int, unsigned long long* __restrict__) {}
};

template <bool RK4, bool USE_DEST>
__global__ void __attribute__((amdgpu_flat_work_group_size(kTraceBlock, kTraceBlock)))
__attribute__((amdgpu_waves_per_eu(RK4 ? KR_CROSSINGS_RK4_WAVES : KR_CROSSINGS_EULER_WAVES, 8)))
crossings_kernel(kr_ray_f64* __restrict__ rays, long long n, TraceConsts<double> c, CrossingArgs a, double* __restrict__ rows, int32_t* __restrict__ seen,
                 unsigned long long* __restrict__ counters)
{
    int has_prio = 0;
    trace_body<double, RK4 ? KR_RK4 : KR_EULER, USE_DEST, false, false, KR_REFILL_MIN, false, CrossingRecorder>(
        rays, n, c, counters, nullptr, nullptr, 0, nullptr, 0, has_prio, -1, 0, CrossingRecorder{a, rays, rows, seen});
}

}  // namespace

// everything that can be refused without a device (include/kr_trace.h lists it): the spec, then what the recording loop refuses (paths_validate)
int crossings_validate(const kr_params* p, const kr_crossing_spec* sp, const char* who)
{
    if (!p || !sp) return invalid_arg(who, "null argument");
    if (const int rc = refuse_plunge(sp->V, who)) return rc;
    if (sp->max_crossings < 1 || sp->max_crossings > kMaxCrossings) return invalid_arg(who, "max_crossings must be 1..16");
    if (sp->motion != 0 && sp->motion != 1) return invalid_arg(who, "unknown motion (0: orbital, 1: radial)");
    const kr_path_spec every_row = {-1.0, -1.0, 1, 0};
    return paths_validate(p, &every_row, who);
}

int trace_crossings_dev(const kr_params* p, const kr_crossing_spec* sp, void* d_rays, int64_t n, void* d_rows, void* d_seen, hipStream_t st, kr_stats* stats)
{
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->rays_total = n; }
    if (n == 0) return KR_OK;
    const CrossingArgs a = {sp->V, p->spin, sp->max_crossings, sp->stop_when_full != 0, sp->reverse, sp->projradius, sp->motion};
    const TraceConsts<double> c = make_consts<double>(p, effective_steplim(p));
    unsigned long long h[kCrossingWords];
    return run_recorder(st, kCrossingWords, stats, [&](unsigned long long* counters) -> int {
        return dispatch_instance(p, [&](auto rk4, auto dest) {
            constexpr bool RK4 = decltype(rk4)::value, USE_DEST = decltype(dest)::value;
            return launch_recorder(crossings_kernel<RK4, USE_DEST>, RK4, n, st, (kr_ray_f64*) d_rays, n, c, a, (double*) d_rows, (int32_t*) d_seen, counters);
        });
    }, h);
}

}  // namespace kr
