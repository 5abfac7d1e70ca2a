// kr_trace_loop.hpp -- the persistent-wave ray loop (trace_body), once: the body of every trace kernel of kr_trace.hip and of the recording
// kernels of kr_paths.hip, kr_volume.hip and kr_observe.hip, with its constants, counter words and wave reductions.
// Free lanes, queue visits, the wave-aggregated claim, the skip
// rule, the per-ray reset, the zero-iteration case and the one store of a ray exist here and nowhere else, so "a recorded ray takes the very
// steps of a flags = 0 trace" holds by construction.
// A recorder (trace_body's last template parameter; NoRecorder below lists the hooks) is called at fixed points and nowhere else, every call
// behind `if constexpr` on its type: with NoRecorder the trace kernels are instruction for instruction what they are without hooks
// (scripts/isa_dump.sh + scripts/isa_diff.py on both builds; profiles/paths_shared_loop_ab.txt).  A hook may keep per-lane state, park the
// lane's status round the step, end the ray and store to buffers of its own; it may not change what the step computes nor take part in the
// queue protocol.  Whether rays[] is stored to at all is a property of the recorder's type.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "kr_common.hpp"
#include "kr_device.hpp"
#include "kr_ray_io.hpp"

namespace kr {

namespace {

// Trace kernels: ONE wave per workgroup -- a wave gives its registers back the moment IT has finished, not when the slowest of four has
// (main launch 93.1 -> 87.2 ms at 1e7 rays against 256-thread workgroups).  The HOG instances (the strict side launch) too: their first claims
// are static (wave g takes list slots 64 g ..), so the listed rays go to the lowest-numbered workgroups -- which the dispatcher spreads over as
// many compute units -- and every other workgroup leaves at once.  (Four HOG waves per workgroup, i.e. a workgroup that owns its compute unit,
// measured worse: four lone waves on one CU slow one another down more than nine waves of the main launch do; profiles/r03_ab_experiments.txt.)
constexpr int kTraceBlock = 64;
// A wave goes back to the queue when at least this many of its lanes are free (or none holds a ray).  The refill / finish / store code runs with
// only the free lanes active: ~90 vector instructions per visit (92 in the RK4 main kernel's listing, a quarter of an RK4 step; ~500 when this was
// measured) and a round trip to memory.  Visiting for every single finished lane cost the image plane (1.25 lanes per visit) 11 % and the Euler launches
// 26 %; waiting for 4 leaves ~1.5 lanes of 64 idle on average.
// Measured 1 -> 4 (8 is the same): image plane 170.4 -> 151.7 ms, Euler 1e7 rays 55.2 -> 40.8, returning radiation 318 -> 307, headline 81.8 -> 80.7,
// RK45 412 -> 406 (profiles/r02_ab_experiments.txt).
#ifndef KR_REFILL_MIN
#define KR_REFILL_MIN 4
#endif
constexpr int kLongRaySteps = 2048;  // a wave whose oldest ray is older than 1 x / 3 x / 8 x this raises its issue priority to 1 / 2 / 3 (trace_body)
#ifndef KR_OCC_STATS
#define KR_OCC_STATS 0               // 1: lane-occupancy bookkeeping of the step loop (diagnostic builds: scripts/gpu_occ_stats.sh), printed by trace_wait
#endif
// Every launch of a trace has a block of counter words of its own in the workspace (device memory; copied out at the end of the trace): the queue
// head (slots handed out so far), rays traced, steps, rk45 attempts / rejects / stationary steps / extrapolated steps, steps of the launch's longest ray (atomicMax).
enum CounterWord { kHead, kTraced, kSteps, kAttempts, kRejects, kStationary, kExtrapolated, kLongest, kCounterWords,
                   // in the split bookkeeping block only (classify_kernel): the ill-conditioned rays that are not radial, the radial ones (both counts
                   // run on past what their lists hold), and whether either list overflowed
                   kFlagged = kTraced, kRadial = kSteps, kListsOverflowed = kAttempts };
constexpr int kGuardStatWord = 13;                                   // KR_GUARD_STATS builds: [13..21] the guards' tallies (kr_device.hpp: kGuardStatWords)
constexpr int kCounters = KR_GUARD_STATS ? kGuardStatWord + kGuardStatWords : KR_OCC_STATS ? 13 : kCounterWords;         // words per block; KR_OCC_STATS builds: [8..12] occupancy sums
constexpr int kRecorderWord = kCounters;                             // a launch with a recorder: the recorder's words from kRecorderWord on (at_exit)

template <typename T> struct RayOf;
template <> struct RayOf<double> { using type = kr_ray_f64; };
template <> struct RayOf<float> { using type = kr_ray_f32; };
// (load_ray / store_ray, make_consts, effective_steplim: kr_ray_io.hpp)

KR_DEV unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// (wave_sum: kr_common.hpp)

// workgroups of a persistent launch over n rays: what the device holds at once (single-wave workgroups per CU times CUs), never more than 64-ray loads
inline int persistent_grid(int cus, int blocks_per_cu, long long n)
{
    return (int) std::max<long long>(1, std::min<long long>((long long) cus * blocks_per_cu, (n + kTraceBlock - 1) / kTraceBlock));
}

// The recorder of a launch that records nothing.  What a recorder type provides (PathRecorder, kr_paths.hip; VolumeRecorder, kr_volume.hip;
// ObserveRecorder, kr_observe.hip; what the three share: kr_recorder.hpp):
//   kActive: the hooks below exist and are called;   kStoresRays: a ray's final record is stored to rays[] where it leaves its lane
//   at_slot(slot, take)     a lane has loaded the record of `slot`; take: it passed the skip rule          claim(slot)     the lane takes that ray
//   before_step(s), after_step<USE_DEST>(s, fin) -> fin     either side of the lane's step_fixed call     leave(idx)      ray idx leaves its lane
//   at_exit(lane, counters)     the wave has left the loop: per-lane tallies -> counters[kRecorderWord ..]
//   kWaveHook: wave_step_end() is called by ALL 64 lanes after every step of the wave (whole-wave reductions are valid there, not in after_step)
struct NoRecorder { static constexpr bool kActive = false, kStoresRays = true; };

// ---- the persistent loop ----------------------------------------------------------------------------
// METHOD: KR_EULER / KR_RK4 / KR_RK45.  REFILL_MIN: a wave goes back to the queue when at least this many of its
// lanes are free (or when none holds a ray).
// `list` (optional): the launch works on rays list[0 .. n) instead of rays 0 .. n); `n_ptr` (optional): the item count is read
// from device memory (the classification kernel of the split path produced it; see n_mode below); `mask` (optional): only
// rays with mask[i] == mask_want are traced (the others belong to another launch of the split).  HOG: the kernel claims the whole register
// file (512 VGPR+AGPR per lane), so each of its waves owns its SIMD and no other kernel's wave can be co-resident on
// the CUs it occupies -- used for the few ill-conditioned / long rays that define the critical path.  RADIAL (trace_side_kernel's
// radial waves): the wave's rays are integrated with step_radial, a lane whose ray turns out not to be radial with step_fixed.
// REC: the recorder (above); strict fp64 Euler / RK4 instances without radial waves only.
// STEP_REGS: what the fast theta-limit Euler / RK4 instances carry through the step loop besides a ray's constant terms (kr_device.hpp: StepRegs).
template <typename T, int METHOD, bool USE_DEST, bool FAST, bool HOG, int REFILL_MIN, bool RADIAL = false, typename REC = NoRecorder, int STEP_REGS = kStepRegsAll>
KR_DEV void trace_body(typename RayOf<T>::type* __restrict__ rays, long long n, const TraceConsts<T>& c, unsigned long long* __restrict__ counters,
                       const int* __restrict__ list, const unsigned long long* __restrict__ n_ptr, int n_mode, const unsigned char* __restrict__ mask, int mask_want,
                       int& has_prio, long long first_slot = -1, unsigned long long head_offset = 0, [[maybe_unused]] REC rec = REC())
{
    static_assert(!REC::kActive || (sizeof(T) == 8 && METHOD != KR_RK45 && !FAST && !RADIAL), "a recorder's step hooks stand round the strict fp64 step_fixed call");
    if (n_ptr) {
        // the item count was produced on the device (classify_kernel) and never visits the host:
        // n_mode 1: the first min(n, *n_ptr) list entries;  n_mode 2: all n slots, but only if *n_ptr says that a list overflowed (else nothing)
        const long long m = (long long) *n_ptr;
        n = (n_mode == 1) ? (m < n ? m : n) : (m != 0 ? n : 0);
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long lane_bit = 1ull << lane;

    Lane<T> s;
    [[maybe_unused]] RadialRay radial;      // RADIAL: the constants of this lane's ray (step_radial)
    // The fast Euler / RK4 instances keep the terms of (k, h, Q, a) that the potentials need (kr_fast.hpp: FastRayConsts) beside the lane state, like
    // `radial` above: computed once per ray instead of once per step.  (Not the fast RK45 instances: the trial's stages go through eval(), which forms
    // the terms itself, and that kernel has no registers to spare at 2 waves per SIMD.)  Every other instance: an empty struct.
    constexpr bool kRayConsts = FAST && sizeof(T) == 8 && METHOD != KR_RK45;
    static_assert(!(RADIAL && FAST), "the radial waves call step_fixed without a ray's constant terms: strict arithmetic only");
    [[maybe_unused]] RayConstsOf<kRayConsts> ray_consts;
    // The theta-limit ones among them also keep the ray's two signs as doubles (per ray, beside ray_consts) and a few of the launch's values in vector
    // registers (once, here): what k1 otherwise converts, reads back from spilled scalars or builds again in every step (kr_fast.hpp: FastRaySigns,
    // FastLaunchRegs).  Every other instance: empty structs.
    constexpr int kStepRegs = (kRayConsts && !USE_DEST) ? (STEP_REGS & (METHOD == KR_RK4 ? kStepRegsAll : ~(kStepNearLead | kStepQuiet))) : 0;      // (Euler has no stages, and scalar registers to spare)
    constexpr bool kSigns = (kStepRegs & kStepSigns) != 0, kLaunchRegs = kRayConsts && !USE_DEST;      // (always: FastLaunchRegs also holds what is merely read once -- equator_inside)
    [[maybe_unused]] RaySignsOf<kSigns> ray_signs;
    [[maybe_unused]] LaunchRegsOf<kLaunchRegs> launch_regs;
    if constexpr (kLaunchRegs) launch_regs = fast_launch_regs<kStepRegs>(c);
    long long idx = -1;
    bool have = false;          // this lane holds a ray
    bool pend = false;          // this lane's ray has ended and is still in its registers: written out at the wave's next visit to the queue (or on exit)
    bool exhausted = false;     // wave-uniform: the queue head has passed n
    unsigned long long my_steps = 0, my_traced = 0;
    int32_t my_longest = 0;     // most steps any of this lane's rays took in this call
    uint32_t my_attempts = 0, my_rejects = 0, my_stationary = 0, my_creep = 0;

#if KR_OCC_STATS
    unsigned long long occ_iters = 0, occ_tail_iters = 0, occ_tail_steps = 0, occ_refills = 0, occ_refill_lanes = 0;
#endif
#if KR_GUARD_STATS
    for (int i = 0; i < kGuardStatWords; ++i) s.guard_stats[i] = 0;
#endif
    for (;;) {
        const unsigned long long need = __builtin_amdgcn_ballot_w64(!have);      // (not __ballot: that one takes its predicate through a vector register and a compare)
        const int n_need = __popcll(need);
        const bool any_have = (need != ~0ull);

        // A wave visits the queue when enough of its lanes are free, and once more when it leaves: rays that have ended since the last visit are
        // written out there -- the ONE place in the kernel where a ray is stored.
        const bool visit = !exhausted && n_need > 0 && (n_need >= REFILL_MIN || !any_have);
        const bool leaving = !visit && !any_have;          // nothing held and nothing left to take
        if (visit || leaving) {
            if (pend) {
                // (not under a divergent branch of its own in the step loop: that branch ran in one wave iteration out of nine for a single
                // lane's ~40 instructions)
                my_steps += (unsigned long long) s.steps;
                my_longest = s.steps > my_longest ? s.steps : my_longest;
                if constexpr (REC::kStoresRays) store_ray(&rays[idx], s, finish_status<T, USE_DEST>(s, c));
                if constexpr (REC::kActive) rec.leave(idx);
                pend = false;
            }
            if (leaving) break;
            // The launch cannot end before its longest ray does, and a ray advances one step per iteration of ITS wave: a wave that carries a long
            // ray (orbiting / polar-axis rays: 2e4..1e7 steps against a median of ~450) is given issue priority over its SIMD neighbours so that the
            // critical path runs at single-wave speed instead of at 1/(waves per SIMD) of it -- graded: the longer the wave's oldest ray, the higher
            // its priority (0..3), so that the rays that define the critical path do not share their level with the many merely "longish" ones.
            // Re-evaluated here, at the queue visits (a wave that carries a long ray keeps visiting for its other 63 lanes until the queue is empty;
            // a counter in the step loop cost three vector instructions per step).  A wave that owns its SIMD (HOG) has nobody to overtake.
            if constexpr (!HOG) {
                const int32_t st = have ? s.steps : 0;
                auto any = [](bool x) { return __builtin_amdgcn_ballot_w64(x) != 0; };
                const int want_prio = any(st > 8 * kLongRaySteps) ? 3 : any(st > 3 * kLongRaySteps) ? 2 : any(st > kLongRaySteps) ? 1 : 0;
                if (want_prio != has_prio) {
                    has_prio = want_prio;
                    switch (want_prio) {
                        case 3: __builtin_amdgcn_s_setprio(3); break;
                        case 2: __builtin_amdgcn_s_setprio(2); break;
                        case 1: __builtin_amdgcn_s_setprio(1); break;
                        default: __builtin_amdgcn_s_setprio(0); break;
                    }
                }
            }
#if KR_OCC_STATS
            ++occ_refills; occ_refill_lanes += n_need;
#endif
            // wave-aggregated dequeue: one atomic for all free lanes
            const int leader = __ffsll((long long) need) - 1;
            unsigned long long base = 0;
            if (first_slot >= 0) {
                // (HOG instances: this wave's first 64 slots are its own by position; the shared queue head counts from head_offset on)
                base = (unsigned long long) first_slot;
                first_slot = -1;
            } else {
                if (lane == leader) base = atomicAdd(&counters[kHead], (unsigned long long) n_need);
                base = __shfl(base, leader, 64) + head_offset;
            }
            if (base + (unsigned long long) n_need >= (unsigned long long) n) exhausted = true;
            if (!have) {
                const long long slot = (long long) base + __popcll(need & (lane_bit - 1));
                if (slot < n) {
                    // (the record is loaded beside its mask byte, not after it -- one memory round trip per visit instead of two; a ray that belongs to
                    // the other launch of a split, 0.03 % of them, is dropped again)
                    long long mine = slot;
                    if constexpr (HOG) { if (list) mine = (long long) list[slot]; }          // (only side launches work from a list)
                    const unsigned char* launch = mask ? mask + slot : (const unsigned char*) &rays[mine];      // one straight line of loads, mask or not
                    const unsigned char launch_of_ray = *launch;
                    load_ray(&rays[mine], s);
                    // skip rule of run_raytrace (raytracer.cpp:116-117; the serial path with an outfile: :91-92 -- a skipped ray has no rows and no blank lines)
                    const bool take = (!mask || launch_of_ray == (unsigned char) mask_want) && s.steps0 >= 0 && s.steps0 < c.steplim;
                    if constexpr (REC::kActive) rec.at_slot(slot, take);
                    if (take) {
                        idx = mine;
                        have = true;
                        ++my_traced;
                        s.steps = 0;
                        s.r_was_positive = false;
                        s.theta_was_positive = true;
                        s.in_retry = false;
                        s.creep_m = 0;
                        s.creep_run = 0;
                        s.creep_mode = false;
                        s.fsal_valid = false;
                        energy_guard_set(s);
                        // (the one place a lane takes a ray: its lanes only -- the others keep the terms of the rays they hold)
                        if constexpr (kRayConsts) ray_consts = fast_ray_consts(s.k, s.h, s.Q, c.a);
                        if constexpr (kSigns) { ray_signs.rdot = (double) s.rdot_sign; ray_signs.thetadot = (double) s.thetadot_sign; }      // (whatever the record holds: a ray mid-flight too)
                        if (METHOD == KR_RK45) rk45_seed(s, c);
                        if constexpr (RADIAL) radial_claim(s, c, radial);
                        if constexpr (REC::kActive) rec.claim(slot);
                        if (!loop_cond<T, USE_DEST>(s, c)) {
                            // zero-iteration call: only the epilogue runs (at the next visit)
                            have = false;
                            pend = true;
                        }
                    }
                }
            }
            continue;   // re-evaluate the ballots (skipped / zero-iteration rays leave lanes free)
        }

        int replay_batch = 1;
        if constexpr (METHOD == KR_RK45 && sizeof(T) == 8) {
            // the tail of an RK45 launch is waves that hold nothing but creeping captured rays: they take 16 cheap steps per iteration
            if (!__any(have && !s.creep_mode)) replay_batch = 16;      // (__any, not the ballot builtin: with the builtin this kernel's allocation came out 19 % slower)
        }
#if KR_OCC_STATS
        ++occ_iters;
        if (exhausted) { ++occ_tail_iters; occ_tail_steps += have ? 1 : 0; }
#endif
        if constexpr (RADIAL) {
            // every wave of a radial launch runs the radial body only; a lane whose ray is not provably radial (radial_claim, or a step that step_radial
            // handed back) is the exception, out of line
            bool fin = false;
            if (have && !radial.general) fin = step_radial<METHOD == KR_RK4>(s, radial, c);
            const bool general = have && radial.general;
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(general) != 0, false)) {
                if (general) fin = step_fixed<T, METHOD == KR_RK4, USE_DEST, FAST, HOG>(s, c);      // (radial waves are strict: no ray constants)
            }
            if (fin) {
                have = false;
                pend = true;
            }
        } else if (have) {
            if constexpr (REC::kActive) rec.before_step(s);
            bool fin;
            if constexpr (kSigns && kLaunchRegs) fin = step_fixed<T, METHOD == KR_RK4, USE_DEST, FAST, HOG>(s, c, &ray_consts, &ray_signs, &launch_regs);
            else if constexpr (kSigns) fin = step_fixed<T, METHOD == KR_RK4, USE_DEST, FAST, HOG>(s, c, &ray_consts, &ray_signs);
            else if constexpr (kLaunchRegs) fin = step_fixed<T, METHOD == KR_RK4, USE_DEST, FAST, HOG>(s, c, &ray_consts, nullptr, &launch_regs);
            else if constexpr (kRayConsts) fin = step_fixed<T, METHOD == KR_RK4, USE_DEST, FAST, HOG>(s, c, &ray_consts);
            else if (METHOD == KR_EULER) fin = step_fixed<T, false, USE_DEST, FAST, HOG>(s, c);
            else if (METHOD == KR_RK4) fin = step_fixed<T, true, USE_DEST, FAST, HOG>(s, c);
            else fin = step_rk45<T, USE_DEST, FAST, HOG>(s, c, my_attempts, my_rejects, my_stationary, my_creep, replay_batch);
            if constexpr (REC::kActive) fin = rec.template after_step<USE_DEST>(s, fin);
            if (fin) {
                have = false;
                pend = true;
            }
        }
        if constexpr (REC::kActive) { if constexpr (REC::kWaveHook) rec.wave_step_end(); }
    }
    // per-wave totals -> global counters (4 atomics per wave, once)
    const unsigned long long w_traced = wave_sum(my_traced);
    const unsigned long long w_steps = wave_sum(my_steps);
    const unsigned long long w_att = wave_sum((unsigned long long) my_attempts);
    const unsigned long long w_rej = wave_sum((unsigned long long) my_rejects);
    const unsigned long long w_sta = wave_sum((unsigned long long) my_stationary);
    const unsigned long long w_creep = wave_sum((unsigned long long) my_creep);
    const unsigned long long w_longest = wave_max((unsigned long long) my_longest);
#if KR_OCC_STATS
    {
        const unsigned long long w_tail_steps = wave_sum(occ_tail_steps);
        if (lane == 0) {
            atomicAdd(&counters[8], occ_iters); atomicAdd(&counters[9], occ_tail_iters); atomicAdd(&counters[10], w_tail_steps);
            atomicAdd(&counters[11], occ_refills); atomicAdd(&counters[12], occ_refill_lanes);
        }
    }
#endif
#if KR_GUARD_STATS
    for (int i = 0; i < kGuardStatWords; ++i) {
        const unsigned long long w = wave_sum(s.guard_stats[i]);
        if (lane == 0 && w) atomicAdd(&counters[kGuardStatWord + i], w);
    }
#endif
    if (lane == 0) {
        if (w_longest) atomicMax(&counters[kLongest], w_longest);
        if (w_sta) atomicAdd(&counters[kStationary], w_sta);
        if (w_creep) atomicAdd(&counters[kExtrapolated], w_creep);
        if (w_traced) atomicAdd(&counters[kTraced], w_traced);
        if (w_steps) atomicAdd(&counters[kSteps], w_steps);
        if (w_att) atomicAdd(&counters[kAttempts], w_att);
        if (w_rej) atomicAdd(&counters[kRejects], w_rej);
    }
    if constexpr (REC::kActive) rec.at_exit(lane, counters);
}

}  // namespace

}  // namespace kr
