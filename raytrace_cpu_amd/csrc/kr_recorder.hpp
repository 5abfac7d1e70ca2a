// kr_recorder.hpp -- what the recorders that ride trace_body (kr_trace_loop.hpp lists the hooks) share: PathRecorder (kr_paths.hip), VolumeRecorder
// (kr_volume.hip), ObserveRecorder (kr_observe.hip) and CrossingRecorder (kr_crossings.hip: the launch helpers only).  Which iterations are rows, which cell a row lies in, the energy shift at a row, the
// wave-aggregated add, the tallies and the way such a launch is sized, enqueued and read back are stated here once; the three files keep only what
// is particular to them.  The device helpers are forced-inline: each kernel compiles to the code it had with the lines written out.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>

#include "kr_pass.hpp"
#include "kr_trace_loop.hpp"

namespace kr {

namespace {

// ---- which iterations are rows ---------------------------------------------------------------------------------------------------------------
// Why an iteration of step_fixed ended is read off the lane afterwards, so the step functions stay as the trace kernels compile them:
//   theta flip (`continue`, writes nothing)   theta_was_positive went from true to false: only the flip clears it (k1_with_flips);
//   horizon / destination (`break` before the write)   the status bit the iteration added (the lane's status is parked during the step).
// A ROW is the state after the update of every iteration that is neither.
struct RowGate {
    bool flip_armed = false; int32_t status_before = 0;       // before_step -> row

    KR_DEV void before_step(Lane<double>& s) { flip_armed = s.theta_was_positive; status_before = s.status; s.status = 0; }
    // after the step: the lane's status is whole again; true iff the iteration left a row
    template <bool USE_DEST> KR_DEV bool row(Lane<double>& s)
    {
        const int32_t added = s.status;
        s.status = status_before | added;
        const bool flipped = flip_armed && !s.theta_was_positive;                               // `continue`
        const bool broke = (added & (KR_STATUS_HORIZON | (USE_DEST ? KR_STATUS_DEST : 0))) != 0;  // `break` before the row
        return !flipped && !broke;
    }
};

// ---- which cell a row lies in (include/kr_trace.h states the rule in full) ---------------------------------------------------------------------
//     q_r  = logbin ? log(r / r_min) / log(dr) : (r - r_min) / dr        q_th = theta / dtheta
//     q_ph = (phi_w + pi) / dphi,  phi_w = phi - 2 pi floor((phi + pi) / (2 pi))          (nphi == 1: no phi test, no wrap, iphi = 0)
// IN THE GRID iff 0 <= q < n on every axis, decided on q itself (a NaN or infinite q is outside, like kr_emis_bins); the cell is
// ((int) q_r * ntheta + (int) q_th) * nphi + (int) q_ph.  Apart from the log every operation is one IEEE operation (-ffp-contract=off).
struct CellGrid {
    double r_min, dr, log_dr, dtheta, dphi;      // log_dr: log(dr) from the host's C library (logbin)
    int32_t nr, ntheta, nphi, logbin;

    // the row's cell, or -1 outside the grid
    KR_DEV int32_t cell_of(double r, double theta, double phi) const
    {
        const double q_r = logbin ? kr_log(r / r_min) / log_dr : (r - r_min) / dr;
        const double q_th = theta / dtheta;
        if (!(q_r >= 0 && q_r < nr && q_th >= 0 && q_th < ntheta)) return -1;
        int32_t iphi = 0;
        if (nphi != 1) {
            const double phi_w = phi - (2 * kPi) * floor((phi + kPi) / (2 * kPi));
            const double q_ph = (phi_w + kPi) / dphi;
            if (!(q_ph >= 0 && q_ph < nphi)) return -1;
            iphi = (int32_t) q_ph;
        }
        return ((int32_t) q_r * ntheta + (int32_t) q_th) * nphi + iphi;
    }
};

inline CellGrid cell_grid_of(const kr_volume_map* m)
{
    return CellGrid{m->r_min, m->dr, m->logbin ? std::log(m->dr) : 0.0, m->dtheta, m->dphi, m->nr, m->ntheta, m->nphi, m->logbin};
}

// ---- the energy shift at a row -------------------------------------------------------------------------------------------------------------------
// g = redshift_value (kr_post_device.hpp: the function the redshift pass applies) at the row, with the lane's signs and the emit of the ray's record
struct ObserverFrame {
    double V, spin;
    int32_t reverse, projradius, motion;

    KR_DEV double row_shift(const Lane<double>& s, double emit) const
    {
        kr_ray_f64 at;
        at.r = s.r; at.theta = s.theta; at.k = s.k; at.h = s.h; at.Q = s.Q; at.rdot_sign = s.rdot_sign; at.thetadot_sign = s.thetadot_sign; at.emit = emit;
        return redshift_value<kr_ray_f64>(at, spin, V, reverse, projradius, motion);
    }
};

inline ObserverFrame observer_frame_of(const kr_params* p, const kr_volume_map* m) { return ObserverFrame{m->V, p->spin, m->reverse, m->projradius, m->motion}; }

// ---- the wave-aggregated add ---------------------------------------------------------------------------------------------------------------------
constexpr int kAggRounds = 8;      // keys (cells, energy bins) per wave and step whose lanes are summed before they add

// All 64 lanes, from wave_step_end.  key >= 0: this lane has something to add under that key.  The lanes that share the key of the first such lane
// are a group: f(key, same, lanes) is called by all 64 lanes -- `same`: this lane is in the group; whole-wave reductions are valid in f -- and the
// group's lanes are done (key = -1); then the next key, ROUNDS times at most.  A group of one is skipped.  On return key >= 0 only in the lanes
// that must add for themselves: those nobody shares a key with, and those left over.
template <int ROUNDS, typename F>
KR_DEV void for_lane_groups(int32_t& key, F&& f)
{
    unsigned long long todo = __builtin_amdgcn_ballot_w64(key >= 0);
    if (todo == 0) return;
#pragma unroll 1
    for (int round = 0; round < ROUNDS && todo != 0; ++round) {
        const int leader = __ffsll((long long) todo) - 1;
        const int32_t k = __builtin_amdgcn_readlane(key, leader);
        const bool same = key == k;
        const unsigned long long group = __builtin_amdgcn_ballot_w64(same);
        todo &= ~group;
        if (__popcll(group) == 1) continue;          // (that lane adds for itself)
        f(k, same, __popcll(group));
        if (same) key = -1;
    }
}

// ---- tallies: counters[kRecorderWord + q] -------------------------------------------------------------------------------------------------------
// at_exit: this lane's tallies, summed over the wave, into the launch's counter words
template <int N>
KR_DEV void flush_tallies(const unsigned long long (&tally)[N], int lane, unsigned long long* __restrict__ counters)
{
    unsigned long long w[N];
#pragma unroll
    for (int q = 0; q < N; ++q) w[q] = wave_sum(tally[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q)
            if (w[q]) atomicAdd(&counters[kRecorderWord + q], w[q]);
    }
}

// after the launch: its tallies into the tail of the caller's output (atomics: launches of other streams may be adding into the same output)
__global__ void __launch_bounds__(64) add_tallies_kernel(const unsigned long long* __restrict__ counters, int n_tallies, double* __restrict__ tail)
{
    if ((int) threadIdx.x < n_tallies) {
        const unsigned long long v = counters[kRecorderWord + threadIdx.x];
        if (v) atomicAdd(tail + threadIdx.x, (double) v);
    }
}

// ---- launching -----------------------------------------------------------------------------------------------------------------------------------
// The persistent launch of a recording kernel over n rays.  Resident waves per SIMD as the strict trace sizes its launches (kr_trace.hip::launch):
// 2 for RK4 -- the pass ends with its longest ray, which advances one step per turn of its wave -- 4 for the short Euler step.
template <typename... P>
int launch_recorder(void (*kern)(P...), bool rk4, long long n, hipStream_t stream, std::common_type_t<P>... args)
{
    int dev = 0, cus = 0, per_cu = 0;
    KR_HIP(hipGetDevice(&dev));
    const int rc = device_cus(dev, &cus);
    if (rc != KR_OK) return rc;
    KR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kTraceBlock, 0));
    per_cu = std::max(1, std::min(per_cu, 4 * (rk4 ? 2 : 4)));
    hipLaunchKernelGGL(kern, dim3(persistent_grid(cus, per_cu, n)), dim3(kTraceBlock), 0, stream, args...);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

// f(RK4, USE_DEST), both std::bool_constant, for the instance that p asks for: Euler, RK4 to the theta limit, RK4 to a destination
template <typename F>
int dispatch_instance(const kr_params* p, F&& f)
{
    if (p->integrator == KR_EULER) return f(std::false_type{}, std::false_type{});
    if (p->stop_kind == KR_STOP_THETA) return f(std::true_type{}, std::false_type{});
    return f(std::true_type{}, std::true_type{});
}

// One timed recording launch: n_words zeroed counter words, launch(counters) between two events, the words copied to h_words[n_words] and the
// stream waited for; stats (optional): the kernel time and the trace's own words.
template <typename Launch>
int run_recorder(hipStream_t st, int n_words, kr_stats* stats, Launch&& launch, unsigned long long* h_words)
{
    struct Events {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        ~Events() { if (ev0) (void) hipEventDestroy(ev0); if (ev1) (void) hipEventDestroy(ev1); }
    } e;
    DeviceBuffer counters;
    int rc = counters.alloc(n_words * sizeof(unsigned long long));
    if (rc != KR_OK) return rc;
    KR_HIP(hipEventCreate(&e.ev0));
    KR_HIP(hipEventCreate(&e.ev1));
    KR_HIP(hipMemsetAsync(counters.p, 0, n_words * sizeof(unsigned long long), st));
    KR_HIP(hipEventRecord(e.ev0, st));
    rc = launch((unsigned long long*) counters.p);
    if (rc != KR_OK) return rc;
    KR_HIP(hipEventRecord(e.ev1, st));
    KR_HIP(hipMemcpyAsync(h_words, counters.p, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    KR_HIP(hipStreamSynchronize(st));
    if (stats) {
        float ms = 0;
        KR_HIP(hipEventElapsedTime(&ms, e.ev0, e.ev1));
        stats->kernel_ms = ms;
        stats->rays_traced = (int64_t) h_words[kTraced];
        stats->steps_total = (int64_t) h_words[kSteps];
        stats->longest_ray_steps = (int64_t) h_words[kLongest];
    }
    return KR_OK;
}

}  // namespace

}  // namespace kr
