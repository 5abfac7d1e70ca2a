// kr_trace.hip -- the hot path: Raytracer<T>::run_raytrace (reference raytracer.cpp:63-127, :972-1034)
// as a persistent gfx950 kernel.
//
// Mapping onto the hardware
//   * one ray per lane, all ray state in VGPRs, metric terms recomputed every evaluation; no LDS, no MFMA
//     (a latency-bound scalar fp64 ODE, SURVEY.md 8d: bound = fp64 VALU, ~0.5 B of HBM traffic per step);
//   * rays live in HBM as the reference's own 144-B (84-B) AoS records; a lane touches its record exactly
//     twice (load on entry, store on exit) -> 288 B per ray, irrelevant next to ~450 steps x ~1200 instructions;
//   * divergence: rays need 60 ... 100 000 steps.  Waves are persistent: a lane whose ray has ended writes it
//     back and, through one wave-aggregated atomicAdd on a global queue head (ballot + popcount), pulls the
//     next unprocessed ray, so a wave never idles on its slowest ray while work is left.  One loop iteration =
//     one integration step (RK45: one trial step) for every lane that holds a ray;
//   * the grid is sized to the device (CUs x resident waves), not to n;
//   * a launch cannot end before its longest ray does.  Large launches are therefore split in two concurrent ones
//     (split_front / split_back): the few ill-conditioned rays -- in the lamp-post workloads also the longest -- run the strict
//     arithmetic on waves that own their SIMDs (HOG instances), everything else fills the rest of the chip, with the
//     fast arithmetic (KR_FLAG_HYBRID) or the strict one (flags = 0; same bits as a single launch).
//
// Work-queue exit: every wave leaves the loop once the queue head has passed n AND none of its lanes holds a
// ray; every ray ends after at most steplim iterations (steps is incremented on every path through a step,
// and RK45 retries either shrink the step to MIN_STEP and force-accept, or end the ray on a NaN error norm).
// The loop itself (trace_body) lives in kr_trace_loop.hpp, where the recording kernel of kr_paths.hip takes it from too.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <limits>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "kr_common.hpp"
#include "kr_post_device.hpp"
#include "kr_trace_loop.hpp"

namespace kr {

namespace {

constexpr int kBlock = 256;          // classification kernel
// main launch, strict side launch (its general waves), strict overflow launch, split bookkeeping, the side launch's radial waves
enum CounterBlock { kMainBlock, kSideBlock, kOverflowBlock, kSplitBlock, kRadialBlock, kCounterBlocks };
constexpr int kListCap = 32768;      // entries of each of the side launch's two index lists (general, radial)

// ---- the persistent kernels ----------------------------------------------------------------------
// Their body is trace_body (kr_trace_loop.hpp), which explains METHOD, REFILL_MIN, `list`, `n_ptr`, `mask`, HOG and RADIAL.
// Resident waves per SIMD the register allocation must allow: HOG 1 (the scheduler may trade registers for ILP; capping it at (1, 1) measured 2 %
// slower), RK4 3 (<= 168 VGPRs), RK45 2, Euler 4 (its step is short and branchy: at 3 waves per SIMD the vector unit is 78 % busy; 1e7 rays
// 38.5 / 31.4 / 28.3 ms at 2 / 3 / 4 resident waves, profiles/r03_ab_experiments.txt).
// (Euler at 5: the fast kernel fits -- 96 registers, 32 B of spills -- and an all-fast 1e7-ray launch gains 2.5 %, but the hybrid pass and the
// returning-radiation batches, whose side launches share the chip with it, lose 1-3 %: profiles/r04_ab_experiments.txt.)
#define KR_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(HOG ? 1 : METHOD == KR_RK4 ? 3 : METHOD == KR_RK45 ? 2 : 4, 8)))
// everything one trace launch works on; a batch of traces hands the kernel an array of these (trace_multi_kernel)
template <typename T> struct TraceDesc {
    typename RayOf<T>::type* rays;
    long long n;
    TraceConsts<T> c;
    unsigned long long* counters;                 // this launch's counter block
    const int* list = nullptr;                    // ray indices, or null for 0 .. n
    const unsigned long long* n_ptr = nullptr;    // item count in device memory, or null (use n)
    const unsigned char* mask = nullptr;          // per-ray launch selector, or null
    int n_mode = 0, mask_want = 0;                // how n_ptr is applied (trace_body); the mask value this launch traces
};

// A wave that owns its SIMD has 512 vector registers to itself and the same ~100 scalar ones as any other wave: in the side launch's kernels the launch
// constants live in vector registers (the empty asm makes them opaque to the compiler's uniformity analysis) instead of being spilled to lanes and
// read back in the step loop, where such a wave pays four cycles for every instruction of any kind.  Euler and RK45 side launches -2 ... -3 %; the RK4
// kernel's allocation comes out 1 % slower with it and stays as it was (profiles/r04_ab_experiments.txt).
template <typename T> KR_DEV void consts_into_vector_registers(TraceConsts<T>& c)
{
    if constexpr (sizeof(T) == 8) {
        auto hold = [](T& x) { asm("" : "+v"(x)); };
        hold(c.a); hold(c.horizon); hold(c.rlim); hold(c.precision); hold(c.theta_precision); hold(c.max_tstep); hold(c.tol);
        hold(c.inv_precision); hold(c.inv_theta_precision); hold(c.tstep_rlim_eff); hold(c.phistep_eff); hold(c.theta_lo); hold(c.theta_hi);
    }
}

template <typename T, int METHOD, bool USE_DEST, bool FAST, bool HOG, int REFILL_MIN>
__global__ void __attribute__((amdgpu_flat_work_group_size(kTraceBlock, kTraceBlock))) KR_WAVES_ATTR
trace_kernel(typename RayOf<T>::type* __restrict__ rays, long long n, TraceConsts<T> c, unsigned long long* __restrict__ counters,
             const int* __restrict__ list, const unsigned long long* __restrict__ n_ptr, int n_mode, const unsigned char* __restrict__ mask, int mask_want)
{
    if (HOG) asm volatile("; claim the whole register file" ::: "v255", "a255");
    int has_prio = 0;
    if constexpr (HOG) {
        if constexpr (METHOD != KR_RK4) consts_into_vector_registers(c);
        trace_body<T, METHOD, USE_DEST, FAST, HOG, REFILL_MIN>(rays, n, c, counters, list, n_ptr, n_mode, mask, mask_want, has_prio, (long long) blockIdx.x * 64,
                                                               (unsigned long long) gridDim.x * 64);
    } else {
        trace_body<T, METHOD, USE_DEST, FAST, HOG, REFILL_MIN>(rays, n, c, counters, list, n_ptr, n_mode, mask, mask_want, has_prio);
    }
}

// The strict side launch of an Euler / RK4 trace with a theta-limit stop: its first `radial_workgroups` single-wave workgroups work on the list of
// radial rays with the radial body (a wave is all-radial or not radial at all: no per-lane choice in the step), the others on the general list with
// the body of trace_kernel's HOG instance.  One launch, so that both kinds start side by side while the chip is empty; two queues, counter blocks
// and lists.  Either count is read from device memory (n_mode 1).
template <int METHOD, int REFILL_MIN>
__global__ void __attribute__((amdgpu_flat_work_group_size(kTraceBlock, kTraceBlock))) __attribute__((amdgpu_waves_per_eu(1, 8)))
trace_side_kernel(kr_ray_f64* __restrict__ rays, long long n_list, TraceConsts<double> c, unsigned long long* __restrict__ counters_general,
                  unsigned long long* __restrict__ counters_radial, const int* __restrict__ list_general, const int* __restrict__ list_radial,
                  const unsigned long long* __restrict__ n_general, const unsigned long long* __restrict__ n_radial, int radial_workgroups)
{
    asm volatile("; claim the whole register file" ::: "v255", "a255");
    int has_prio = 0;
    if constexpr (METHOD != KR_RK4) consts_into_vector_registers(c);
    const int b = (int) blockIdx.x, g = (int) gridDim.x;
    if (b < radial_workgroups) {
        trace_body<double, METHOD, false, false, true, REFILL_MIN, true>(rays, n_list, c, counters_radial, list_radial, n_radial, 1, nullptr, 0, has_prio, (long long) b * 64,
                                                                         (unsigned long long) radial_workgroups * 64);
    } else {
        trace_body<double, METHOD, false, false, true, REFILL_MIN>(rays, n_list, c, counters_general, list_general, n_general, 1, nullptr, 0, has_prio,
                                                                   (long long) (b - radial_workgroups) * 64, (unsigned long long) (g - radial_workgroups) * 64);
    }
}

// ONE grid over MANY traces (kr_trace_batch_async_f64 when all traces of the batch use the same kernel instances).  Every wave serves
// ONE trace -- wave_trace[workgroup index], or workgroup index mod n_desc when no table is given -- with the persistent loop above,
// and leaves when that trace's queue is exhausted and its own lanes have drained.  The table interleaves the traces in proportion to
// their ray counts and the grid is larger than what is resident, so that waves of later workgroups move in wherever earlier ones have
// left: traces balance at wave granularity, a trace's tail is covered by the other traces' work, and the whole batch is two or three
// launches on two streams whatever the number of traces (beyond ~16 streams per process side launches slow down,
// profiles/r02_hw_queues.txt).  (A first version let each wave walk through all traces in turn: every wave then paid the tail of one
// long ray PER TRACE, 2.9 s for the 18-point sweep instead of 0.6 s.)  Per-ray arithmetic is the single-trace kernel's: same bits.
template <typename T, int METHOD, bool USE_DEST, bool FAST, bool HOG, int REFILL_MIN>
__global__ void __attribute__((amdgpu_flat_work_group_size(kTraceBlock, kTraceBlock))) KR_WAVES_ATTR
trace_multi_kernel(const TraceDesc<T>* __restrict__ descs, int n_desc, const int* __restrict__ wave_trace)
{
    if (HOG) asm volatile("; claim the whole register file" ::: "v255", "a255");
    int has_prio = 0;
    const int ti = wave_trace ? wave_trace[blockIdx.x] : (int) (blockIdx.x % (unsigned) n_desc);
    const TraceDesc<T>* d = &descs[ti];                           // wave-uniform: scalar loads
    if constexpr (HOG) {
        // (HOG batches map workgroup -> trace by modulo: workgroup b is the (b / n_desc)-th of its trace's gridDim.x / n_desc workgroups)
        const long long g = (long long) (blockIdx.x / (unsigned) n_desc);
        if constexpr (METHOD != KR_RK4) {
            TraceConsts<T> c = d->c;
            consts_into_vector_registers(c);
            trace_body<T, METHOD, USE_DEST, FAST, HOG, REFILL_MIN>(d->rays, d->n, c, d->counters, d->list, d->n_ptr, d->n_mode, d->mask, d->mask_want, has_prio, g * 64,
                                                                   (unsigned long long) (gridDim.x / (unsigned) n_desc) * 64);
        } else {
            trace_body<T, METHOD, USE_DEST, FAST, HOG, REFILL_MIN>(d->rays, d->n, d->c, d->counters, d->list, d->n_ptr, d->n_mode, d->mask, d->mask_want, has_prio, g * 64,
                                                                   (unsigned long long) (gridDim.x / (unsigned) n_desc) * 64);
        }
    } else {
        // (the merged kernels read their launch constants through `d`: with the time cap's words held in vector registers as well, the fast theta-limit
        // instances' allocation re-reads constants from memory inside the step loop -- they carry the signs and the Horner coefficients only)
        trace_body<T, METHOD, USE_DEST, FAST, HOG, REFILL_MIN, false, NoRecorder, kStepSigns | kStepNearLead>(d->rays, d->n, d->c, d->counters, d->list, d->n_ptr, d->n_mode, d->mask, d->mask_want, has_prio);
    }
}

// ---- hybrid path: which rays must be integrated with the reference's exact arithmetic? ----------------------------
// A ray is ILL-CONDITIONED when its polar motion or its axial angular momentum is a cancellation residue:
//   thetadot^2 rho^4 = Q + (k a cos + h cos/sin)(k a cos - h cos/sin)  with |sum| <= 1e-9 (|Q| + |product|), or |h| < 1e-13
// (PointSource rays emitted at beta = -pi: sin(beta) = -1.2e-16; ImagePlane rays on x = 0 / y = 0; NaN rays).  The
// reference's outcome for such a ray is decided by the rounding of exactly its own operation sequence, so only the
// strict path reproduces it; every other ray is insensitive to a few ulp per operation (tests/parity.py) and may
// take the fast path.  In the lamp-post workloads the ill-conditioned rays are also the longest ones: most of the beta = -pi column is held at the
// source's theta_0 next to the polar axis (the sum above is exactly zero there: RADIAL rays, kr_device.hpp) and winds round it, its step set by the
// max_phistep cap -- phi advances by ~0.4-0.6 rad per step, to -12 389 rad on the longest ray -- which is why they get SIMDs of their own (HOG launch).
KR_DEV bool ill_conditioned(double k, double h, double Q, double theta, double a)
{
    double sn, cs;
    kr_sincos_f64(theta, sn, cs);
    const double kac = k * a * cs;
    const double hcs = h * cs / sn;
    const double prod = (kac + hcs) * (kac - hcs);
    const double sum = Q + prod;
    return !(__builtin_fabs(sum) > 1e-9 * (__builtin_fabs(Q) + __builtin_fabs(prod))) || !(__builtin_fabs(h) >= 1e-13);
}

// wave-aggregated append; ill-conditioned rays are rare (a column / a row of the source grid), so are the atomics.
// mask: 0 = main launch, 1 = listed (strict side launch), 2 = ill-conditioned but its list is full (strict overflow launch)
KR_DEV unsigned char classify_append(bool strict, long long i, int* __restrict__ list_strict, unsigned long long* __restrict__ n_strict, unsigned long long* __restrict__ overflowed)
{
    const unsigned long long m = __ballot(strict);
    unsigned char mine = 0;
    if (m != 0) {
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((long long) m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(n_strict, (unsigned long long) __popcll(m));
        base = __shfl(base, leader, 64);
        if (strict) {
            const unsigned long long slot = base + __popcll(m & ((1ull << lane) - 1));
            if (slot < (unsigned long long) kListCap) { list_strict[slot] = (int) i; mine = 1; }
            else { *overflowed = 1; mine = 2; }
        }
    }
    return mine;
}

__global__ void __launch_bounds__(kBlock)
classify_kernel(const kr_ray_f64* __restrict__ rays, long long n, double a, unsigned char* __restrict__ strict_mask, int* __restrict__ list_strict,
                unsigned long long* __restrict__ split_words, bool radial_lists, double theta_lo, double theta_hi)
{
    // one ray per work-item: the pass is a 4-field gather over 144-byte records, so it wants every load in flight at once
    const long long i = blockIdx.x * (long long) kBlock + threadIdx.x;
    if (i >= n) return;
    const kr_ray_f64* ray = &rays[i];
    bool strict = false, radial = false;
    if (ray->steps >= 0) strict = ill_conditioned(ray->k, ray->h, ray->Q, ray->theta, a);       // unused slots (steps == -1) are skipped by either launch
    // radial_lists (the trace's side launch has radial waves): the flagged rays whose polar numerator is exactly zero at the state they are stored
    // in -- a ray that has been traced part of its way included: the proof needs k, h, Q and theta only -- go to the second list.  The lane that
    // takes such a ray decides again (radial_claim): this choice only says which waves a ray rides on.
    if (strict && radial_lists) {
        double sn, cs;
        kr_sincos<true>(ray->theta, sn, cs);
        radial = ray_is_radial(ray->k, ray->h, ray->Q, ray->r, ray->theta, a, theta_lo, theta_hi, sn, cs, lean_recip(sn));
    }
    const unsigned char general = classify_append(strict && !radial, i, list_strict, split_words + kFlagged, split_words + kListsOverflowed);
    const unsigned char listed = classify_append(radial, i, list_strict + kListCap, split_words + kRadial, split_words + kListsOverflowed);
    strict_mask[i] = general | listed;
}

// ---- host side ---------------------------------------------------------------------------------------
// Everything one trace call needs besides the rays -- queue heads and counters, the strict list and mask, timing events, the
// second stream of a split launch -- lives in a Workspace taken from a per-device pool for the duration of the call
// (until the call's last kernel has finished, which the pool learns from an event, not from the host).  Two traces on two
// streams, or from two host threads, therefore never share mutable state: any number may be in flight on one device.
struct Workspace {
    int device = 0;
    int cus = 0;
    unsigned long long* counters = nullptr;      // device: kCounterBlocks x kCounters
    unsigned long long* h_counters = nullptr;    // pinned host copy, filled by an async copy at the end of the call
    int* list = nullptr;                         // device: 2 x kListCap ray indices (the general list, then the radial one)
    unsigned char* mask = nullptr;               // device: one byte per ray
    int64_t mask_capacity = 0;
    std::vector<void*> retired;                  // outgrown masks (workspace_mask_reserve)
    hipStream_t side_stream = nullptr;                   // the second stream of a split trace: belongs to the caller's stream (side_stream_for)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;             // the whole trace, caller's stream
    hipEvent_t ev_strict0 = nullptr, ev_strict1 = nullptr; // strict side (+ overflow) launch, caller's stream
    hipEvent_t ev_main0 = nullptr, ev_main1 = nullptr;     // main launch of a split, side stream
    hipEvent_t ev_classified = nullptr, done = nullptr;
    hipEvent_t ev_in = nullptr;                          // merged batch: the caller's stream of this trace has reached the batch call
    void* d_descs = nullptr;                             // merged batch (held by its first trace): 3 x kMaxBatch descriptors on the device ...
    void* h_descs = nullptr;                             // ... and their pinned staging copy
    bool leased = false;       // a caller holds it (between trace_async and trace_wait / trace_release)
    bool pending = false;      // `done` has been recorded and not yet seen complete
    bool split = false;        // the last call used the split path (ev_strict*/ev_main* are valid)
    int64_t n = 0;
};

unsigned long long* block(const Workspace* ws, CounterBlock which) { return ws->counters + which * kCounters; }
const unsigned long long* host_block(const Workspace* ws, CounterBlock which) { return ws->h_counters + which * kCounters; }
constexpr size_t kCounterBytes = kCounterBlocks * kCounters * sizeof(unsigned long long);

constexpr size_t kMaxPool = 512;
constexpr int kMaxBatch = 256;                           // traces one merged batch can hold
constexpr int kMaxMultiGrid = 32768;                     // single-wave workgroups of a merged main launch (wave -> trace table entries)

// The second stream of a split trace is a property of the CALLER's stream, not of the call: traces issued on one stream run one after
// the other anyway, so they can share it, and a driver with 8 streams and 30 tickets outstanding then holds 16 streams, not 38 --
// beyond ~16 streams in a process the strict side launches slow down (profiles/r02_hw_queues.txt).
// It must not share a hardware queue with the caller's stream, or the two launches of a split serialise (seen once a process also
// holds RCCL's streams: HIP multiplexes streams onto a few queues per priority level).  A different priority level has queues of
// its own; the main launch it carries is also the one that may wait.
// One table per device: every caller stream that has run a split trace has an entry; at most kMaxSideStreams DISTINCT side streams exist per
// device -- a process that keeps making streams shares them (chosen by a hash of the caller's stream), each sharer with an entry of its own, so that
// a side stream is counted by everyone who may launch on it.  kr_stream_destroy / side_stream_forget drops the caller's entry and destroys the side
// stream when its last user has gone; kr_shutdown destroys the rest.
constexpr size_t kMaxSideStreams = 16;

// What the library keeps per device.  g_mu guards the pools, the workspaces' leased / pending flags and the side-stream tables; polling has a mutex
// of its own, so that a poll never waits behind a workspace acquisition that is blocked in hipEventSynchronize.
constexpr int kMaxDevices = 64;
struct DeviceState {
    std::vector<Workspace*> pool;                        // g_mu
    std::map<hipStream_t, hipStream_t> side_streams;     // g_mu: caller's stream -> side stream
    std::map<hipStream_t, int> side_users;               // g_mu: side stream -> number of entries above that point at it
    std::atomic<int> cus{0};                             // compute units, asked once (device_cus)
    hipStream_t poll_stream = nullptr;                   // g_poll_mu (trace_poll)
    unsigned long long* poll_word = nullptr;             // g_poll_mu: pinned, 8 bytes
};
std::mutex g_mu, g_poll_mu;
DeviceState g_devices[kMaxDevices];

DeviceState* device_state(int dev)
{
    if (dev < 0 || dev >= kMaxDevices) { set_error("device ordinal out of range"); return nullptr; }
    return &g_devices[dev];
}

int side_stream_for(int dev, hipStream_t user, hipStream_t* out)
{
    DeviceState* ds = device_state(dev);
    if (!ds) return KR_EINVAL;
    std::lock_guard<std::mutex> lk(g_mu);
    auto& table = ds->side_streams;
    auto& users = ds->side_users;
    auto it = table.find(user);
    if (it == table.end()) {
        hipStream_t s = nullptr;
        if (users.size() >= kMaxSideStreams) {             // share one of this device's
            auto pick = users.begin();
            std::advance(pick, (size_t) (((uintptr_t) user) >> 8) % users.size());
            s = pick->first;
        } else {
            int least = 0, greatest = 0;
            KR_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
            KR_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least));
        }
        ++users[s];
        it = table.emplace(user, s).first;
    }
    *out = it->second;
    return KR_OK;
}

void workspace_destroy(Workspace* w)
{
    if (!w) return;
    for (void* d : {(void*) w->counters, (void*) w->list, (void*) w->mask, w->d_descs}) if (d) (void) hipFree(d);
    for (void* h : {(void*) w->h_counters, w->h_descs}) if (h) (void) hipHostFree(h);
    for (void* old : w->retired) (void) hipFree(old);
    for (hipEvent_t e : {w->ev0, w->ev1, w->ev_strict0, w->ev_strict1, w->ev_main0, w->ev_main1, w->ev_classified, w->done, w->ev_in})
        if (e) (void) hipEventDestroy(e);
    delete w;
}

int workspace_create(int dev, Workspace** out)
{
    Workspace* w = new Workspace();
    w->device = dev;
    auto fail = [&](int rc) { workspace_destroy(w); return rc; };
#define KR_WS(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail(kr::hip_fail(e__, #call, __FILE__, __LINE__)); } while (0)
    KR_WS(hipMalloc((void**) &w->counters, kCounterBytes));
    KR_WS(hipHostMalloc((void**) &w->h_counters, kCounterBytes, hipHostMallocDefault));
    KR_WS(hipMalloc((void**) &w->list, 2 * kListCap * sizeof(int)));
    for (hipEvent_t* timed : {&w->ev0, &w->ev1, &w->ev_strict0, &w->ev_strict1, &w->ev_main0, &w->ev_main1}) KR_WS(hipEventCreate(timed));
    for (hipEvent_t* untimed : {&w->ev_classified, &w->done, &w->ev_in}) KR_WS(hipEventCreateWithFlags(untimed, hipEventDisableTiming));
#undef KR_WS
    const int rc = device_cus(dev, &w->cus);
    if (rc != KR_OK) return fail(rc);
    *out = w;
    return KR_OK;
}

// The per-ray launch selector of a split trace grows geometrically and never frees in the launch path: hipFree synchronises the whole
// device, i.e. every trace in flight on every stream would stall whenever a pooled workspace met a larger n (the returning-radiation
// radii differ in ray count).  The outgrown buffer is parked on the workspace and released by kr_shutdown; the parked
// bytes of a workspace sum to less than its current capacity.
int workspace_mask_reserve(Workspace* ws, int64_t n)
{
    if (ws->mask_capacity >= n) return KR_OK;
    const int64_t want = std::max<int64_t>(n, ws->mask_capacity + ws->mask_capacity / 2);
    unsigned char* grown = nullptr;
    KR_HIP(hipMalloc((void**) &grown, (size_t) want));
    if (ws->mask) ws->retired.push_back(ws->mask);
    ws->mask = grown;
    ws->mask_capacity = want;
    return KR_OK;
}

// takes an idle workspace of the current device out of the pool (or makes one); the caller owns it until workspace_release
int workspace_acquire(Workspace** out)
{
    int dev = 0;
    KR_HIP(hipGetDevice(&dev));
    DeviceState* ds = device_state(dev);
    if (!ds) return KR_EINVAL;
    Workspace* wait_for = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (Workspace* w : ds->pool) {
            if (w->leased) continue;
            if (w->pending) {
                if (hipEventQuery(w->done) != hipSuccess) { (void) hipGetLastError(); if (!wait_for) wait_for = w; continue; }
                w->pending = false;
            }
            w->leased = true;
            *out = w;
            return KR_OK;
        }
        if (ds->pool.size() < kMaxPool) {
            Workspace* w = nullptr;
            const int rc = workspace_create(dev, &w);
            if (rc != KR_OK) return rc;
            w->leased = true;
            ds->pool.push_back(w);
            *out = w;
            return KR_OK;
        }
        if (!wait_for) { set_error("kr_trace: too many trace tickets outstanding on this device (kr_trace_wait releases them)"); return KR_EINVAL; }
        wait_for->leased = true;          // ours from here on; its last call is still running
    }
    KR_HIP(hipEventSynchronize(wait_for->done));
    wait_for->pending = false;
    *out = wait_for;
    return KR_OK;
}

void workspace_release(Workspace* w)
{
    std::lock_guard<std::mutex> lk(g_mu);
    w->leased = false;
}

constexpr int64_t kIsolateMinRays = 1 << 18;      // below this a strict launch is too short for the split to pay

// (integrator, dest) -> the METHOD and USE_DEST template arguments, handed to `f` as two integral constants: the one place that knows
// which of them exist (Euler has no stop surfaces: validate).  FAST and HOG stay compile-time at the call sites, so that only the
// combinations in use are instantiated.
template <typename F>
int with_instance(int integrator, bool dest, F&& f)
{
    using std::integral_constant;
    switch (integrator) {
        case KR_EULER: return f(integral_constant<int, KR_EULER>(), std::false_type());
        case KR_RK4: return dest ? f(integral_constant<int, KR_RK4>(), std::true_type()) : f(integral_constant<int, KR_RK4>(), std::false_type());
        default: return dest ? f(integral_constant<int, KR_RK45>(), std::true_type()) : f(integral_constant<int, KR_RK45>(), std::false_type());
    }
}

// how many workgroups a launch gets
struct GridPolicy {
    int max_blocks_per_cu = 0;                    // sized by occupancy, at most this many resident waves per SIMD (0: the table in launch)
    int exact = 0;                                // > 0: exactly this many workgroups
    static GridPolicy occupancy(int max_blocks_per_cu) { return GridPolicy{max_blocks_per_cu, 0}; }
    static GridPolicy exactly(int workgroups) { return GridPolicy{0, workgroups}; }
};

template <typename T, int METHOD, bool USE_DEST, bool FAST, bool HOG = false>
int launch(const TraceDesc<T>& d, GridPolicy policy, int cus, hipStream_t stream)
{
    auto kern = trace_kernel<T, METHOD, USE_DEST, FAST, HOG, KR_REFILL_MIN>;
    // occupancy of each instance is a property of the code object: asked once per process
    static std::atomic<int> occ{0};                 // (host threads may race here: both would store the same value)
    int blocks_per_cu = occ.load(std::memory_order_relaxed);
    if (blocks_per_cu == 0) {
        int v = 0;
        KR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kern, kTraceBlock, 0));
        blocks_per_cu = v < 1 ? 1 : v;
        occ.store(blocks_per_cu, std::memory_order_relaxed);
    }
    // Resident workgroups per CU (= waves per SIMD).  The launch ends with its longest ray, which advances one step
    // per turn of its wave: with w waves per SIMD that turn comes round ~w times slower, while throughput keeps
    // improving up to ~3 waves.  Measured on MI355X, RK4 f64 strict, kernel ms at 1 / 2 / 3 workgroups per CU:
    //   PointSource 1e7 rays (longest ray 39 280 steps)  211 / 165 / 183      PointSource 3e7 rays   - / 455 / 432
    //   ImagePlane 4097^2 rays (longest ~2 000 steps)     480 / 344 / 318      fast-math 1e7 rays   176 / 121 / 110
    // Default: 3 when the launch is long enough for throughput to dominate (n >= 2e7, or fast-math with n >= 5e6),
    // else 2.  kr_params.flags bits 8..11 (KR_FLAG_BLOCKS_PER_CU) or the KR_BLOCKS_PER_CU environment variable override.
    int want = policy.max_blocks_per_cu > 0 ? policy.max_blocks_per_cu : (METHOD == KR_EULER && FAST) ? 4 : ((d.n >= 20000000 || (FAST && d.n >= 5000000)) ? 3 : 2);
    if (const char* e = getenv("KR_BLOCKS_PER_CU")) {
        const int v = atoi(e);
        if (v >= 1) want = v;
    }
    want *= 4;                                  // `want` counts waves per SIMD; a workgroup is one wave, a CU has four SIMDs
    if (want < blocks_per_cu) blocks_per_cu = want;
    const int grid = policy.exact > 0 ? policy.exact : persistent_grid(cus, blocks_per_cu, d.n);
    if (!HOG && d.list) { set_error("kr_trace: only side launches work from a list"); return KR_EINVAL; }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kTraceBlock), 0, stream, d.rays, d.n, d.c, d.counters, d.list, d.n_ptr, d.n_mode, d.mask, d.mask_want);
    KR_HIP(hipGetLastError());
    return KR_OK;
}

// one trace launch of the requested flavour (double only): FAST over `d` on `stream`, or strict HOG over `d`
template <bool FAST, bool HOG>
int launch_f64(const kr_params* p, const TraceDesc<double>& d, GridPolicy policy, int cus, hipStream_t stream)
{
    return with_instance(p->integrator, p->stop_kind != KR_STOP_THETA, [&](auto method, auto dest) -> int {
        return launch<double, decltype(method)::value, decltype(dest)::value, FAST, HOG>(d, policy, cus, stream);
    });
}

// the same for a whole batch of traces in ONE launch (trace_multi_kernel): `grid` single-wave workgroups, wave -> trace by table or modulo
template <bool FAST, bool HOG>
int launch_multi_f64(int integrator, bool dest, const TraceDesc<double>* d_descs, int n_desc, const int* d_wave_trace, int grid, hipStream_t stream)
{
    return with_instance(integrator, dest, [&](auto method, auto use_dest) -> int {
        auto kern = trace_multi_kernel<double, decltype(method)::value, decltype(use_dest)::value, FAST, HOG, KR_REFILL_MIN>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kTraceBlock), 0, stream, d_descs, n_desc, d_wave_trace);
        KR_HIP(hipGetLastError());
        return KR_OK;
    });
}

// The split trace: classify -> strict HOG launch over the (listed) ill-conditioned rays, on the caller's stream, first, so that
// its workgroups are placed while the chip is still empty  ||  main launch over all other rays on the workspace's side
// stream, filling what is left (the other way round the main launch takes every SIMD's registers and the strict one waits).
// fast_main: the main launch uses the fast arithmetic (KR_FLAG_HYBRID); otherwise it is the strict kernel too, i.e. the
// results are those of one strict launch, bit for bit, and only the placement of the long rays differs.
// Nothing here waits for the device: how many rays were flagged stays in device memory (split bookkeeping block, kFlagged) and the
// launches read it there.  The side launch is sized for the worst case the list can hold (workgroups that find the queue
// empty leave at once); a source made mostly of ill-conditioned rays (all rays in one meridional plane, say) overflows the
// list, and the overflow -- mask value 2 -- is traced by a third, ordinary-occupancy strict launch that is a no-op otherwise
// (its workgroups read the count and leave).
struct SplitPlan {
    TraceDesc<double> side;           // n_mode 1: the first min(flagged, side.n) list entries; side.n = what the list can hold of this trace
    TraceDesc<double> radial;         // the same over the list of radial rays, if has_radial (else that list stays empty)
    TraceDesc<double> main;           // every ray whose mask byte is 0
    TraceDesc<double> overflow;       // n_mode 2: the rays with mask byte 2, if a list overflowed
    bool has_overflow = false;        // a list can overflow at all (n > kListCap): without it there is no third launch
    bool has_radial = false;          // the side launch has radial waves (trace_side_kernel): strict Euler / RK4 with a theta-limit stop, not in a merged batch
};

// the three launches of one split trace over the workspace's list, mask and counter blocks (the mask is grown here if need be)
int plan_split(const kr_params* p, kr_ray_f64* rays, int64_t n, int steplim, Workspace* ws, SplitPlan* plan, bool radial_waves)
{
    if (n > 0x7fffffff) { set_error("kr_trace: the split path indexes rays with 32 bits"); return KR_EINVAL; }
    const int rc = workspace_mask_reserve(ws, n);
    if (rc != KR_OK) return rc;
    const unsigned long long* flagged = block(ws, kSplitBlock) + kFlagged;     // (zeroed by begin_trace)
    const TraceDesc<double> all{rays, (long long) n, make_consts<double>(p, steplim), nullptr};
    plan->side = plan->main = plan->overflow = all;
    plan->side.n = (long long) std::min<int64_t>(n, kListCap);
    plan->side.counters = block(ws, kSideBlock);
    plan->side.list = ws->list;
    plan->side.n_ptr = flagged;
    plan->side.n_mode = 1;
    plan->radial = plan->side;
    plan->radial.counters = block(ws, kRadialBlock);
    plan->radial.list = ws->list + kListCap;
    plan->radial.n_ptr = block(ws, kSplitBlock) + kRadial;
    // KR_NO_RADIAL=1 keeps every flagged ray on the general waves (A/B and bit-identity tests)
    plan->has_radial = radial_waves && p->integrator != KR_RK45 && p->stop_kind == KR_STOP_THETA && !getenv("KR_NO_RADIAL");
    plan->main.counters = block(ws, kMainBlock);
    plan->main.mask = ws->mask;
    plan->main.mask_want = 0;
    plan->overflow.counters = block(ws, kOverflowBlock);
    plan->overflow.n_ptr = block(ws, kSplitBlock) + kListsOverflowed;
    plan->overflow.n_mode = 2;
    plan->overflow.mask = ws->mask;
    plan->overflow.mask_want = 2;
    plan->has_overflow = n > kListCap;
    return KR_OK;
}

// fills the workspace's mask, list and flagged count for the rays of `plan`
int enqueue_classify(const SplitPlan& plan, Workspace* ws, hipStream_t stream)
{
    const long long n = plan.main.n;
    const int cgrid = (int) ((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(classify_kernel, dim3(cgrid), dim3(kBlock), 0, stream, plan.main.rays, n, plan.main.c.a, ws->mask, ws->list, block(ws, kSplitBlock), plan.has_radial,
                       plan.main.c.theta_lo, plan.main.c.theta_hi);
    KR_HIP(hipGetLastError());
    return KR_OK;
}

int validate(const kr_params* p, void* d_rays, int64_t n)
{
    if (!p || n < 0 || (n > 0 && !d_rays)) { set_error("kr_trace: null argument or negative n"); return KR_EINVAL; }
    const int rc = validate_run(p, "kr_trace");
    return rc != KR_OK ? rc : require_device();
}

// the two ends of every trace on its (primary) stream: counters zeroed and the clock started; the clock stopped, the counters
// copied out and `done` recorded
int begin_trace(Workspace* ws, hipStream_t stream)
{
    KR_HIP(hipMemsetAsync(ws->counters, 0, kCounterBytes, stream));
    KR_HIP(hipEventRecord(ws->ev0, stream));
    return KR_OK;
}

int end_trace(Workspace* ws, hipStream_t stream)
{
    KR_HIP(hipEventRecord(ws->ev1, stream));
    KR_HIP(hipMemcpyAsync(ws->h_counters, ws->counters, kCounterBytes, hipMemcpyDeviceToHost, stream));
    KR_HIP(hipEventRecord(ws->done, stream));
    return KR_OK;
}

// One trace is enqueued in two halves, so that a batch of traces can put ALL its front halves on the device before any back half:
//   front: counters zeroed, [classification + strict side launch] -- a handful of waves that want SIMDs of their own and carry the
//          launch's longest rays;        back: the main launch (and the overflow launch), counters copied out, `done` recorded.
// A lone kr_trace_async runs both at once.  In a batch (kr_trace_batch_async: one launch per tolerance, per source radius, ...)
// every side launch is placed while the chip is still empty; enqueued trace by trace, the main launch of trace k would own every
// SIMD's registers by the time the side launch of trace k+1 asks for them (measured: 18 RK45 sweep points in 1.6 s instead of 0.6 s).
struct Pending {
    const kr_params* p = nullptr;
    void* d_rays = nullptr;
    int64_t n = 0;
    hipStream_t stream = nullptr;
    bool f32 = false, hybrid = false, split = false;
    int steplim = 0;
    Workspace* ws = nullptr;
    SplitPlan plan;                   // split traces: made by the front half (launch constants included), used by both
};

int split_front(Pending& t)
{
    Workspace* ws = t.ws;
    int rc = plan_split(t.p, (kr_ray_f64*) t.d_rays, t.n, t.steplim, ws, &t.plan, true);
    if (rc != KR_OK) return rc;
    rc = enqueue_classify(t.plan, ws, t.stream);
    if (rc != KR_OK) return rc;
    KR_HIP(hipEventRecord(ws->ev_classified, t.stream));
    KR_HIP(hipEventRecord(ws->ev_strict0, t.stream));
    // strict side launch: one wave, alone on its SIMD, per 64 listed rays, on at most half of the chip
    const int grid = (int) std::max<int64_t>(1, std::min<int64_t>((t.plan.side.n + kTraceBlock - 1) / kTraceBlock, (int64_t) (ws->cus / 2) * 4));
    if (t.plan.has_radial) {
        // ... of either kind: the radial waves first (theirs are the longest rays), each kind on at most a quarter of the chip
        const int each = std::max(1, std::min(grid, (ws->cus / 4) * 4));
        const TraceDesc<double>& g = t.plan.side, & q = t.plan.radial;
        auto side = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(2 * each), dim3(kTraceBlock), 0, t.stream, g.rays, g.n, g.c, g.counters, q.counters, g.list, q.list, g.n_ptr, q.n_ptr, each);
        };
        if (t.p->integrator == KR_EULER) side(trace_side_kernel<KR_EULER, KR_REFILL_MIN>);
        else side(trace_side_kernel<KR_RK4, KR_REFILL_MIN>);
        KR_HIP(hipGetLastError());
    } else {
        rc = launch_f64<false, true>(t.p, t.plan.side, GridPolicy::exactly(grid), ws->cus, t.stream);
        if (rc != KR_OK) return rc;
    }
    KR_HIP(hipEventRecord(ws->ev_strict1, t.stream));
    ws->split = true;
    return KR_OK;
}

int split_back(Pending& t)
{
    Workspace* ws = t.ws;
    const int mb = KR_FLAG_GET_BLOCKS_PER_CU(t.p->flags);
    // main launch
    KR_HIP(hipStreamWaitEvent(ws->side_stream, ws->ev_classified, 0));
    KR_HIP(hipEventRecord(ws->ev_main0, ws->side_stream));
    const GridPolicy main_waves = GridPolicy::occupancy(mb ? mb : (t.hybrid && t.p->integrator == KR_EULER) ? 4 : 3);      // resident waves per SIMD of the main launch
    int rc = t.hybrid ? launch_f64<true, false>(t.p, t.plan.main, main_waves, ws->cus, ws->side_stream)
                      : launch_f64<false, false>(t.p, t.plan.main, main_waves, ws->cus, ws->side_stream);
    if (rc != KR_OK) return rc;
    // strict overflow launch (mask == 2): only has work when more than kListCap rays were flagged, and then the main launch has
    // next to none.  It follows the main launch on the side stream: behind the side launch on the caller's stream its idle
    // workgroups would sit waiting for the main launch's registers (measured: 10 ms of "kernel time" doing nothing).
    if (t.plan.has_overflow) {
        rc = launch_f64<false, false>(t.p, t.plan.overflow, GridPolicy::occupancy(mb), ws->cus, ws->side_stream);
        if (rc != KR_OK) return rc;
    }
    KR_HIP(hipEventRecord(ws->ev_main1, ws->side_stream));
    KR_HIP(hipStreamWaitEvent(t.stream, ws->ev_main1, 0));
    return KR_OK;
}

// the unsplit trace: one launch over all rays, strict or (double only) fast
template <typename T>
int dispatch(const Pending& t)
{
    const TraceDesc<T> d{(typename RayOf<T>::type*) t.d_rays, (long long) t.n, make_consts<T>(t.p, t.steplim), block(t.ws, kMainBlock)};
    const GridPolicy policy = GridPolicy::occupancy(KR_FLAG_GET_BLOCKS_PER_CU(t.p->flags));
    return with_instance(t.p->integrator, t.p->stop_kind != KR_STOP_THETA, [&](auto method, auto dest) -> int {
        if constexpr (std::is_same<T, double>::value) {
            if (t.p->flags & KR_FLAG_FAST_MATH) return launch<T, decltype(method)::value, decltype(dest)::value, true>(d, policy, t.ws->cus, t.stream);
        }
        return launch<T, decltype(method)::value, decltype(dest)::value, false>(d, policy, t.ws->cus, t.stream);
    });
}

int trace_front(Pending& t, bool batch)
{
    int rc = validate(t.p, t.d_rays, t.n);
    if (rc != KR_OK) return rc;
    if (t.n == 0) return KR_OK;
    t.steplim = effective_steplim(t.p);
    rc = workspace_acquire(&t.ws);
    if (rc != KR_OK) return rc;
    Workspace* ws = t.ws;
    ws->split = false;
    ws->n = t.n;
    t.hybrid = !t.f32 && (t.p->flags & KR_FLAG_HYBRID) && !(t.p->flags & KR_FLAG_FAST_MATH);
    // all-strict launches of some size isolate their ill-conditioned (in the lamp-post workloads: longest) rays the same way:
    // identical results, no tail; in a batch every strict launch does, whatever its size (its tail is what the batch overlaps).
    // KR_NO_ISOLATE=1 keeps the single launch (A/B and bit-identity tests).
    const bool isolate = !t.f32 && !t.hybrid && !(t.p->flags & KR_FLAG_FAST_MATH) && (t.n >= kIsolateMinRays || (batch && t.n >= 4096)) && !getenv("KR_NO_ISOLATE");
    t.split = t.hybrid || isolate;
    rc = begin_trace(ws, t.stream);
    if (rc != KR_OK || !t.split) return rc;
    rc = side_stream_for(ws->device, t.stream, &ws->side_stream);
    if (rc != KR_OK) return rc;
    return split_front(t);
}

int trace_back(Pending& t)
{
    if (t.n == 0 || !t.ws) return KR_OK;
    const int rc = t.f32 ? dispatch<float>(t) : t.split ? split_back(t) : dispatch<double>(t);
    if (rc != KR_OK) return rc;
    return end_trace(t.ws, t.stream);
}

// After a failure part-way: whatever was enqueued must drain before the workspace is reused.  The kernels of a split trace sit on the
// caller's stream AND its side stream, those of a merged batch on the batch's primary stream whatever t.stream is -- an event on
// t.stream alone would not cover them -- so the (rare) error path simply waits for the device before it lets the workspace go.
void abandon(Pending& t)
{
    if (!t.ws) return;
    (void) hipDeviceSynchronize();
    (void) hipGetLastError();
    {
        std::lock_guard<std::mutex> lk(g_mu);
        t.ws->pending = false;
    }
    workspace_release(t.ws);
    t.ws = nullptr;
}

void hand_over(Pending& t, void** ticket)
{
    if (t.ws) {
        std::lock_guard<std::mutex> lk(g_mu);
        t.ws->pending = true;
    }
    *ticket = t.ws;
}

}  // namespace

// what a kr_params must satisfy whichever kernel integrates its rays (the trace, the recording trace of kr_paths.hip); `who` prefixes the message
int validate_run(const kr_params* p, const char* who)
{
    const char* what = nullptr;
    if (p->integrator < KR_EULER || p->integrator > KR_RK45) what = "unknown integrator";
    else if (p->stop_kind < KR_STOP_THETA || p->stop_kind > KR_STOP_THICKDISC) what = "unknown stop_kind";
    // assert(method != Integrator::Euler), raytracer.cpp:983
    else if (p->stop_kind != KR_STOP_THETA && p->integrator == KR_EULER) what = "Integrator::Euler does not support RayDestination stopping conditions";
    else if (p->stop_kind == KR_STOP_THICKDISC) {
        // stop_params = {r_in, r_out, slope, scale} (include/kr_trace.h); r_out <= 0: open
        const double* sp = p->stop_params;
        if (!std::isfinite(sp[0]) || !(sp[0] > 0)) what = "KR_STOP_THICKDISC: r_in (stop_params[0]) must be positive and finite";
        else if (!std::isfinite(sp[1])) what = "KR_STOP_THICKDISC: r_out (stop_params[1]) must be finite (<= 0: open)";
        else if (!std::isfinite(sp[2]) || sp[2] < 0) what = "KR_STOP_THICKDISC: slope (stop_params[2]) must be non-negative and finite";
        else if (!std::isfinite(sp[3]) || sp[3] < 0) what = "KR_STOP_THICKDISC: scale (stop_params[3]) must be non-negative and finite";
    }
    if (what) set_error(std::string(who) + ": " + what);
    return what ? KR_EINVAL : KR_OK;
}

// compute units of device `dev`, asked once per process (host threads may race here: both would store the same value)
int device_cus(int dev, int* cus)
{
    DeviceState* ds = device_state(dev);
    if (!ds) return KR_EINVAL;
    if (ds->cus.load(std::memory_order_relaxed) == 0) {
        hipDeviceProp_t prop;
        KR_HIP(hipGetDeviceProperties(&prop, dev));
        ds->cus.store(prop.multiProcessorCount, std::memory_order_relaxed);
    }
    *cus = ds->cus.load(std::memory_order_relaxed);
    return KR_OK;
}

// Enqueues one trace on `stream` and returns at once; *ticket (never null on success, unless n == 0) must go to trace_wait or
// trace_release.  Nothing in here synchronises with the device.
int trace_async(const kr_params* p, void* d_rays, int64_t n, hipStream_t stream, bool f32, void** ticket)
{
    *ticket = nullptr;
    Pending t;
    t.p = p; t.d_rays = d_rays; t.n = n; t.stream = stream; t.f32 = f32;
    int rc = trace_front(t, false);
    if (rc == KR_OK) rc = trace_back(t);
    if (rc != KR_OK) { abandon(t); return rc; }
    hand_over(t, ticket);
    return KR_OK;
}

// A batch whose traces all run the same kernel instances (same integrator, same kind of stop surface, same arithmetic mode) is
// MERGED: one classification per trace, then ONE side launch, ONE main launch (and one overflow launch) over all of them
// (trace_multi_kernel), on the first trace's stream and its second stream; every other trace's stream waits for the batch at both ends.
int merged_batch(std::vector<Pending>& ts, bool hybrid)
{
    const int count = (int) ts.size();
    const kr_params* p0 = ts[0].p;
    const bool dest = p0->stop_kind != KR_STOP_THETA;
    hipStream_t primary = ts[0].stream;
    for (auto& t : ts) {
        t.steplim = effective_steplim(t.p);
        int rc = workspace_acquire(&t.ws);
        if (rc != KR_OK) return rc;
        t.ws->split = true;
        t.ws->n = t.n;
    }
    Workspace* w0 = ts[0].ws;
    hipStream_t side = nullptr;
    int rc = side_stream_for(w0->device, primary, &side);
    if (rc != KR_OK) return rc;
    const size_t table_off = 3 * kMaxBatch * sizeof(TraceDesc<double>);                   // [side descs | main descs | overflow descs | wave -> trace table of the main launch]
    const size_t staging_bytes = table_off + kMaxMultiGrid * sizeof(int);
    if (!w0->d_descs) {
        KR_HIP(hipMalloc(&w0->d_descs, staging_bytes));
        KR_HIP(hipHostMalloc(&w0->h_descs, staging_bytes, hipHostMallocDefault));
    }
    // inputs: whatever the callers enqueued on the traces' own streams (their ray sources) comes first
    for (auto& t : ts)
        if (t.stream != primary) {
            KR_HIP(hipEventRecord(t.ws->ev_in, t.stream));
            KR_HIP(hipStreamWaitEvent(primary, t.ws->ev_in, 0));
        }
    TraceDesc<double>* h = (TraceDesc<double>*) w0->h_descs;
    TraceDesc<double>* hog = h, * mainv = h + kMaxBatch, * rest = h + 2 * kMaxBatch;
    int n_rest = 0;
    int64_t hog_max = 1, main_waves = 0, n_total = 0;
    for (int i = 0; i < count; i++) {
        Pending& t = ts[i];
        Workspace* ws = t.ws;
        ws->side_stream = side;
        rc = plan_split(t.p, (kr_ray_f64*) t.d_rays, t.n, t.steplim, ws, &t.plan, false);      // (merged side launches have no radial waves)
        if (rc == KR_OK) rc = begin_trace(ws, primary);
        if (rc == KR_OK) rc = enqueue_classify(t.plan, ws, primary);
        if (rc != KR_OK) return rc;
        hog[i] = t.plan.side;
        mainv[i] = t.plan.main;
        if (t.plan.has_overflow) rest[n_rest++] = t.plan.overflow;
        hog_max = std::max<int64_t>(hog_max, (t.plan.side.n + kTraceBlock - 1) / kTraceBlock);
        main_waves += (t.n + kTraceBlock - 1) / kTraceBlock;
        n_total += t.n;
    }
    // main launch: twice what is resident (3 waves per SIMD), never more waves than 64-ray loads; wave -> trace in proportion to the
    // traces' ray counts, interleaved so that the first waves to be placed cover every trace
    const int mb = KR_FLAG_GET_BLOCKS_PER_CU(p0->flags);
    const int64_t resident = (int64_t) w0->cus * 4 * (mb ? mb : (hybrid && p0->integrator == KR_EULER) ? 4 : 3);
    const int main_grid = (int) std::max<int64_t>(count, std::min<int64_t>({main_waves, 2 * resident, (int64_t) kMaxMultiGrid}));
    int* wave_trace = (int*) ((char*) w0->h_descs + table_off);
    {
        std::vector<std::pair<double, int>> order;
        order.reserve((size_t) main_grid + (size_t) count);
        for (int i = 0; i < count; i++) {
            const int64_t q = std::max<int64_t>(1, (int64_t) ((double) (main_grid - count) * (double) ts[i].n / (double) n_total) + 1);
            for (int64_t k = 0; k < q; k++) order.emplace_back(((double) k + 0.5) / (double) q + 1e-9 * i, i);
        }
        std::sort(order.begin(), order.end());
        for (int b = 0; b < main_grid; b++) wave_trace[b] = order[(size_t) b % order.size()].second;     // (quotas sum to main_grid up to rounding)
    }
    KR_HIP(hipMemcpyAsync(w0->d_descs, w0->h_descs, staging_bytes, hipMemcpyHostToDevice, primary));
    const TraceDesc<double>* d = (const TraceDesc<double>*) w0->d_descs;
    const int* d_wave_trace = (const int*) ((const char*) w0->d_descs + table_off);
    KR_HIP(hipEventRecord(w0->ev_classified, primary));
    for (auto& t : ts) KR_HIP(hipEventRecord(t.ws->ev_strict0, primary));
    // side launch (wave -> trace by modulo): as many waves per trace as its list could need, but no more than fit on the chip at once
    // in total (1024 SIMDs; at least 4 per trace) -- a wave refills from its trace's list, so fewer waves only mean more rays per wave,
    // whereas thousands of exclusive single-wave workgroups that find nothing to do still have to be placed one by one
    const int64_t hog_per_trace = std::max<int64_t>(4, std::min<int64_t>(hog_max, (4 * (int64_t) w0->cus) / count));            // waves
    rc = launch_multi_f64<false, true>(p0->integrator, dest, d, count, nullptr, (int) (hog_per_trace * count), primary);
    if (rc != KR_OK) return rc;
    for (auto& t : ts) KR_HIP(hipEventRecord(t.ws->ev_strict1, primary));
    KR_HIP(hipStreamWaitEvent(side, w0->ev_classified, 0));
    for (auto& t : ts) KR_HIP(hipEventRecord(t.ws->ev_main0, side));
    rc = hybrid ? launch_multi_f64<true, false>(p0->integrator, dest, d + kMaxBatch, count, d_wave_trace, main_grid, side)
                : launch_multi_f64<false, false>(p0->integrator, dest, d + kMaxBatch, count, d_wave_trace, main_grid, side);
    if (rc != KR_OK) return rc;
    if (n_rest > 0) {
        // overflow launch: a no-op unless some trace flagged more rays than its list holds (then: few persistent waves per such trace)
        rc = launch_multi_f64<false, false>(p0->integrator, dest, d + 2 * kMaxBatch, n_rest, nullptr, (int) std::min<int64_t>((int64_t) n_rest * 64, resident), side);
        if (rc != KR_OK) return rc;
    }
    for (auto& t : ts) KR_HIP(hipEventRecord(t.ws->ev_main1, side));
    KR_HIP(hipStreamWaitEvent(primary, ts.back().ws->ev_main1, 0));      // the last one recorded: every ev_main1 has completed by then
    for (auto& t : ts) {
        rc = end_trace(t.ws, primary);
        if (rc != KR_OK) return rc;
        if (t.stream != primary) KR_HIP(hipStreamWaitEvent(t.stream, t.ws->done, 0));       // the caller's next kernels on that stream see the traced rays
    }
    return KR_OK;
}

// The same for `count` traces at once (double precision).  On failure nothing is left outstanding.
int trace_batch_async(int count, const kr_params* const* p, void* const* d_rays, const int64_t* n, void* const* streams, void** tickets)
{
    if (count < 0 || (count > 0 && (!p || !d_rays || !n || !tickets))) { set_error("kr_trace_batch_async: null argument"); return KR_EINVAL; }
    std::vector<Pending> ts((size_t) count);
    for (int i = 0; i < count; i++) {
        tickets[i] = nullptr;
        ts[i].p = p[i]; ts[i].d_rays = d_rays[i]; ts[i].n = n[i]; ts[i].stream = streams ? (hipStream_t) streams[i] : nullptr;
    }
    int rc = KR_OK;
    // mergeable: every trace valid, non-empty, split-capable, and on the same kernel instances
    bool merge = count >= 2 && count <= kMaxBatch && !getenv("KR_NO_MERGED_BATCH") && !getenv("KR_NO_ISOLATE");
    for (int i = 0; i < count && merge; i++) {
        if (validate(p[i], d_rays[i], n[i]) != KR_OK || n[i] < 4096 || (p[i]->flags & KR_FLAG_FAST_MATH)) merge = false;
        else if (p[i]->integrator != p[0]->integrator || (p[i]->stop_kind != KR_STOP_THETA) != (p[0]->stop_kind != KR_STOP_THETA) ||
                 (p[i]->flags & KR_FLAG_HYBRID) != (p[0]->flags & KR_FLAG_HYBRID) || KR_FLAG_GET_BLOCKS_PER_CU(p[i]->flags) != KR_FLAG_GET_BLOCKS_PER_CU(p[0]->flags))
            merge = false;
    }
    if (merge) {
        rc = merged_batch(ts, (p[0]->flags & KR_FLAG_HYBRID) != 0);
    } else {
        for (int i = 0; i < count && rc == KR_OK; i++) rc = trace_front(ts[i], true);
        for (int i = 0; i < count && rc == KR_OK; i++) rc = trace_back(ts[i]);
    }
    if (rc != KR_OK) {
        for (auto& t : ts) abandon(t);
        return rc;
    }
    for (int i = 0; i < count; i++) hand_over(ts[i], &tickets[i]);
    return KR_OK;
}

// Waits for the trace behind `ticket`, fills *stats (may be null) and returns the workspace to the pool.
int trace_wait(void* ticket, kr_stats* stats)
{
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!ticket) return KR_OK;                       // the n == 0 call
    Workspace* ws = (Workspace*) ticket;
    auto body = [&]() -> int {
        KR_HIP(hipEventSynchronize(ws->done));
        if (!stats) return KR_OK;
        const unsigned long long* mainb = host_block(ws, kMainBlock), * over = host_block(ws, kOverflowBlock);
        unsigned long long side[kCounterWords];             // the side launch: its general and its radial waves
        for (int i = 0; i < kCounterWords; i++) side[i] = host_block(ws, kSideBlock)[i] + host_block(ws, kRadialBlock)[i];
        side[kLongest] = std::max(host_block(ws, kSideBlock)[kLongest], host_block(ws, kRadialBlock)[kLongest]);
        unsigned long long h[kCounterWords];
        for (int i = 0; i < kCounterWords; i++) h[i] = mainb[i] + side[i] + over[i];
        h[kLongest] = std::max(mainb[kLongest], std::max(side[kLongest], over[kLongest]));      // a maximum, not a sum
#if KR_OCC_STATS
        for (CounterBlock b : {kMainBlock, kSideBlock, kOverflowBlock, kRadialBlock}) {
            const unsigned long long* q = host_block(ws, b);
            if (q[8]) std::fprintf(stderr, "kr_occ: launch %d (0 main, 1 strict side, 2 overflow, 4 radial side): steps %llu wave_iters %llu step-loop lane occupancy %.4f | after queue exhaustion: "
                                   "wave_iters %llu (%.2f %%) lane occupancy %.4f | refills %llu lanes/refill %.2f | longest ray %llu steps\n", (int) b, q[kSteps], q[8], (double) q[kSteps] / (64.0 * q[8]), q[9],
                                   100.0 * q[9] / q[8], q[9] ? (double) q[10] / (64.0 * q[9]) : 0.0, q[11], q[11] ? (double) q[12] / q[11] : 0.0, q[kLongest]);
        }
#endif
#if KR_GUARD_STATS
        {
            const unsigned long long* q = host_block(ws, kMainBlock) + kGuardStatWord;
            if (q[2]) std::fprintf(stderr, "kr_guards: main launch wave-steps %llu | quiet: at %llu all %llu | turn: at %llu all %llu | cap: at %llu all %llu | sine band: at %llu all-0 %llu all-1 %llu\n",
                                   q[2], q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
        }
#endif
        stats->rays_total = ws->n;
        stats->rays_strict_side = (int64_t) (host_block(ws, kSplitBlock)[kFlagged] + host_block(ws, kSplitBlock)[kRadial]);
        stats->rays_traced = (int64_t) h[kTraced];
        stats->steps_total = (int64_t) h[kSteps];
        stats->rk45_attempts = (int64_t) h[kAttempts];
        stats->rk45_rejects = (int64_t) h[kRejects];
        stats->rk45_stationary_steps = (int64_t) h[kStationary];
        stats->rk45_extrapolated_steps = (int64_t) h[kExtrapolated];
        stats->longest_ray_steps = (int64_t) h[kLongest];
        stats->longest_ray_steps_strict_side = ws->split ? (int64_t) side[kLongest] : 0;
        stats->steps_strict_side = ws->split ? (int64_t) side[kSteps] : 0;
        stats->rk45_evaluated_strict_side = ws->split ? (int64_t) (side[kAttempts] - side[kStationary] - side[kExtrapolated]) : 0;
        float ms = 0;
        KR_HIP(hipEventElapsedTime(&ms, ws->ev0, ws->ev1));
        stats->kernel_ms = ms;
        if (ws->split) {
            KR_HIP(hipEventElapsedTime(&ms, ws->ev_strict0, ws->ev_strict1));
            stats->strict_side_ms = ms;
            KR_HIP(hipEventElapsedTime(&ms, ws->ev_main0, ws->ev_main1));
            stats->main_ms = ms;
        }
        return KR_OK;
    };
    const int rc = body();
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (rc == KR_OK) ws->pending = false;
        ws->leased = false;
    }
    return rc;
}

// How far the trace behind `ticket` has come: the number of rays its waves have taken off the work queue so far (what the reference's progress
// counter counts, raytracer.cpp:107-112: a ray is counted when its loop iteration STARTS), and whether the trace has finished.  The queue head lives
// in device memory; it is read with an 8-byte copy on a stream of the library's own (a DMA transfer: it needs no compute unit, so it completes while
// the persistent kernels hold every SIMD), a few microseconds per call.  Does not wait for the trace and does not retire the ticket.
int trace_poll(void* ticket, int64_t* rays_started, int32_t* finished)
{
    if (rays_started) *rays_started = 0;
    if (finished) *finished = 1;
    if (!ticket) return KR_OK;                       // the n == 0 call
    Workspace* ws = (Workspace*) ticket;
    const hipError_t q = hipEventQuery(ws->done);
    if (q == hipSuccess) {
        if (rays_started) *rays_started = ws->n;
        return KR_OK;
    }
    (void) hipGetLastError();
    if (q != hipErrorNotReady) return kr::hip_fail(q, "hipEventQuery(trace)", __FILE__, __LINE__);
    if (finished) *finished = 0;
    int dev = 0;
    KR_HIP(hipGetDevice(&dev));
    if (dev != ws->device) { set_error("kr_trace_poll: the ticket belongs to another device than the current one"); return KR_EINVAL; }
    DeviceState* ds = device_state(dev);
    if (!ds) return KR_EINVAL;
    std::lock_guard<std::mutex> lk(g_poll_mu);
    if (!ds->poll_stream) {
        KR_HIP(hipStreamCreateWithFlags(&ds->poll_stream, hipStreamNonBlocking));
        KR_HIP(hipHostMalloc((void**) &ds->poll_word, sizeof(unsigned long long), hipHostMallocDefault));
    }
    // the main launch (or the only one): its head runs over all n slots, also those whose rays belong to the side launch
    KR_HIP(hipMemcpyAsync(ds->poll_word, block(ws, kMainBlock) + kHead, sizeof(unsigned long long), hipMemcpyDeviceToHost, ds->poll_stream));
    KR_HIP(hipStreamSynchronize(ds->poll_stream));
    if (rays_started) *rays_started = (int64_t) std::min<unsigned long long>(*ds->poll_word, (unsigned long long) ws->n);
    return KR_OK;
}

// Gives the ticket back without waiting: the workspace is reused once its trace has finished.
void trace_release(void* ticket)
{
    if (ticket) workspace_release((Workspace*) ticket);
}

// kr_stream_destroy: the side stream that belonged to `user` goes with it (its work has drained: the caller's stream waits for it at the
// end of every split trace, and is synchronised here before it is destroyed).
void side_stream_forget(hipStream_t user)
{
    // (the entry is looked for on every device: the device that is current when a stream is destroyed need not be the one it was used on)
    hipStream_t side = nullptr;
    int side_dev = -1;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (int dev = 0; dev < kMaxDevices && side_dev < 0; dev++) {
            DeviceState& ds = g_devices[dev];
            auto it = ds.side_streams.find(user);
            if (it == ds.side_streams.end()) continue;
            hipStream_t s = it->second;
            ds.side_streams.erase(it);
            auto u = ds.side_users.find(s);
            if (u != ds.side_users.end() && --u->second <= 0) {
                ds.side_users.erase(u);
                side = s;                                    // its last user: nobody can be handed it any more
                side_dev = dev;
            } else {
                return;                                      // other caller streams still launch on it
            }
        }
    }
    if (!side) return;
    CurrentDeviceGuard restore;
    if (hipSetDevice(side_dev) == hipSuccess) {
        (void) hipStreamSynchronize(side);
        (void) hipStreamDestroy(side);
    }
}

// kr_shutdown: waits for the devices this library has used, then gives back every pooled workspace and side stream.  Refused (KR_EINVAL, nothing
// released) while a trace ticket is outstanding: its kr_trace_wait / kr_trace_release would touch a freed workspace.
int trace_shutdown()
{
    CurrentDeviceGuard restore;
    std::lock_guard<std::mutex> lk(g_mu);
    for (const DeviceState& ds : g_devices)
        for (const Workspace* w : ds.pool)
            if (w->leased) {
                set_error("kr_shutdown: trace tickets are outstanding (kr_trace_wait / kr_trace_release them first)");
                return KR_EINVAL;
            }
    for (int dev = 0; dev < kMaxDevices; dev++) {
        DeviceState& ds = g_devices[dev];
        if (ds.pool.empty() && ds.side_users.empty() && !ds.poll_stream) continue;
        if (hipSetDevice(dev) != hipSuccess) { (void) hipGetLastError(); continue; }
        (void) hipDeviceSynchronize();
        for (Workspace* w : ds.pool) workspace_destroy(w);
        ds.pool.clear();
        {
            std::lock_guard<std::mutex> pl(g_poll_mu);
            if (ds.poll_stream) { (void) hipStreamDestroy(ds.poll_stream); ds.poll_stream = nullptr; }
            if (ds.poll_word) { (void) hipHostFree(ds.poll_word); ds.poll_word = nullptr; }
        }
        for (auto& kv : ds.side_users) (void) hipStreamDestroy(kv.first);
        ds.side_users.clear();
        ds.side_streams.clear();
    }
    return KR_OK;
}

int trace_dev(const kr_params* p, void* d_rays, int64_t n, hipStream_t stream, kr_stats* stats, bool f32)
{
    if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->rays_total = n; }
    void* ticket = nullptr;
    const int rc = trace_async(p, d_rays, n, stream, f32, &ticket);
    if (rc != KR_OK) return rc;
    if (!stats) { trace_release(ticket); return KR_OK; }
    const int rc2 = trace_wait(ticket, stats);
    stats->rays_total = n;
    return rc2;
}

}  // namespace kr
