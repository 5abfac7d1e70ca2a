// kr_paths.hip -- the per-step trajectory dump of Raytracer<T>::run_raytrace(..., outfile, write_step, write_rmax, write_rmin, write_cartesian)
// (reference raytracer.cpp:86-100; the write rule :293-312 Euler, :923-942 and :1209-1228 RK4) as two passes of a persistent gfx950 kernel.
//
// fp64, strict arithmetic, Euler and RK4 only.  A recorded ray is integrated by the very step function a flags = 0 trace uses
// (step_fixed<double, RK4, USE_DEST, false>, kr_device.hpp), so it takes the same steps and ends with the same record, bit for bit.
//
// Mapping onto the hardware: one ray per lane, persistent single-wave workgroups that refill their free lanes from a global queue through
// one wave-aggregated atomicAdd (ballot + popcount), as the trace does -- rays need 60 ... 40 000 steps, and a launch without refill would
// idle 63 of 64 lanes on its longest ray.
//
// Rows are stored compressed: ray i owns rows[offsets[i] .. offsets[i + 1]).  Two passes make that possible without a worst-case allocation:
//   count   integrates every ray and stores only how many rows it writes (and whether it was traced at all); rays[] is not modified;
//           an exclusive scan turns the counts into offsets[0 .. n], offsets[n] is the total;
//   record  integrates again -- the same arithmetic, hence the same rows -- and stores row k of ray i at rows[offsets[i] + k], then the
//           final ray record as a trace does.  It counts what it writes; a ray whose count differs from its slab is reported, and no row is
//           ever stored outside the ray's slab or the buffer.
// A row is {t, r, theta, phi}: four doubles, 32 aligned bytes, two 16-byte vector stores.  Boyer-Lindquist always: write_cartesian is applied by
// the host-side writers (host/include/kerr.h cartesian()), with the C library the reference calls.
//
// Why an iteration of step_fixed ended is read off the lane afterwards, so the step functions stay as the trace kernels compile them:
//   theta flip (`continue`, writes nothing)   theta_was_positive went from true to false: only the flip clears it (k1_with_flips);
//   horizon / destination (`break` before the write)   the status bit the iteration added (the lane's status is parked during the step).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kr_pass.hpp"
#include "kr_ray_io.hpp"

namespace kr {

namespace {

constexpr int kPathBlock = 64;        // one wave per workgroup: a wave gives its registers back when IT has finished (kr_trace.hip)
constexpr int kPathRefillMin = 4;     // a wave goes back to the queue when this many of its lanes are free (kr_trace.hip, KR_REFILL_MIN)
constexpr int kScanBlock = 1024;

// device words of one pass: queue head, rays traced, steps, longest ray, rays whose row count differs from their slab
enum PathWord { kPHead, kPTraced, kPSteps, kPLongest, kPMismatch, kPWords };

struct PathWindow {
    double rmin, rmax;        // write_rmin, write_rmax: < 0 switches that side off
    int32_t write_step;
};

// (write_rmax < 0 || r < write_rmax) && (write_rmin < 0 || r > write_rmin), raytracer.cpp:295
KR_DEV bool in_window(const PathWindow& w, double r)
{
    return (w.rmax < 0 || r < w.rmax) && (w.rmin < 0 || r > w.rmin);
}

KR_DEV unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

KR_DEV unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// RECORD = false: the count pass.  offsets[i] receives ray i's row count (the scan below turns the counts into offsets), traced[i] (optional)
// whether the ray passed the skip rule; rays[] is read only.
// RECORD = true: offsets[0 .. n] are the scanned offsets; rows and the final ray records are stored.
template <bool RK4, bool USE_DEST, bool RECORD>
__global__ void __attribute__((amdgpu_flat_work_group_size(kPathBlock, kPathBlock))) __attribute__((amdgpu_waves_per_eu(RK4 ? 3 : 4, 8)))
paths_kernel(kr_ray_f64* __restrict__ rays, long long n, TraceConsts<double> c, PathWindow w, long long* __restrict__ offsets, unsigned char* __restrict__ traced,
             double* __restrict__ rows, long long total_rows, unsigned long long* __restrict__ counters)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long lane_bit = 1ull << lane;

    Lane<double> s;
    long long idx = -1;
    long long slab = 0, cap = 0;      // RECORD: first row of this lane's ray and how many it may write
    int32_t n_rows = 0;               // rows this lane's ray has written so far (write_started == n_rows > 0)
    int32_t until_write = 0;          // iterations left until steps % write_step == 0
    bool have = false, pend = false, exhausted = false;
    unsigned long long my_steps = 0, my_traced = 0, my_mismatch = 0;
    int32_t my_longest = 0;

    for (;;) {
        const unsigned long long need = __builtin_amdgcn_ballot_w64(!have);
        const int n_need = __popcll(need);
        const bool any_have = (need != ~0ull);
        const bool visit = !exhausted && n_need > 0 && (n_need >= kPathRefillMin || !any_have);
        const bool leaving = !visit && !any_have;
        if (visit || leaving) {
            if (pend) {
                // the one place where a ray's results leave its lane
                my_steps += (unsigned long long) s.steps;
                my_longest = s.steps > my_longest ? s.steps : my_longest;
                if constexpr (RECORD) {
                    store_ray(&rays[idx], s, finish_status<double, USE_DEST>(s, c));
                    if ((long long) n_rows != cap) ++my_mismatch;
                } else {
                    offsets[idx] = (long long) n_rows;
                }
                pend = false;
            }
            if (leaving) break;
            // wave-aggregated dequeue: one atomic for all free lanes
            const int leader = __ffsll((long long) need) - 1;
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(&counters[kPHead], (unsigned long long) n_need);
            base = __shfl(base, leader, 64);
            if (base + (unsigned long long) n_need >= (unsigned long long) n) exhausted = true;
            if (!have) {
                const long long slot = (long long) base + __popcll(need & (lane_bit - 1));
                if (slot < n) {
                    load_ray(&rays[slot], s);
                    // skip rule of run_raytrace's serial path (raytracer.cpp:91-92): a skipped ray has no rows and no blank lines
                    const bool take = s.steps0 >= 0 && s.steps0 < c.steplim;
                    if constexpr (!RECORD) {
                        if (traced) traced[slot] = take ? 1 : 0;
                        if (!take) offsets[slot] = 0;
                    }
                    if (take) {
                        idx = slot;
                        have = true;
                        ++my_traced;
                        n_rows = 0;
                        until_write = w.write_step;
                        if constexpr (RECORD) {
                            slab = offsets[slot];
                            cap = offsets[slot + 1] - slab;
                        }
                        s.steps = 0;
                        s.r_was_positive = false;
                        s.theta_was_positive = true;
                        energy_guard_set(s);
                        if (!loop_cond<double, USE_DEST>(s, c)) {      // zero-iteration call: only the epilogue runs
                            have = false;
                            pend = true;
                        }
                    }
                }
            }
            continue;
        }

        if (have) {
            const bool flip_armed = s.theta_was_positive;
            const int32_t status_before = s.status;
            s.status = 0;
            bool fin = step_fixed<double, RK4, USE_DEST, false>(s, c);
            const int32_t added = s.status;
            s.status = status_before | added;
            const bool due = (--until_write == 0);            // steps % write_step == 0: every iteration increments steps once
            if (due) until_write = w.write_step;
            const bool flipped = flip_armed && !s.theta_was_positive;                               // `continue`
            const bool broke = (added & (KR_STATUS_HORIZON | (USE_DEST ? KR_STATUS_DEST : 0))) != 0;  // `break` before the write
            if (due && !flipped && !broke) {
                if (in_window(w, s.r)) {
                    if constexpr (RECORD) {
                        const long long at = slab + n_rows;
                        if ((long long) n_rows < cap && at >= 0 && at < total_rows) {
                            double2* q = reinterpret_cast<double2*>(rows + 4 * at);
                            q[0] = make_double2(s.t, s.r);
                            q[1] = make_double2(s.theta, s.phi);
                        }
                    }
                    ++n_rows;
                } else if (n_rows > 0) {
                    fin = true;           // `else if (write_started) break;`  (:308-311)
                }
            }
            if (fin) {
                have = false;
                pend = true;
            }
        }
    }
    const unsigned long long w_traced = wave_sum_u64(my_traced);
    const unsigned long long w_steps = wave_sum_u64(my_steps);
    const unsigned long long w_mismatch = wave_sum_u64(my_mismatch);
    const unsigned long long w_longest = wave_max_u64((unsigned long long) my_longest);
    if (lane == 0) {
        if (w_traced) atomicAdd(&counters[kPTraced], w_traced);
        if (w_steps) atomicAdd(&counters[kPSteps], w_steps);
        if (w_mismatch) atomicAdd(&counters[kPMismatch], w_mismatch);
        if (w_longest) atomicMax(&counters[kPLongest], w_longest);
    }
}

// In-place exclusive scan of v[0 .. n) with the total in v[n], by ONE workgroup: every work-item sums a contiguous piece, the 1024 piece sums are
// scanned in LDS, every work-item then rewrites its piece.  (A work-item walks its own piece, so a wave's loads are not coalesced; the scan is part
// of the count pass's time in profiles/ray_paths.txt, next to a pass that integrates every ray.)
__global__ void __launch_bounds__(kScanBlock) scan_counts_kernel(long long* __restrict__ v, long long n)
{
    __shared__ long long part[kScanBlock];
    const int t = threadIdx.x;
    const long long per = (n + kScanBlock - 1) / kScanBlock;
    const long long lo = (long long) t * per < n ? (long long) t * per : n;
    const long long hi = lo + per < n ? lo + per : n;
    long long sum = 0;
    for (long long i = lo; i < hi; i++) sum += v[i];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < kScanBlock; off <<= 1) {          // inclusive Hillis-Steele scan of the piece sums
        const long long add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    long long run = part[t] - sum;                            // exclusive prefix of this piece
    for (long long i = lo; i < hi; i++) {
        const long long count = v[i];
        v[i] = run;
        run += count;
    }
    if (t == kScanBlock - 1) v[n] = part[t];
}

template <bool RK4, bool USE_DEST, bool RECORD>
int launch_paths(kr_ray_f64* rays, long long n, const TraceConsts<double>& c, const PathWindow& w, long long* offsets, unsigned char* traced, double* rows,
                 long long total_rows, unsigned long long* counters, hipStream_t stream)
{
    auto kern = paths_kernel<RK4, USE_DEST, RECORD>;
    int dev = 0, per_cu = 0;
    KR_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    KR_HIP(hipGetDeviceProperties(&prop, dev));
    KR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kPathBlock, 0));
    // resident waves per SIMD as the strict trace sizes its launches (kr_trace.hip::launch): 2 for RK4 -- the pass ends with its longest ray,
    // which advances one step per turn of its wave -- 4 for the short Euler step
    per_cu = std::max(1, std::min(per_cu, 4 * (RK4 ? 2 : 4)));
    const long long resident = (long long) prop.multiProcessorCount * per_cu;
    const long long wanted = (n + kPathBlock - 1) / kPathBlock;
    const int grid = (int) std::max<long long>(1, std::min(resident, wanted));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kPathBlock), 0, stream, rays, n, c, w, offsets, traced, rows, total_rows, counters);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

template <bool RECORD>
int launch_paths_for(const kr_params* p, kr_ray_f64* rays, long long n, const PathWindow& w, long long* offsets, unsigned char* traced, double* rows,
                     long long total_rows, unsigned long long* counters, hipStream_t stream)
{
    const TraceConsts<double> c = make_consts<double>(p, effective_steplim(p));
    if (p->integrator == KR_EULER) return launch_paths<false, false, RECORD>(rays, n, c, w, offsets, traced, rows, total_rows, counters, stream);
    if (p->stop_kind == KR_STOP_THETA) return launch_paths<true, false, RECORD>(rays, n, c, w, offsets, traced, rows, total_rows, counters, stream);
    return launch_paths<true, true, RECORD>(rays, n, c, w, offsets, traced, rows, total_rows, counters, stream);
}

PathWindow window_of(const kr_path_spec* w) { return PathWindow{w->write_rmin, w->write_rmax, w->write_step}; }

int fail(const char* who, const char* what)
{
    set_error(std::string(who) + ": " + what);
    return KR_EINVAL;
}

}  // namespace

// everything that can be refused without a device (include/kr_trace.h lists it)
int paths_validate(const kr_params* p, const kr_path_spec* w, const char* who)
{
    if (!p || !w) return fail(who, "null argument");
    if (w->write_step <= 0) return fail(who, "write_step must be positive (the reference takes steps % write_step)");
    if (std::isnan(w->write_rmin) || std::isnan(w->write_rmax)) return fail(who, "write_rmin / write_rmax must not be NaN");
    if (p->flags & (KR_FLAG_FAST_MATH | KR_FLAG_HYBRID))
        return fail(who, "paths carry the reference's arithmetic: KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted");
    if (p->integrator == KR_RK45) return fail(who, "RK45 paths are not recorded (Euler and RK4 only)");
    if (p->integrator != KR_EULER && p->integrator != KR_RK4) return fail(who, "unknown integrator");
    if (p->stop_kind < KR_STOP_THETA || p->stop_kind > KR_STOP_FLATPLANE) return fail(who, "unknown stop_kind");
    // assert(method != Integrator::Euler), raytracer.cpp:983
    if (p->stop_kind != KR_STOP_THETA && p->integrator == KR_EULER) return fail(who, "Integrator::Euler does not support RayDestination stopping conditions");
    return KR_OK;
}

int paths_count_dev(const kr_params* p, const kr_path_spec* w, const void* d_rays, int64_t n, void* d_offsets, void* d_traced, int64_t* total_rows, hipStream_t st)
{
    DeviceBuffer counters;
    int rc = counters.alloc(kPWords * sizeof(unsigned long long));
    if (rc != KR_OK) return rc;
    KR_HIP(hipMemsetAsync(counters.p, 0, kPWords * sizeof(unsigned long long), st));
    if (n > 0) {
        // (the count pass only reads the records: the kernel's RECORD = false instance has no store to rays[])
        rc = launch_paths_for<false>(p, const_cast<kr_ray_f64*>((const kr_ray_f64*) d_rays), (long long) n, window_of(w), (long long*) d_offsets,
                                     (unsigned char*) d_traced, nullptr, 0, (unsigned long long*) counters.p, st);
        if (rc != KR_OK) return rc;
    }
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(kScanBlock), 0, st, (long long*) d_offsets, (long long) n);
    KR_LAUNCH_CHECK();
    long long total = 0;
    KR_HIP(hipMemcpyAsync(&total, (const long long*) d_offsets + n, sizeof total, hipMemcpyDeviceToHost, st));
    KR_HIP(hipStreamSynchronize(st));
    *total_rows = (int64_t) total;
    return KR_OK;
}

int paths_record_dev(const kr_params* p, const kr_path_spec* w, void* d_rays, int64_t n, const void* d_offsets, void* d_rows, int64_t total_rows, hipStream_t st,
                     kr_stats* stats)
{
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->rays_total = n; }
    long long need = 0;
    KR_HIP(hipMemcpyAsync(&need, (const long long*) d_offsets + n, sizeof need, hipMemcpyDeviceToHost, st));
    KR_HIP(hipStreamSynchronize(st));
    if (need < 0 || (long long) total_rows < need) return fail("kr_trace_paths_record", "total_rows is smaller than offsets[n]");
    if (n == 0) return KR_OK;
    DeviceBuffer counters;
    int rc = counters.alloc(kPWords * sizeof(unsigned long long));
    if (rc != KR_OK) return rc;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KR_HIP(hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) { (void) hipEventDestroy(ev0); return hip_fail(hipGetLastError(), "hipEventCreate", __FILE__, __LINE__); }
    auto body = [&]() -> int {
        KR_HIP(hipMemsetAsync(counters.p, 0, kPWords * sizeof(unsigned long long), st));
        KR_HIP(hipEventRecord(ev0, st));
        const int rc2 = launch_paths_for<true>(p, (kr_ray_f64*) d_rays, (long long) n, window_of(w), const_cast<long long*>((const long long*) d_offsets), nullptr,
                                               (double*) d_rows, (long long) total_rows, (unsigned long long*) counters.p, st);
        if (rc2 != KR_OK) return rc2;
        KR_HIP(hipEventRecord(ev1, st));
        unsigned long long h[kPWords];
        KR_HIP(hipMemcpyAsync(h, counters.p, sizeof h, hipMemcpyDeviceToHost, st));
        KR_HIP(hipStreamSynchronize(st));
        if (stats) {
            float ms = 0;
            KR_HIP(hipEventElapsedTime(&ms, ev0, ev1));
            stats->kernel_ms = ms;
            stats->rays_traced = (int64_t) h[kPTraced];
            stats->steps_total = (int64_t) h[kPSteps];
            stats->longest_ray_steps = (int64_t) h[kPLongest];
        }
        if (h[kPMismatch] != 0) {
            set_error("kr_trace_paths_record: " + std::to_string(h[kPMismatch]) + " rays wrote a different number of rows than the count pass gave them "
                      "(offsets from another call, other parameters, or rays[] modified in between?)");
            return KR_EINVAL;
        }
        return KR_OK;
    };
    rc = body();
    (void) hipEventDestroy(ev0);
    (void) hipEventDestroy(ev1);
    return rc;
}

}  // namespace kr
