// kr_paths.hip -- the per-step trajectory dump of Raytracer<T>::run_raytrace(..., outfile, write_step, write_rmax, write_rmin, write_cartesian)
// (reference raytracer.cpp:86-100; the write rule :293-312 Euler, :923-942 and :1209-1228 RK4) as two passes of a persistent gfx950 kernel.
//
// fp64, strict arithmetic, Euler and RK4 only.  The kernel is the trace's own persistent-wave loop (trace_body, kr_trace_loop.hpp: one ray per lane,
// single-wave workgroups that refill their free lanes from a global queue) in its strict, non-HOG instance, with a recorder (PathRecorder below)
// called at the loop's hook points: a recorded ray is claimed, reset, stepped (step_fixed<double, RK4, USE_DEST, false>, kr_device.hpp) and stored by
// the very code a flags = 0 trace runs, so it takes the same steps and ends with the same record, bit for bit.  This file has no loop of its own;
// the recorder only counts and stores rows, and may end a ray that leaves the window.
//
// Rows are stored compressed: ray i owns rows[offsets[i] .. offsets[i + 1]).  Two passes make that possible without a worst-case allocation:
//   count   integrates every ray and stores only how many rows it writes (and whether it was traced at all); rays[] is not modified;
//           an exclusive scan turns the counts into offsets[0 .. n], offsets[n] is the total;
//   record  integrates again -- the same arithmetic, hence the same rows -- and stores row k of ray i at rows[offsets[i] + k], then the
//           final ray record as a trace does.  It counts what it writes; a ray whose count differs from its slab is reported, and no row is
//           ever stored outside the ray's slab or the buffer.
// A row is {t, r, theta, phi}: four doubles, 32 aligned bytes, two 16-byte vector stores.  Boyer-Lindquist always: write_cartesian is applied by
// the host-side writers (host/include/kerr.h cartesian()), with the C library the reference calls.
// Which iterations leave a row (RowGate), the launch and the host's timed run are the recorders' shared ones (kr_recorder.hpp).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kr_recorder.hpp"

namespace kr {

namespace {

constexpr int kScanBlock = 1024;
constexpr int kPathWords = kRecorderWord + 1;      // the trace's counter words, then the rays whose row count differs from their slab

struct PathWindow {
    double rmin, rmax;        // write_rmin, write_rmax: < 0 switches that side off
    int32_t write_step;
};

// (write_rmax < 0 || r < write_rmax) && (write_rmin < 0 || r > write_rmin), raytracer.cpp:295
KR_DEV bool in_window(const PathWindow& w, double r)
{
    return (w.rmax < 0 || r < w.rmax) && (w.rmin < 0 || r > w.rmin);
}

// The recorder of trace_body (kr_trace_loop.hpp lists the hooks).
// RECORD = false: the count pass.  offsets[i] receives ray i's row count (the scan below turns the counts into offsets), traced[i] (optional)
// whether the ray passed the skip rule; rays[] is read only -- kStoresRays is false, so the instance has no store to it.
// RECORD = true: offsets[0 .. n] are the scanned offsets; rows and the final ray records are stored.
template <bool RECORD> struct PathRecorder {
    static constexpr bool kActive = true, kStoresRays = RECORD, kWaveHook = false;
    PathWindow w;                     // the launch
    long long* __restrict__ offsets; unsigned char* __restrict__ traced; double* __restrict__ rows; long long total_rows;
    // this lane's ray
    long long slab = 0, cap = 0;      // RECORD: its first row and how many it may write
    int32_t n_rows = 0;               // rows it has written so far (write_started == n_rows > 0)
    int32_t until_write = 0;          // iterations left until steps % write_step == 0
    RowGate gate;
    uint32_t mismatch = 0;            // this lane's rays whose row count differed from their slab (32 bits: one register less across the step)

    KR_DEV void at_slot(long long slot, bool take)
    {
        if constexpr (!RECORD) {
            if (traced) traced[slot] = take ? 1 : 0;
            if (!take) offsets[slot] = 0;
        }
    }
    KR_DEV void claim(long long slot)
    {
        n_rows = 0;
        until_write = w.write_step;
        if constexpr (RECORD) { slab = offsets[slot]; cap = offsets[slot + 1] - slab; }
    }
    KR_DEV void before_step(Lane<double>& s) { gate.before_step(s); }
    template <bool USE_DEST> KR_DEV bool after_step(Lane<double>& s, bool fin)
    {
        const bool due = (--until_write == 0);            // steps % write_step == 0: every iteration increments steps once
        if (due) until_write = w.write_step;
        const bool row = gate.template row<USE_DEST>(s);
        if (due && row) {
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
        return fin;
    }
    KR_DEV void leave(long long idx)
    {
        if constexpr (RECORD) mismatch += (long long) n_rows != cap;
        else offsets[idx] = (long long) n_rows;
    }
    KR_DEV void at_exit(int lane, unsigned long long* __restrict__ counters)
    {
        const unsigned long long tally[1] = {mismatch};
        flush_tallies(tally, lane, counters);
    }
};

// resident waves per SIMD the register allocation must allow: as the strict trace kernels, RK4 3, Euler 4 (kr_trace.hip)
template <bool RK4, bool USE_DEST, bool RECORD>
__global__ void __attribute__((amdgpu_flat_work_group_size(kTraceBlock, kTraceBlock))) __attribute__((amdgpu_waves_per_eu(RK4 ? 3 : 4, 8)))
paths_kernel(kr_ray_f64* __restrict__ rays, long long n, TraceConsts<double> c, PathWindow w, long long* __restrict__ offsets, unsigned char* __restrict__ traced,
             double* __restrict__ rows, long long total_rows, unsigned long long* __restrict__ counters)
{
    int has_prio = 0;
    trace_body<double, RK4 ? KR_RK4 : KR_EULER, USE_DEST, false, false, KR_REFILL_MIN, false, PathRecorder<RECORD>>(
        rays, n, c, counters, nullptr, nullptr, 0, nullptr, 0, has_prio, -1, 0, PathRecorder<RECORD>{w, offsets, traced, rows, total_rows});
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

template <bool RECORD>
int launch_paths(const kr_params* p, kr_ray_f64* rays, long long n, const PathWindow& w, long long* offsets, unsigned char* traced, double* rows, long long total_rows,
                 unsigned long long* counters, hipStream_t stream)
{
    const TraceConsts<double> c = make_consts<double>(p, effective_steplim(p));
    return dispatch_instance(p, [&](auto rk4, auto dest) {
        constexpr bool RK4 = decltype(rk4)::value, USE_DEST = decltype(dest)::value;
        return launch_recorder(paths_kernel<RK4, USE_DEST, RECORD>, RK4, n, stream, rays, n, c, w, offsets, traced, rows, total_rows, counters);
    });
}

PathWindow window_of(const kr_path_spec* w) { return PathWindow{w->write_rmin, w->write_rmax, w->write_step}; }

}  // namespace

// everything that can be refused without a device (include/kr_trace.h lists it)
int paths_validate(const kr_params* p, const kr_path_spec* w, const char* who)
{
    if (!p || !w) return invalid_arg(who, "null argument");
    if (w->write_step <= 0) return invalid_arg(who, "write_step must be positive (the reference takes steps % write_step)");
    if (std::isnan(w->write_rmin) || std::isnan(w->write_rmax)) return invalid_arg(who, "write_rmin / write_rmax must not be NaN");
    if (p->flags & (KR_FLAG_FAST_MATH | KR_FLAG_HYBRID))
        return invalid_arg(who, "paths carry the reference's arithmetic: KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted");
    if (p->integrator == KR_RK45) return invalid_arg(who, "RK45 paths are not recorded (Euler and RK4 only)");
    return validate_run(p, who);      // (the checks the trace makes, under this call's name)
}

int paths_count_dev(const kr_params* p, const kr_path_spec* w, const void* d_rays, int64_t n, void* d_offsets, void* d_traced, int64_t* total_rows, hipStream_t st)
{
    DeviceBuffer counters;
    int rc = counters.alloc(kPathWords * sizeof(unsigned long long));
    if (rc != KR_OK) return rc;
    KR_HIP(hipMemsetAsync(counters.p, 0, kPathWords * sizeof(unsigned long long), st));
    if (n > 0) {
        // (the count pass only reads the records: the kernel's RECORD = false instance has no store to rays[])
        rc = launch_paths<false>(p, const_cast<kr_ray_f64*>((const kr_ray_f64*) d_rays), (long long) n, window_of(w), (long long*) d_offsets,
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
    if (need < 0 || (long long) total_rows < need) return invalid_arg("kr_trace_paths_record", "total_rows is smaller than offsets[n]");
    if (n == 0) return KR_OK;
    unsigned long long h[kPathWords];
    const int rc = run_recorder(st, kPathWords, stats, [&](unsigned long long* counters) {
        return launch_paths<true>(p, (kr_ray_f64*) d_rays, (long long) n, window_of(w), const_cast<long long*>((const long long*) d_offsets), nullptr, (double*) d_rows,
                                  (long long) total_rows, counters, st);
    }, h);
    if (rc != KR_OK) return rc;
    if (h[kRecorderWord] != 0) {
        set_error("kr_trace_paths_record: " + std::to_string(h[kRecorderWord]) + " rays wrote a different number of rows than the count pass gave them "
                  "(offsets from another call, other parameters, or rays[] modified in between?)");
        return KR_EINVAL;
    }
    return KR_OK;
}

}  // namespace kr
