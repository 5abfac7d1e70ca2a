// kr_volume.hip -- volume illumination maps: every ray is binned into an (r, theta, phi) grid AS IT STEPS, with its arrival time and energy shift
// (reference src/mapper/mapper.cpp, Mapper::map_ray :110-281; the deposit :230-265), as a second recorder on the trace's own persistent-wave loop.
//
// fp64, strict arithmetic, Euler and RK4 only -- the instances of kr_paths.hip.  VolumeRecorder below rides trace_body (kr_trace_loop.hpp) exactly as
// PathRecorder does: a mapped ray is claimed, reset, stepped and stored by the very code a flags = 0 trace runs, so it ends with the same record, bit
// for bit, and the states the recorder sees are the rows a write_step = 1 recording with an open window stores.  This file has no loop of its own.
//
// The rule (include/kr_trace.h states it in full).  A ROW is the state (t, r, theta, phi) after the update of every iteration that is neither a
// theta flip nor one that ended on the horizon or on dest->reached().  Its axis quotients are
//     q_r  = logbin ? log(r / r_min) / log(dr) : (r - r_min) / dr        q_th = theta / dtheta
//     q_ph = (phi_w + pi) / dphi,  phi_w = phi - 2 pi floor((phi + pi) / (2 pi))          (nphi == 1: no phi test, no wrap, iphi = 0)
// and it is IN THE GRID iff 0 <= q < n on every axis, decided on q itself (a NaN or infinite q is outside, like kr_emis_bins); the cell is
// ((int) q_r * ntheta + (int) q_th) * nphi + (int) q_ph.  Apart from the log every operation is one IEEE operation (-ffp-contract=off).
// A due deposit evaluates g = redshift_value (kr_post_device.hpp: the function the redshift pass applies) at the row, with the lane's signs and the
// emit of the ray's record; g > 0 and finite: count += 1, time += t, redshift += g; otherwise only bad_g moves.
//
// Two deliberate departures from the reference's text:
//   * its in-range test `ir > 0 && ir < Nr && ...` (:247) silently drops cell 0 of every axis.  Here cell 0 is a cell.
//   * it never assigns last_ir / last_itheta / last_iphi (:148-150, :246), so it deposits at EVERY step although what consumes the map
//     (Nrays / (num_rays * volume)) expects one deposit per crossing.  Both are offered: mode 0 (passage) keeps last_cell per lane, -1 at the claim;
//     a row deposits iff it is in the grid and its cell differs from last_cell, which then becomes the row's cell (-1 outside the grid) whether or
//     not g passed.  mode 1 (every row) is the reference's literal behaviour.
// Its velocity modes vel_mode 1 and 2 (V scaled with r / rmax) are left out.
//
// Accumulation.  A deposit is three f64 atomics (global_atomic_add_f64 under -munsafe-fp-atomics: no compare-and-swap loop), and they are what mapping
// costs: all rays start in the source's cell, and the rays of a wave -- neighbours in the source's (alpha, beta) grid, claimed together -- cross the
// same cells at the same steps, so lanes of one wave keep adding into the same few addresses.  Three forms are built (KR_VOLUME_ACC; figures in
// profiles/volume_map_ab.txt):
//   2 (the product)  per wave and step, the lanes that deposit into the same cell are summed in registers first and ONE lane adds the three sums
//                    (wave_step_end: at most kAggRounds cells per step, lanes left over add for themselves);
//   0                every lane adds into the caller's three planes for itself;
//   1                every lane adds into one 32-byte slot [count, time, redshift, pad] of a scratch buffer, and the finishing kernel adds the touched
//                    slots into the caller's planes -- one cache line per deposit instead of three, which measured no faster on a large grid and
//                    2.7 x slower on a small one (three atomics queue on one line).
// The finishing kernel also adds the launch's four tallies into the map's tail.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kr_pass.hpp"
#include "kr_trace_loop.hpp"

#ifndef KR_VOLUME_ACC
#define KR_VOLUME_ACC 2
#endif
#ifndef KR_VOLUME_EULER_WAVES
#define KR_VOLUME_EULER_WAVES 3      // resident waves per SIMD the Euler instance's register allocation must allow: 4, as paths_kernel has it, spills 73
                                     // registers and measured 16-18 % slower in passage mode (profiles/volume_map_ab.txt)
#endif

namespace kr {

namespace {

constexpr int kVolumeTallies = 4;                              // rows, in_grid, deposits, bad_g
constexpr int kVolumeWords = kRecorderWord + kVolumeTallies;   // the trace's counter words, then the tallies
constexpr long long kMaxCells = 1ll << 27;

struct VolumeGrid {
    double r_min, dr, log_dr, dtheta, dphi;      // log_dr: log(dr) from the host's C library (logbin)
    double V, spin;
    int32_t nr, ntheta, nphi, logbin, mode, reverse, projradius, motion;
};

constexpr int kAggRounds = 8;      // cells per wave and step whose depositing lanes are summed before they add (KR_VOLUME_ACC 2)

// The recorder of trace_body (kr_trace_loop.hpp lists the hooks).  acc: the caller's planes, or with KR_VOLUME_ACC 1 the [cell][4] scratch.
struct VolumeRecorder {
    static constexpr bool kActive = true, kStoresRays = true, kWaveHook = KR_VOLUME_ACC == 2;
    VolumeGrid g;                                  // the launch
    const kr_ray_f64* __restrict__ records;        // rays[]: emit is read at the claim (the loop's Lane does not carry it, and no kernel writes it)
    double* __restrict__ acc;
    // this lane's ray
    double emit = 0;
    int32_t last_cell = -1;
    bool flip_armed = false; int32_t status_before = 0;       // before_step -> after_step
    int32_t dep_cell = -1; double dep_t = 0, dep_z = 0;       // after_step -> wave_step_end: this step's deposit (dep_cell < 0: none)
    // this lane's tallies
    unsigned long long rows = 0, in_grid = 0, deposits = 0, bad_g = 0;

    KR_DEV void at_slot(long long, bool) {}
    KR_DEV void claim(long long slot)
    {
        last_cell = -1;
        emit = records[slot].emit;
    }
    KR_DEV void before_step(Lane<double>& s) { flip_armed = s.theta_was_positive; status_before = s.status; s.status = 0; }

    // the row's cell, or -1 outside the grid
    KR_DEV int32_t cell_of(double r, double theta, double phi) const
    {
        const double q_r = g.logbin ? kr_log(r / g.r_min) / g.log_dr : (r - g.r_min) / g.dr;
        const double q_th = theta / g.dtheta;
        if (!(q_r >= 0 && q_r < g.nr && q_th >= 0 && q_th < g.ntheta)) return -1;
        int32_t iphi = 0;
        if (g.nphi != 1) {
            const double phi_w = phi - (2 * kPi) * floor((phi + kPi) / (2 * kPi));
            const double q_ph = (phi_w + kPi) / g.dphi;
            if (!(q_ph >= 0 && q_ph < g.nphi)) return -1;
            iphi = (int32_t) q_ph;
        }
        return ((int32_t) q_r * g.ntheta + (int32_t) q_th) * g.nphi + iphi;
    }

    KR_DEV void add_to_planes(int32_t cell, double count, double t, double z) const
    {
        const long long ncell = (long long) g.nr * g.ntheta * g.nphi;
        atomicAdd(acc + cell, count);
        atomicAdd(acc + ncell + cell, t);
        atomicAdd(acc + 2 * ncell + cell, z);
    }

    // All 64 lanes, after every step of the wave: the lanes that deposit into the cell of the first depositing lane are summed and lane 0 adds the
    // sums; then the next cell, kAggRounds times at most; a lane whose cell nobody shares, or that is left over, adds for itself.
    KR_DEV void wave_step_end()
    {
        unsigned long long todo = __builtin_amdgcn_ballot_w64(dep_cell >= 0);
        if (todo == 0) return;
#pragma unroll 1
        for (int round = 0; round < kAggRounds && todo != 0; ++round) {
            const int leader = __ffsll((long long) todo) - 1;
            const int32_t cell = __builtin_amdgcn_readlane(dep_cell, leader);
            const bool same = dep_cell == cell;
            const unsigned long long group = __builtin_amdgcn_ballot_w64(same);
            todo &= ~group;
            if (__popcll(group) == 1) continue;          // (that lane adds for itself below)
            const double sum_t = wave_sum(same ? dep_t : 0.0), sum_z = wave_sum(same ? dep_z : 0.0);
            if ((threadIdx.x & 63) == 0) add_to_planes(cell, (double) __popcll(group), sum_t, sum_z);
            if (same) dep_cell = -1;
        }
        if (dep_cell >= 0) {
            add_to_planes(dep_cell, 1.0, dep_t, dep_z);
            dep_cell = -1;
        }
    }

    template <bool USE_DEST> KR_DEV bool after_step(Lane<double>& s, bool fin)
    {
        const int32_t added = s.status;
        s.status = status_before | added;
        const bool flipped = flip_armed && !s.theta_was_positive;                               // `continue`
        const bool broke = (added & (KR_STATUS_HORIZON | (USE_DEST ? KR_STATUS_DEST : 0))) != 0;  // `break` before the deposit
        if (!flipped && !broke) {
            ++rows;
            const int32_t cell = cell_of(s.r, s.theta, s.phi);
            const bool due = cell >= 0 && (g.mode != 0 || cell != last_cell);
            last_cell = cell;
            if (cell >= 0) ++in_grid;
            if (due) {
                kr_ray_f64 at;
                at.r = s.r; at.theta = s.theta; at.k = s.k; at.h = s.h; at.Q = s.Q; at.rdot_sign = s.rdot_sign; at.thetadot_sign = s.thetadot_sign; at.emit = emit;
                const double z = redshift_value<kr_ray_f64>(at, g.spin, g.V, g.reverse, g.projradius, g.motion);
                if (z > 0 && z < __builtin_huge_val()) {
                    ++deposits;
#if KR_VOLUME_ACC == 2
                    dep_cell = cell; dep_t = s.t; dep_z = z;
#elif KR_VOLUME_ACC == 1
                    double* slot = acc + 4 * (long long) cell;
                    atomicAdd(slot, 1.0);
                    atomicAdd(slot + 1, s.t);
                    atomicAdd(slot + 2, z);
#else
                    add_to_planes(cell, 1.0, s.t, z);
#endif
                } else {
                    ++bad_g;
                }
            }
        }
        return fin;
    }
    KR_DEV void leave(long long) {}
    KR_DEV void at_exit(int lane, unsigned long long* __restrict__ counters)
    {
        const unsigned long long w_rows = wave_sum(rows), w_in = wave_sum(in_grid), w_dep = wave_sum(deposits), w_bad = wave_sum(bad_g);
        if (lane == 0) {
            if (w_rows) atomicAdd(&counters[kRecorderWord], w_rows);
            if (w_in) atomicAdd(&counters[kRecorderWord + 1], w_in);
            if (w_dep) atomicAdd(&counters[kRecorderWord + 2], w_dep);
            if (w_bad) atomicAdd(&counters[kRecorderWord + 3], w_bad);
        }
    }
};

// resident waves per SIMD the register allocation must allow: 3 (paths_kernel, kr_paths.hip, gives its Euler instance 4: KR_VOLUME_EULER_WAVES above)
template <bool RK4, bool USE_DEST>
__global__ void __attribute__((amdgpu_flat_work_group_size(kTraceBlock, kTraceBlock))) __attribute__((amdgpu_waves_per_eu(RK4 ? 3 : KR_VOLUME_EULER_WAVES, 8)))
volume_kernel(kr_ray_f64* __restrict__ rays, long long n, TraceConsts<double> c, VolumeGrid g, double* __restrict__ acc, unsigned long long* __restrict__ counters)
{
    int has_prio = 0;
    trace_body<double, RK4 ? KR_RK4 : KR_EULER, USE_DEST, false, false, KR_REFILL_MIN, false, VolumeRecorder>(
        rays, n, c, counters, nullptr, nullptr, 0, nullptr, 0, has_prio, -1, 0, VolumeRecorder{g, rays, acc});
}

// The finishing kernel: the touched slots of the scratch into the caller's planes [count | time | redshift] (atomics: maps of other streams may be
// adding into the same planes), the launch's tallies into the map's tail.  scratch == nullptr (every form but KR_VOLUME_ACC 1): the tallies only.
__global__ void __launch_bounds__(kBlock) volume_finish_kernel(const double* __restrict__ scratch, long long ncell, const unsigned long long* __restrict__ counters,
                                                               double* __restrict__ map)
{
    if (scratch) {
        KR_GRID_STRIDE(i, ncell) {
            const double2 ct = reinterpret_cast<const double2*>(scratch + 4 * i)[0];
            if (ct.x != 0) {
                atomicAdd(map + i, ct.x);
                atomicAdd(map + ncell + i, ct.y);
                atomicAdd(map + 2 * ncell + i, scratch[4 * i + 2]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < kVolumeTallies) {
        const unsigned long long v = counters[kRecorderWord + threadIdx.x];
        if (v) atomicAdd(map + 3 * ncell + threadIdx.x, (double) v);
    }
}

template <bool RK4, bool USE_DEST>
int launch_volume(kr_ray_f64* rays, long long n, const TraceConsts<double>& c, const VolumeGrid& g, double* acc, unsigned long long* counters, hipStream_t stream)
{
    auto kern = volume_kernel<RK4, USE_DEST>;
    int dev = 0, cus = 0, per_cu = 0;
    KR_HIP(hipGetDevice(&dev));
    const int rc = device_cus(dev, &cus);
    if (rc != KR_OK) return rc;
    KR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kTraceBlock, 0));
    per_cu = std::max(1, std::min(per_cu, 4 * (RK4 ? 2 : 4)));      // (launch_paths, kr_paths.hip)
    hipLaunchKernelGGL(kern, dim3(persistent_grid(cus, per_cu, n)), dim3(kTraceBlock), 0, stream, rays, n, c, g, acc, counters);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int fail(const char* who, const char* what)
{
    set_error(std::string(who) + ": " + what);
    return KR_EINVAL;
}

bool positive_finite(double x) { return x > 0 && std::isfinite(x); }

}  // namespace

// everything that can be refused without a device (include/kr_trace.h lists it): the grid, then what the recording loop refuses (paths_validate)
int volume_validate(const kr_params* p, const kr_volume_map* m, const char* who)
{
    if (!p || !m) return fail(who, "null argument");
    if (m->nr < 1 || m->ntheta < 1 || m->nphi < 1) return fail(who, "nr, ntheta and nphi must be at least 1");
    if ((long long) m->nr * m->ntheta * m->nphi > kMaxCells || (long long) m->nr * m->ntheta > kMaxCells) return fail(who, "the grid has more than 2^27 cells");
    if (!positive_finite(m->dr) || !positive_finite(m->dtheta) || !positive_finite(m->dphi)) return fail(who, "dr, dtheta and dphi must be positive and finite");
    if (m->logbin && !(m->dr > 1)) return fail(who, "a logarithmic grid needs dr > 1 (the ratio of successive edges)");
    if (m->logbin && !positive_finite(m->r_min)) return fail(who, "a logarithmic grid needs r_min > 0");
    if (!std::isfinite(m->r_min)) return fail(who, "r_min must be finite");
    if (m->mode != 0 && m->mode != 1) return fail(who, "unknown mode (0: one deposit per passage of a cell, 1: one per row)");
    if (m->motion != 0 && m->motion != 1) return fail(who, "unknown motion (0: orbital, 1: radial)");
    const kr_path_spec every_row = {-1.0, -1.0, 1, 0};
    return paths_validate(p, &every_row, who);
}

int trace_volume_dev(const kr_params* p, const kr_volume_map* m, void* d_rays, int64_t n, void* d_map, hipStream_t st, kr_stats* stats)
{
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->rays_total = n; }
    if (n == 0) return KR_OK;
    const long long ncell = (long long) m->nr * m->ntheta * m->nphi;
    VolumeGrid g;
    g.r_min = m->r_min; g.dr = m->dr; g.log_dr = m->logbin ? std::log(m->dr) : 0.0; g.dtheta = m->dtheta; g.dphi = m->dphi;
    g.V = m->V; g.spin = p->spin;
    g.nr = m->nr; g.ntheta = m->ntheta; g.nphi = m->nphi; g.logbin = m->logbin; g.mode = m->mode; g.reverse = m->reverse; g.projradius = m->projradius; g.motion = m->motion;
    DeviceBuffer counters, scratch;
    int rc = counters.alloc(kVolumeWords * sizeof(unsigned long long));
    if (rc != KR_OK) return rc;
#if KR_VOLUME_ACC == 1
    rc = scratch.alloc((size_t) ncell * 4 * sizeof(double));
    if (rc != KR_OK) return rc;
#endif
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KR_HIP(hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) { (void) hipEventDestroy(ev0); return hip_fail(hipGetLastError(), "hipEventCreate", __FILE__, __LINE__); }
    auto body = [&]() -> int {
        KR_HIP(hipMemsetAsync(counters.p, 0, kVolumeWords * sizeof(unsigned long long), st));
        KR_HIP(hipEventRecord(ev0, st));
        if (scratch.p) KR_HIP(hipMemsetAsync(scratch.p, 0, (size_t) ncell * 4 * sizeof(double), st));
        double* acc = scratch.p ? (double*) scratch.p : (double*) d_map;
        const TraceConsts<double> c = make_consts<double>(p, effective_steplim(p));
        int rc2;
        if (p->integrator == KR_EULER) rc2 = launch_volume<false, false>((kr_ray_f64*) d_rays, (long long) n, c, g, acc, (unsigned long long*) counters.p, st);
        else if (p->stop_kind == KR_STOP_THETA) rc2 = launch_volume<true, false>((kr_ray_f64*) d_rays, (long long) n, c, g, acc, (unsigned long long*) counters.p, st);
        else rc2 = launch_volume<true, true>((kr_ray_f64*) d_rays, (long long) n, c, g, acc, (unsigned long long*) counters.p, st);
        if (rc2 != KR_OK) return rc2;
        hipLaunchKernelGGL(volume_finish_kernel, dim3(scratch.p ? grid_for(ncell, kBlock, kCapStream) : 1), dim3(kBlock), 0, st, (const double*) scratch.p, ncell,
                           (const unsigned long long*) counters.p, (double*) d_map);
        KR_LAUNCH_CHECK();
        KR_HIP(hipEventRecord(ev1, st));
        unsigned long long h[kVolumeWords];
        KR_HIP(hipMemcpyAsync(h, counters.p, sizeof h, hipMemcpyDeviceToHost, st));
        KR_HIP(hipStreamSynchronize(st));
        if (stats) {
            float ms = 0;
            KR_HIP(hipEventElapsedTime(&ms, ev0, ev1));
            stats->kernel_ms = ms;
            stats->rays_traced = (int64_t) h[kTraced];
            stats->steps_total = (int64_t) h[kSteps];
            stats->longest_ray_steps = (int64_t) h[kLongest];
        }
        return KR_OK;
    };
    rc = body();
    (void) hipEventDestroy(ev0);
    (void) hipEventDestroy(ev1);
    return rc;
}

}  // namespace kr
