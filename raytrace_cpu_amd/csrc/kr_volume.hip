// kr_volume.hip -- volume illumination maps: every ray is binned into an (r, theta, phi) grid AS IT STEPS, with its arrival time and energy shift
// (reference src/mapper/mapper.cpp, Mapper::map_ray :110-281; the deposit :230-265), as a second recorder on the trace's own persistent-wave loop.
//
// fp64, strict arithmetic, Euler and RK4 only -- the instances of kr_paths.hip.  VolumeRecorder below rides trace_body (kr_trace_loop.hpp) exactly as
// PathRecorder does: a mapped ray is claimed, reset, stepped and stored by the very code a flags = 0 trace runs, so it ends with the same record, bit
// for bit, and the states the recorder sees are the rows a write_step = 1 recording with an open window stores.  This file has no loop of its own.
//
// The rule (include/kr_trace.h states it in full).  ROWS, the CELL a row lies in and the energy shift g at a row are the recorders' shared ones
// (kr_recorder.hpp: RowGate, CellGrid, ObserverFrame).  A due deposit evaluates g at the row; g > 0 and finite: count += 1, time += t, redshift += g;
// otherwise only bad_g moves.
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
// same cells at the same steps, so lanes of one wave keep adding into the same few addresses.  Two forms are built (KR_VOLUME_ACC; figures in
// profiles/volume_map_ab.txt, with those of a third that lost):
//   2 (the product)  per wave and step, the lanes that deposit into the same cell are summed in registers first and ONE lane adds the three sums
//                    (wave_step_end: at most kAggRounds cells per step, lanes left over add for themselves);
//   0                every lane adds into the caller's three planes for itself.
// add_tallies_kernel adds the launch's four tallies into the map's tail.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kr_recorder.hpp"

#ifndef KR_VOLUME_ACC
#define KR_VOLUME_ACC 2
#endif
#if KR_VOLUME_ACC != 0 && KR_VOLUME_ACC != 2
#error "KR_VOLUME_ACC: 2 (wave-aggregated, the product) or 0 (every lane for itself)"
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
    CellGrid cells;
    ObserverFrame frame;
    int32_t mode;
};

// What the kernel is handed: VolumeGrid's fields, doubles first.  The order of the kernel arguments decides which scalar registers the compiler spills:
// handed the nested struct, the Euler instance reloads 307 spilled scalars instead of 205 and measured 7-15 % slower in passage mode
// (profiles/recorder_shared_ab.txt).
struct VolumeArgs {
    double r_min, dr, log_dr, dtheta, dphi, V, spin;
    int32_t nr, ntheta, nphi, logbin, mode, reverse, projradius, motion;

    VolumeArgs(const CellGrid& c, const ObserverFrame& f, int32_t mode_)
        : r_min(c.r_min), dr(c.dr), log_dr(c.log_dr), dtheta(c.dtheta), dphi(c.dphi), V(f.V), spin(f.spin), nr(c.nr), ntheta(c.ntheta), nphi(c.nphi), logbin(c.logbin),
          mode(mode_), reverse(f.reverse), projradius(f.projradius), motion(f.motion) {}
    KR_DEV VolumeGrid grid() const { return VolumeGrid{{r_min, dr, log_dr, dtheta, dphi, nr, ntheta, nphi, logbin}, {V, spin, reverse, projradius, motion}, mode}; }
};

// The recorder of trace_body (kr_trace_loop.hpp lists the hooks).  acc: the caller's planes [count | time | redshift].
struct VolumeRecorder {
    static constexpr bool kActive = true, kStoresRays = true, kWaveHook = KR_VOLUME_ACC == 2;
    VolumeGrid g;                                  // the launch
    const kr_ray_f64* __restrict__ records;        // rays[]: emit is read at the claim (the loop's Lane does not carry it, and no kernel writes it)
    double* __restrict__ acc;
    // this lane's ray
    double emit = 0;
    int32_t last_cell = -1;
    RowGate gate;
    int32_t dep_cell = -1; double dep_t = 0, dep_z = 0;       // after_step -> wave_step_end: this step's deposit (dep_cell < 0: none)
    // this lane's tallies
    unsigned long long rows = 0, in_grid = 0, deposits = 0, bad_g = 0;

    KR_DEV void at_slot(long long, bool) {}
    KR_DEV void claim(long long slot)
    {
        last_cell = -1;
        emit = records[slot].emit;
    }
    KR_DEV void before_step(Lane<double>& s) { gate.before_step(s); }

    KR_DEV void add_to_planes(int32_t cell, double count, double t, double z) const
    {
        const long long ncell = (long long) g.cells.nr * g.cells.ntheta * g.cells.nphi;
        atomicAdd(acc + cell, count);
        atomicAdd(acc + ncell + cell, t);
        atomicAdd(acc + 2 * ncell + cell, z);
    }

    // All 64 lanes, after every step of the wave: the lanes that deposit into the cell of the first depositing lane are summed and lane 0 adds the
    // sums; then the next cell, kAggRounds times at most; a lane whose cell nobody shares, or that is left over, adds for itself.
    KR_DEV void wave_step_end()
    {
        for_lane_groups<kAggRounds>(dep_cell, [&](int32_t cell, bool same, int lanes) {
            const double sum_t = wave_sum(same ? dep_t : 0.0), sum_z = wave_sum(same ? dep_z : 0.0);
            if ((threadIdx.x & 63) == 0) add_to_planes(cell, (double) lanes, sum_t, sum_z);
        });
        if (dep_cell >= 0) {
            add_to_planes(dep_cell, 1.0, dep_t, dep_z);
            dep_cell = -1;
        }
    }

    template <bool USE_DEST> KR_DEV bool after_step(Lane<double>& s, bool fin)
    {
        if (gate.template row<USE_DEST>(s)) {
            ++rows;
            const int32_t cell = g.cells.cell_of(s.r, s.theta, s.phi);
            const bool due = cell >= 0 && (g.mode != 0 || cell != last_cell);
            last_cell = cell;
            if (cell >= 0) ++in_grid;
            if (due) {
                const double z = g.frame.row_shift(s, emit);
                if (z > 0 && z < __builtin_huge_val()) {
                    ++deposits;
#if KR_VOLUME_ACC == 2
                    dep_cell = cell; dep_t = s.t; dep_z = z;
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
        const unsigned long long tally[kVolumeTallies] = {rows, in_grid, deposits, bad_g};
        flush_tallies(tally, lane, counters);
    }
};

// resident waves per SIMD the register allocation must allow: 3 (paths_kernel, kr_paths.hip, gives its Euler instance 4: KR_VOLUME_EULER_WAVES above)
template <bool RK4, bool USE_DEST>
__global__ void __attribute__((amdgpu_flat_work_group_size(kTraceBlock, kTraceBlock))) __attribute__((amdgpu_waves_per_eu(RK4 ? 3 : KR_VOLUME_EULER_WAVES, 8)))
volume_kernel(kr_ray_f64* __restrict__ rays, long long n, TraceConsts<double> c, VolumeArgs a, double* __restrict__ acc, unsigned long long* __restrict__ counters)
{
    int has_prio = 0;
    trace_body<double, RK4 ? KR_RK4 : KR_EULER, USE_DEST, false, false, KR_REFILL_MIN, false, VolumeRecorder>(
        rays, n, c, counters, nullptr, nullptr, 0, nullptr, 0, has_prio, -1, 0, VolumeRecorder{a.grid(), rays, acc});
}

}  // namespace

// everything that can be refused without a device (include/kr_trace.h lists it): the grid, then what the recording loop refuses (paths_validate)
int volume_validate(const kr_params* p, const kr_volume_map* m, const char* who)
{
    if (!p || !m) return invalid_arg(who, "null argument");
    if (const int rc = refuse_plunge(m->V, who)) return rc;
    if (m->nr < 1 || m->ntheta < 1 || m->nphi < 1) return invalid_arg(who, "nr, ntheta and nphi must be at least 1");
    if ((long long) m->nr * m->ntheta * m->nphi > kMaxCells || (long long) m->nr * m->ntheta > kMaxCells) return invalid_arg(who, "the grid has more than 2^27 cells");
    if (!positive_finite(m->dr) || !positive_finite(m->dtheta) || !positive_finite(m->dphi)) return invalid_arg(who, "dr, dtheta and dphi must be positive and finite");
    if (m->logbin && !(m->dr > 1)) return invalid_arg(who, "a logarithmic grid needs dr > 1 (the ratio of successive edges)");
    if (m->logbin && !positive_finite(m->r_min)) return invalid_arg(who, "a logarithmic grid needs r_min > 0");
    if (!std::isfinite(m->r_min)) return invalid_arg(who, "r_min must be finite");
    if (m->mode != 0 && m->mode != 1) return invalid_arg(who, "unknown mode (0: one deposit per passage of a cell, 1: one per row)");
    if (m->motion != 0 && m->motion != 1) return invalid_arg(who, "unknown motion (0: orbital, 1: radial)");
    const kr_path_spec every_row = {-1.0, -1.0, 1, 0};
    return paths_validate(p, &every_row, who);
}

int trace_volume_dev(const kr_params* p, const kr_volume_map* m, void* d_rays, int64_t n, void* d_map, hipStream_t st, kr_stats* stats)
{
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->rays_total = n; }
    if (n == 0) return KR_OK;
    const long long ncell = (long long) m->nr * m->ntheta * m->nphi;
    const VolumeArgs a(cell_grid_of(m), observer_frame_of(p, m), m->mode);
    const TraceConsts<double> c = make_consts<double>(p, effective_steplim(p));
    unsigned long long h[kVolumeWords];
    return run_recorder(st, kVolumeWords, stats, [&](unsigned long long* counters) -> int {
        const int rc = dispatch_instance(p, [&](auto rk4, auto dest) {
            constexpr bool RK4 = decltype(rk4)::value, USE_DEST = decltype(dest)::value;
            return launch_recorder(volume_kernel<RK4, USE_DEST>, RK4, n, st, (kr_ray_f64*) d_rays, n, c, a, (double*) d_map, counters);
        });
        if (rc != KR_OK) return rc;
        hipLaunchKernelGGL(add_tallies_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*) counters, kVolumeTallies, (double*) d_map + 3 * ncell);
        KR_LAUNCH_CHECK();
        return KR_OK;
    }, h);
}

}  // namespace kr
