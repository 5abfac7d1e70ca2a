// kr_observe.hip -- observing a volume map: camera rays are marched back through the emitting volume and, AS THEY STEP, gather the emissivity of the
// cells they cross into an energy spectrum, an energy-time response and a per-ray total (reference src/source_tracer/source_tracer.cpp,
// SourceTracer::propagate_source :102-310, stale there as Mapper was), as a third recorder on the trace's own persistent-wave loop.
//
// fp64, strict arithmetic, Euler and RK4 only -- the instances of kr_paths.hip and kr_volume.hip.  ObserveRecorder below rides trace_body
// (kr_trace_loop.hpp) exactly as VolumeRecorder does: an observed ray is claimed, reset, stepped and stored by the very code a flags = 0 trace runs, so
// it ends with the same record, bit for bit, and the states the recorder sees are the rows a write_step = 1 recording with an open window stores.
// This file has no loop of its own.  VolumeRecorder scatters into cells; this one is its mirror image: it gathers from cells and accumulates per ray,
// per energy bin and per (energy, time) bin.
//
// The rule (include/kr_trace.h states it in full).  ROWS and CELL are the volume map's (kr_volume.hip).  The step that produced a row moved the lane
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
// The ray's total lives in a register and is stored once, in leave().  The finishing kernel adds the launch's six tallies into the output's tail.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kr_pass.hpp"
#include "kr_trace_loop.hpp"

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
    double r_min, dr, log_dr, dtheta, dphi;      // log_dr: log(dr) from the host's C library (logbin)
    double V, spin;
    double en0, den, log_den, t0, dt;            // log_den: log(den) from the host's C library (logbin_en)
    const double* __restrict__ emis;
    const double* __restrict__ kappa;            // or null: optically thin
    const double* __restrict__ delay;            // or null: 0
    int32_t nr, ntheta, nphi, logbin, reverse, projradius, motion;
    int32_t nen, nt, logbin_en;
};

constexpr int kAggRounds = 8;      // energy bins per wave and step whose contributing lanes are summed before they add (KR_OBSERVE_ACC 1)

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
    bool flip_armed = false; int32_t status_before = 0;       // before_step -> after_step
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
        flip_armed = s.theta_was_positive; status_before = s.status; s.status = 0;
        r0 = s.r; theta0 = s.theta; phi0 = s.phi;
    }

    // the row's cell, or -1 outside the grid (VolumeRecorder::cell_of, kr_volume.hip: the same quotients)
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

    KR_DEV void add_spectrum(int32_t e, double w, double heads) const
    {
        atomicAdd(out + e, w);
        atomicAdd(out + g.nen + e, heads);
    }
    KR_DEV void add_response(int32_t et, double w) const { atomicAdd(out + 2 * (long long) g.nen + et, w); }

    // All 64 lanes, after every step of the wave: the lanes that contribute to the energy bin of the first contributing lane are summed and lane 0 adds
    // the sum; then the next bin, kAggRounds times at most; a lane whose bin nobody shares, or that is left over, adds for itself.
    KR_DEV void wave_step_end()
    {
        unsigned long long todo = __builtin_amdgcn_ballot_w64(dep_e >= 0);
        if (todo == 0) return;
#pragma unroll 1
        for (int round = 0; round < kAggRounds && todo != 0; ++round) {
            const int leader = __ffsll((long long) todo) - 1;
            const int32_t e = __builtin_amdgcn_readlane(dep_e, leader);
            const bool same = dep_e == e;
            const unsigned long long group = __builtin_amdgcn_ballot_w64(same);
            todo &= ~group;
            if (__popcll(group) == 1) continue;          // (that lane adds for itself below)
            const double sum_w = wave_sum(same ? dep_w : 0.0);
            if ((threadIdx.x & 63) == 0) add_spectrum(e, sum_w, (double) __popcll(group));
            if (g.nt > 0) {
                const int32_t et = __builtin_amdgcn_readlane(dep_et, leader);
                const bool same_et = same && dep_et == et;
                const double sum_et = wave_sum(same_et ? dep_w : 0.0);
                if (et >= 0 && (threadIdx.x & 63) == 0) add_response(et, sum_et);
                if (same && !same_et && dep_et >= 0) add_response(dep_et, dep_w);
            }
            if (same) dep_e = -1;
        }
        if (dep_e >= 0) {
            add_spectrum(dep_e, dep_w, 1.0);
            if (dep_et >= 0) add_response(dep_et, dep_w);
            dep_e = -1;
        }
    }

    template <bool USE_DEST> KR_DEV bool after_step(Lane<double>& s, bool fin)
    {
        const int32_t added = s.status;
        s.status = status_before | added;
        const bool flipped = flip_armed && !s.theta_was_positive;                               // `continue`
        const bool broke = (added & (KR_STATUS_HORIZON | (USE_DEST ? KR_STATUS_DEST : 0))) != 0;  // `break` before the row
        if (flipped || broke) return fin;
        ++rows;
        const int32_t cell = cell_of(s.r, s.theta, s.phi);
        if (cell < 0) return fin;
        ++in_grid;
        const double j = g.emis[cell];
        const double kap = g.kappa ? g.kappa[cell] : 0.0;
        if (!(j > 0) && !(kap > 0)) return fin;
        ++lit;
        const double dr = s.r - r0, dth = s.theta - theta0, dph = s.phi - phi0;
        const double a = g.spin, r = s.r;
        double sn, cs;
        kr_sincos_f64(s.theta, sn, cs);
        const double sigma = r * r + (a * cs) * (a * cs);
        const double delta = r * r - 2 * r + a * a;
        const double big_a = (r * r + a * a) * (r * r + a * a) - a * a * delta * sn * sn;
        const double len = kr_sqrt((sigma / delta) * dr * dr + sigma * dth * dth + (big_a * sn * sn / sigma) * dph * dph);
        if (!(len > 0 && len < __builtin_huge_val() && kr_abs(dph) < kPi / 2)) { ++degenerate; return fin; }
        if (j > 0) {
            kr_ray_f64 at;
            at.r = s.r; at.theta = s.theta; at.k = s.k; at.h = s.h; at.Q = s.Q; at.rdot_sign = s.rdot_sign; at.thetadot_sign = s.thetadot_sign; at.emit = emit;
            const double z = redshift_value<kr_ray_f64>(at, g.spin, g.V, g.reverse, g.projradius, g.motion);
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
        const unsigned long long w[kObserveTallies] = {wave_sum(rows), wave_sum(in_grid), wave_sum(lit), wave_sum(contributions), wave_sum(bad_g), wave_sum(degenerate)};
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < kObserveTallies; ++q)
                if (w[q]) atomicAdd(&counters[kRecorderWord + q], w[q]);
        }
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

// The finishing kernel: the launch's tallies into the output's tail (atomics: launches of other streams may be adding into the same output).
__global__ void __launch_bounds__(64) observe_finish_kernel(const unsigned long long* __restrict__ counters, double* __restrict__ tail)
{
    if (threadIdx.x < kObserveTallies) {
        const unsigned long long v = counters[kRecorderWord + threadIdx.x];
        if (v) atomicAdd(tail + threadIdx.x, (double) v);
    }
}

template <bool RK4, bool USE_DEST>
int launch_observe(kr_ray_f64* rays, long long n, const TraceConsts<double>& c, const ObserveGrid& g, double* out, double* image, unsigned long long* counters,
                   hipStream_t stream)
{
    auto kern = observe_kernel<RK4, USE_DEST>;
    int dev = 0, cus = 0, per_cu = 0;
    KR_HIP(hipGetDevice(&dev));
    const int rc = device_cus(dev, &cus);
    if (rc != KR_OK) return rc;
    KR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kTraceBlock, 0));
    per_cu = std::max(1, std::min(per_cu, 4 * (RK4 ? 2 : 4)));      // (launch_paths, kr_paths.hip)
    hipLaunchKernelGGL(kern, dim3(persistent_grid(cus, per_cu, n)), dim3(kTraceBlock), 0, stream, rays, n, c, g, out, image, counters);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int fail(const char* who, const char* what)
{
    set_error(std::string(who) + ": " + what);
    return KR_EINVAL;
}

}  // namespace

// everything that can be refused without a device (include/kr_trace.h lists it): what volume_validate refuses, then the bins
int observe_validate(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const char* who)
{
    const int rc = volume_validate(p, m, who);
    if (rc != KR_OK) return rc;
    if (!b) return fail(who, "null argument (bins)");
    if (b->nen < 1) return fail(who, "nen must be at least 1");
    if (b->nt < 0) return fail(who, "nt must not be negative (0: no response)");
    if (2 * (long long) b->nen + (long long) b->nen * b->nt > kMaxBins) return fail(who, "2 nen + nen nt is more than 2^27 bins");
    if (!(b->den > 0 && std::isfinite(b->den))) return fail(who, "den must be positive and finite");
    if (!std::isfinite(b->en0)) return fail(who, "en0 must be finite");
    if (b->logbin_en && !(b->den > 1)) return fail(who, "a logarithmic energy grid needs den > 1 (the ratio of successive edges)");
    if (b->logbin_en && !(b->en0 > 0)) return fail(who, "a logarithmic energy grid needs en0 > 0");
    if (b->nt > 0 && !(b->dt > 0 && std::isfinite(b->dt))) return fail(who, "dt must be positive and finite when nt > 0");
    if (!std::isfinite(b->t0)) return fail(who, "t0 must be finite");
    return KR_OK;
}

int trace_observe_dev(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const void* d_emis, const void* d_kappa, const void* d_delay, void* d_rays,
                      int64_t n, void* d_out, void* d_image, hipStream_t st, kr_stats* stats)
{
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->rays_total = n; }
    if (n == 0) return KR_OK;
    ObserveGrid g;
    g.r_min = m->r_min; g.dr = m->dr; g.log_dr = m->logbin ? std::log(m->dr) : 0.0; g.dtheta = m->dtheta; g.dphi = m->dphi;
    g.V = m->V; g.spin = p->spin;
    g.en0 = b->en0; g.den = b->den; g.log_den = b->logbin_en ? std::log(b->den) : 0.0; g.t0 = b->t0; g.dt = b->dt;
    g.emis = (const double*) d_emis; g.kappa = (const double*) d_kappa; g.delay = (const double*) d_delay;
    g.nr = m->nr; g.ntheta = m->ntheta; g.nphi = m->nphi; g.logbin = m->logbin; g.reverse = m->reverse; g.projradius = m->projradius; g.motion = m->motion;
    g.nen = b->nen; g.nt = b->nt; g.logbin_en = b->logbin_en;
    const long long nbins = 2 * (long long) b->nen + (long long) b->nen * b->nt;
    DeviceBuffer counters;
    int rc = counters.alloc(kObserveWords * sizeof(unsigned long long));
    if (rc != KR_OK) return rc;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KR_HIP(hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) { (void) hipEventDestroy(ev0); return hip_fail(hipGetLastError(), "hipEventCreate", __FILE__, __LINE__); }
    auto body = [&]() -> int {
        KR_HIP(hipMemsetAsync(counters.p, 0, kObserveWords * sizeof(unsigned long long), st));
        KR_HIP(hipEventRecord(ev0, st));
        const TraceConsts<double> c = make_consts<double>(p, effective_steplim(p));
        int rc2;
        if (p->integrator == KR_EULER) rc2 = launch_observe<false, false>((kr_ray_f64*) d_rays, (long long) n, c, g, (double*) d_out, (double*) d_image, (unsigned long long*) counters.p, st);
        else if (p->stop_kind == KR_STOP_THETA) rc2 = launch_observe<true, false>((kr_ray_f64*) d_rays, (long long) n, c, g, (double*) d_out, (double*) d_image, (unsigned long long*) counters.p, st);
        else rc2 = launch_observe<true, true>((kr_ray_f64*) d_rays, (long long) n, c, g, (double*) d_out, (double*) d_image, (unsigned long long*) counters.p, st);
        if (rc2 != KR_OK) return rc2;
        hipLaunchKernelGGL(observe_finish_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*) counters.p, (double*) d_out + nbins);
        KR_LAUNCH_CHECK();
        KR_HIP(hipEventRecord(ev1, st));
        unsigned long long h[kObserveWords];
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
