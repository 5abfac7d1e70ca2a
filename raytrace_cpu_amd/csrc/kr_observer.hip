// kr_observer.hip -- the source-to-observer link (kr_observer_spec, include/kr_trace.h): the direct continuum of a source by OBSERVER INCLINATION.
// Per traced record the class of kr_return_bins (return / escape / lost / other, as kr_angdist.hip applies it); of an escaping ray the direction at
// infinity (the position angle plus the first-order rest of the way, r ptheta / pr), the energy at infinity over the emitted one (k / emit) and the
// arrival time on the sphere r = dist; binned by cos(theta_obs) into four planes (count, sum w, sum w shift, sum w t_ref) and an optional time row.
// One body for the reducing form (records read only) and the fused form (range_phi + redshift + the reduction, each record loaded once and left
// bit for bit as kr_range_phi_dev_f64 + kr_redshift_dev_f64 leave it).  The planes are accumulated per workgroup in LDS (ds_add_f64) when
// nmu (4 + nt) doubles fit the 40 KB the emissivity and line reducers take, and flushed with one global atomic per non-zero word; above that the
// kernel adds into the global planes directly, and there lanes of a wave that hit the same inclination bin (time row) are summed first: a source's
// grid puts neighbouring directions in neighbouring lanes.  The tallies go wave shuffle -> LDS -> one atomic per word and workgroup, as in
// kr_angdist.hip.  cos is kr_sincos.hpp's; log and pow are the device library's.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "kr_pass.hpp"
#include "kr_recorder.hpp"

namespace kr {

namespace {

constexpr int kObsScalars = 10;                  // ray_count, return, escape, lost, other, binned, outside_mu, outside_time, inbound, bad_g
constexpr int kObsPlanes = 4;                    // count, sum_w, sum_ws, sum_wt; then the nmu x nt time rows
constexpr int kObsMaxMu = 4096;
constexpr int kObsMaxWords = 1 << 24;
constexpr int kObsLdsWords = 5 * kMaxLdsBins;    // 5120 doubles: the planes of a workgroup stay within the emissivity reducer's 40 KB

// GROUPED: lanes of a wave that add under the same key are summed first (for_lane_groups, kr_recorder.hpp) and their leader adds once.
// kr_angdist.hip measured this on its histograms (profiles/source_vel_ab.txt): a gain on the global planes, a loss on the LDS ones; the same
// choice is made here, and KR_OBSERVER_AGG = 0 / 2 build the never / always variants for the A/B of profiles/observer_link_ab.txt.
// Every lane of the wave calls; key < 0: nothing to add.
#ifndef KR_OBSERVER_AGG
#define KR_OBSERVER_AGG 1
#endif

// the four planes of one inclination bin: one group loop for all of them
template <bool GROUPED>
KR_DEV void bin_add(double* planes, int nmu, int32_t imu, double w, double ws, double wt)
{
    if (GROUPED) {
        for_lane_groups<kAggRounds>(imu, [&](int32_t k, bool same, int lanes) {
            const double sum_w = wave_sum(same ? w : 0.0), sum_ws = wave_sum(same ? ws : 0.0), sum_wt = wave_sum(same ? wt : 0.0);
            if ((threadIdx.x & 63) == 0) {
                atomicAdd(&planes[k], (double) lanes);
                atomicAdd(&planes[nmu + k], sum_w);
                atomicAdd(&planes[2 * nmu + k], sum_ws);
                atomicAdd(&planes[3 * nmu + k], sum_wt);
            }
        });
    }
    if (imu >= 0) {
        atomicAdd(&planes[imu], 1.0);
        atomicAdd(&planes[nmu + imu], w);
        atomicAdd(&planes[2 * nmu + imu], ws);
        atomicAdd(&planes[3 * nmu + imu], wt);
    }
}

template <bool GROUPED>
KR_DEV void row_add(double* planes, int32_t key, double w)
{
    if (GROUPED) {
        for_lane_groups<kAggRounds>(key, [&](int32_t k, bool same, int lanes) {
            const double sum = wave_sum(same ? w : 0.0);
            if ((threadIdx.x & 63) == 0) atomicAdd(&planes[k], sum);
        });
    }
    if (key >= 0) atomicAdd(&planes[key], w);
}

template <bool USE_LDS, bool FUSED>
__global__ void __launch_bounds__(kBlock)
observer_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_observer_spec sp, double* __restrict__ out, double spin, double V, int reverse, int projradius,
                int motion, double lo, double hi)
{
    __shared__ double lds[USE_LDS ? kObsLdsWords : 1];
    __shared__ double part[kBlock / 64][kObsScalars];
    const kr_return_bins& b = sp.cls;
    const int nmu = sp.nmu, nt = sp.nt;
    const int words = nmu * (kObsPlanes + nt);   // <= 2^24 (observer_validate); with USE_LDS <= kObsLdsWords (the launchers)
    if (USE_LDS) {
        for (int w = threadIdx.x; w < words; w += kBlock) lds[w] = 0;
        __syncthreads();
    }
    double* planes = USE_LDS ? lds : out;
    double acc[kObsScalars] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // whole workgroups stride over the records, so that all 64 lanes of a wave reach the grouped adds together; a lane beyond n adds nothing
    for (long long base = blockIdx.x * (long long) kBlock; base < n; base += (long long) gridDim.x * kBlock) {
        const long long i = base + threadIdx.x;
        int32_t key_mu = -1, key_t = -1;         // the inclination bin, and the word of the time row: both in [0, words) or -1
        double w = 0, ws = 0, wt = 0;
        if (i < n) {
            kr_ray_f64* ray = &rays[i];
            const int steps = ray->steps;
            const kr_ray_f64 v = geodesic_of(ray);
            const double r = v.r, theta = v.theta;
            double phi;
            if (FUSED) {
                phi = wrap_phi(ray, steps, lo, hi);
                ray->redshift = redshift_value(v, spin, V, reverse, projradius, motion);
            } else {
                phi = ray->phi;
            }
            if (steps > 0) {
                acc[0] += 1;
                int cls = -1;                    // 0 escape, 1 return, 2 lost: kr_angdist.hip's classification
                if (theta >= kPi2 && r >= b.r_isco && r < b.r_disc) {
                    if (kr_abs(r - b.source_r) > 0.1 * b.source_r || kr_abs(phi - b.source_phi) > 0.1) cls = 1;
                } else if (r > b.r_esc) {
                    cls = 0;
                } else if (r < b.r_isco) {
                    cls = 2;
                }
                if (cls < 0) acc[4] += 1;
                else if (cls == 1) acc[1] += 1;
                else if (cls == 2) acc[3] += 1;
                else {
                    acc[2] += 1;
                    double pt, pr, ptheta, pphi;
                    momentum<double>(pt, pr, ptheta, pphi, v.k, v.h, v.Q, v.rdot_sign, v.thetadot_sign, r, theta, sp.spin);
                    const double shift = v.k / v.emit;          // E_inf = + k (include/kr_trace.h)
                    if (!(pr > 0) || !__builtin_isfinite(pt) || !__builtin_isfinite(pr) || !__builtin_isfinite(ptheta) || !__builtin_isfinite(pphi)) {
                        acc[8] += 1;
                    } else if (!(shift > 0)) {
                        acc[9] += 1;
                    } else {
                        const double theta_obs = theta + r * ptheta / pr;
                        double sin_obs, mu;
                        kr_sincos_f64(theta_obs, sin_obs, mu);
                        const double q = (mu - sp.mu0) / sp.dmu;
                        if (!(q > -1 && q < nmu)) {
                            acc[6] += 1;
                        } else {
                            key_mu = (int) q;
                            acc[5] += 1;
                            const double t = ray->t;
                            const double t_ref = sp.dist > 0 ? t + (sp.dist - r) + 2 * kr_log(sp.dist / r) : t;
                            w = kr_pow(shift, sp.gamma);
                            ws = w * shift;
                            wt = w * t_ref;
                            if (nt > 0) {
                                const double ft = (t_ref - sp.t0) / sp.dt;
                                if (ft >= 0 && ft < nt) key_t = kObsPlanes * nmu + key_mu * nt + (int) ft;      // (a NaN fails)
                                else acc[7] += 1;
                            }
                        }
                    }
                }
            }
        }
        constexpr bool kGrouped = KR_OBSERVER_AGG == 2 || (KR_OBSERVER_AGG == 1 && !USE_LDS);
        row_add<kGrouped>(planes, key_t, w);
        bin_add<kGrouped>(planes, nmu, key_mu, w, ws, wt);
    }
#pragma unroll
    for (int k = 0; k < kObsScalars; k++) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();                             // the tallies' partial sums and, with USE_LDS, every wave's additions to the planes
    if (threadIdx.x < kObsScalars) {
        double v = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) v += part[w][threadIdx.x];
        if (v != 0) atomicAdd(&out[words + threadIdx.x], v);
    }
    if (USE_LDS) {
        for (int w = threadIdx.x; w < words; w += kBlock)
            if (lds[w] != 0) atomicAdd(&out[w], lds[w]);
    }
}

template <bool FUSED>
int observer_launch(const kr_observer_spec* sp, kr_ray_f64* d, int64_t n, void* d_out, hipStream_t st, double spin, double V, int reverse, int projradius, int motion,
                    double lo, double hi)
{
    if (n <= 0) return KR_OK;
    const int grid = grid_for(n, kBlock, kCapHist);
    if (observer_words(sp) - kObsScalars <= kObsLdsWords)
        hipLaunchKernelGGL((observer_kernel<true, FUSED>), dim3(grid), dim3(kBlock), 0, st, d, (long long) n, *sp, (double*) d_out, spin, V, reverse, projradius, motion, lo, hi);
    else
        hipLaunchKernelGGL((observer_kernel<false, FUSED>), dim3(grid), dim3(kBlock), 0, st, d, (long long) n, *sp, (double*) d_out, spin, V, reverse, projradius, motion, lo, hi);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace

// nmu (4 + nt) + 10 of a spec that passed observer_validate
int64_t observer_words(const kr_observer_spec* sp) { return (int64_t) sp->nmu * (kObsPlanes + sp->nt) + kObsScalars; }

int observer_validate(const kr_observer_spec* sp, const char* who)
{
    if (!sp) return invalid_arg(who, "null spec");
    if (sp->nmu < 1 || sp->nmu > kObsMaxMu) return invalid_arg(who, "nmu must be in 1 ... 4096");
    if (sp->nt < 0) return invalid_arg(who, "nt must be >= 0");
    if ((int64_t) sp->nmu * (kObsPlanes + (int64_t) sp->nt) > kObsMaxWords) return invalid_arg(who, "nmu * (4 + nt) must not exceed 2^24");
    if (!positive_finite(sp->dmu)) return invalid_arg(who, "dmu must be positive and finite");
    if (sp->nt > 0 && !positive_finite(sp->dt)) return invalid_arg(who, "dt must be positive and finite");
    if (!std::isfinite(sp->mu0) || !std::isfinite(sp->t0) || !std::isfinite(sp->gamma) || !std::isfinite(sp->spin))
        return invalid_arg(who, "non-finite mu0, t0, gamma or spin");
    if (!(sp->dist >= 0) || !std::isfinite(sp->dist)) return invalid_arg(who, "dist must be >= 0 and finite");
    return KR_OK;
}

int reduce_observer_dev(const kr_observer_spec* sp, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return observer_launch<false>(sp, (kr_ray_f64*) d, n, d_out, st, 0.0, 0.0, 0, 0, 0, 0.0, 0.0);
}

int post_observer_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_observer_spec* sp, void* d, int64_t n, void* d_out,
                      hipStream_t st)
{
    return observer_launch<true>(sp, (kr_ray_f64*) d, n, d_out, st, spin, V, reverse, projradius, motion, lo, hi);
}

}  // namespace kr
