// kr_angdist.hip -- where the rays of one source end, by EMISSION ANGLE (kr_angdist_spec, include/kr_trace.h): the loop of
// disc_source_return_angdist.cpp:132-196 as one more reducer of the post-pass framework.  Per traced record four angles of the source's own sky
// -- alpha, beta, the angle to the disc normal and the azimuth about it, from rays[].alpha (= cos alpha) and rays[].beta -- are binned into
// Nangle = (int) (2 pi / dangle) bins per class (escape / return / lost, the rule and the weight of kr_return_bins: ONE rule set with
// kr_reduce_return_f64 and the landing map), plus the two unweighted totals and eight tallies.
// One body for the reducing form (records read only) and the fused form (range_phi + redshift + the reduction, each record loaded once and left
// bit for bit as kr_range_phi_dev_f64 + kr_redshift_dev_f64 leave it).  The fourteen histograms are accumulated per workgroup in LDS (ds_add_f64)
// when 14 Nangle doubles fit the 40 KB the emissivity and line reducers take (Nangle <= 365; the default dangle = 0.1 gives 62), and flushed with
// one global atomic per non-zero word; above that the kernel adds into the global histograms directly, and there lanes of a wave that hit the
// same bin are summed first (hist_add below).  The tallies go wave shuffle -> LDS -> one
// atomic per word and workgroup, as in kr_return_map.hip.  acos is kr_crmath.hpp's correctly rounded routine, sin / cos kr_sincos.hpp's.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "kr_pass.hpp"
#include "kr_crmath.hpp"
#include "kr_recorder.hpp"

namespace kr {

namespace {

constexpr int kAngScalars = 8;                   // ray_count, escape, return, lost, other, skipped, out_of_range, bad_g
constexpr int kAngPlanes = 14;                   // 3 classes x {alpha, beta, norm, az} + total_norm + total_az
constexpr int kAngMaxBins = 4096;
constexpr int kAngLdsBins = 5 * kMaxLdsBins / kAngPlanes;      // 365: the histograms of a workgroup stay within the emissivity reducer's 40 KB

// (x + pi) / dangle as the reference forms it; the index rule of kr_emis_bins, decided on the quotient itself: a NaN fails, (-1, 0] is bin 0
KR_DEV bool angle_bin(double x, double dangle, int nangle, int& bin)
{
    const double q = (x + kPi) / dangle;
    if (!(q > -1 && q < nangle)) return false;
    bin = (int) q;
    return true;
}

// GROUPED: lanes of a wave that add under the same key are summed first (for_lane_groups, kr_recorder.hpp) and their leader adds once.  A source's
// grid puts the rays of one cos(alpha) -- at 1e7 rays also of one beta, norm and az bin -- next to each other, so a wave's 64 atomics go to a few words.
// Measured at 1e7 records (profiles/source_vel_ab.txt): on the GLOBAL histograms (Nangle > 365) grouping is 1.9 x faster, 2.1 ms against 4.0 ms; on
// the LDS histograms it is 1.3 x SLOWER, 0.84 ms against 0.62 ms -- the LDS takes same-address ds_add_f64 faster than the six group loops run.  So
// the global instantiation groups and the LDS one does not.  Every lane of the wave calls; key < 0: nothing to add.
// KR_ANGDIST_AGG = 0 / 2 build the never / always variants of that A/B.
#ifndef KR_ANGDIST_AGG
#define KR_ANGDIST_AGG 1
#endif
template <bool GROUPED>
KR_DEV void hist_add(double* planes, int32_t key, double w)
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
angdist_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_angdist_spec sp, int nangle, double* __restrict__ out, double spin, double V, int reverse,
               int projradius, int motion, double lo, double hi)
{
    __shared__ double lds[USE_LDS ? kAngPlanes * kAngLdsBins : 1];
    __shared__ double part[kBlock / 64][kAngScalars];
    const kr_return_bins& b = sp.cls;
    const int words = kAngPlanes * nangle;
    if (USE_LDS) {
        for (int w = threadIdx.x; w < words; w += kBlock) lds[w] = 0;
        __syncthreads();
    }
    double* planes = USE_LDS ? lds : out;
    double acc[kAngScalars] = {0, 0, 0, 0, 0, 0, 0, 0};
    // whole workgroups stride over the records, so that all 64 lanes of a wave reach the grouped adds together; a lane beyond n adds nothing
    for (long long base = blockIdx.x * (long long) kBlock; base < n; base += (long long) gridDim.x * kBlock) {
        const long long i = base + threadIdx.x;
        int32_t key_n = -1, key_z = -1, key_ca = -1, key_cb = -1, key_cn = -1, key_cz = -1;      // the two totals, the four histograms of the ray's class
        double w = 0;
        if (i < n) {
            kr_ray_f64* ray = &rays[i];
            const int steps = ray->steps;
            double phi, g;
            const double r = ray->r, theta = ray->theta;
            if (FUSED) {
                const kr_ray_f64 v = geodesic_of(ray);
                phi = wrap_phi(ray, steps, lo, hi);
                g = redshift_value(v, spin, V, reverse, projradius, motion);
                ray->redshift = g;
            } else {
                phi = ray->phi;
                g = ray->redshift;
            }
            const double cosalpha = ray->alpha;   // rays[].alpha holds cos(alpha)
            if (steps > 0) {
                if (!(g > 0)) acc[7] += 1;
                if (cosalpha == 0) {
                    acc[5] += 1;
                } else {
                    const double alpha = krcr::kr_acos_cr(cosalpha);
                    const double beta = ray->beta;
                    const double sin_alpha = kr_sin(alpha);
                    double sin_beta, cos_beta;
                    kr_sincos_f64(beta, sin_beta, cos_beta);
                    // labels 1 (records of kr_pointsource_vel_spec): that tetrad's leg 1 is +theta and leg 2 +phi, PointSource's are +phi and -theta, so its
                    // (alpha, beta) is PointSource's (alpha, beta - pi/2): sin(beta - pi/2) = -cos(beta), cos(beta - pi/2) = sin(beta), both exact here
                    if (sp.labels) { const double c0 = cos_beta; cos_beta = sin_beta; sin_beta = -1 * c0; }
                    const double s = sin_alpha * sin_beta;
                    const double sasb = kr_abs(s);
                    const double norm_angle = krcr::kr_acos_cr(sasb);
                    double az_angle = krcr::kr_acos_cr(-cosalpha / kr_sqrt(1 - s * s));
                    if (sin_alpha * cos_beta < 0) az_angle *= -1;
                    int ia, ib, in, iz;
                    // (all four evaluated: no short-circuit, so that the bins are defined together or not at all)
                    const bool ok_a = angle_bin(alpha, sp.dangle, nangle, ia), ok_b = angle_bin(beta, sp.dangle, nangle, ib);
                    const bool ok_n = angle_bin(norm_angle, sp.dangle, nangle, in), ok_z = angle_bin(az_angle, sp.dangle, nangle, iz);
                    if (!(ok_a && ok_b && ok_n && ok_z)) {
                        acc[6] += 1;
                    } else {
                        w = b.plane_iso ? sasb : 1;
                        if (b.limb) w *= 1 + 2.06 * sasb;
                        acc[0] += b.weight_norm ? w : 1;
                        key_n = 12 * nangle + in;
                        key_z = 13 * nangle + iz;
                        int cls = -1;            // 0 escape, 1 return, 2 lost: the order of the reference's output columns
                        if (theta >= kPi2 && r >= b.r_isco && r < b.r_disc) {
                            if (kr_abs(r - b.source_r) > 0.1 * b.source_r || kr_abs(phi - b.source_phi) > 0.1) cls = 1;
                        } else if (r > b.r_esc) {
                            cls = 0;
                        } else if (r < b.r_isco) {
                            cls = 2;
                        }
                        if (cls < 0) {
                            acc[4] += 1;
                        } else {
                            acc[1 + cls] += w;
                            const int h = 4 * cls * nangle;
                            key_ca = h + ia; key_cb = h + nangle + ib; key_cn = h + 2 * nangle + in; key_cz = h + 3 * nangle + iz;
                        }
                    }
                }
            }
        }
        constexpr bool kGrouped = KR_ANGDIST_AGG == 2 || (KR_ANGDIST_AGG == 1 && !USE_LDS);
        hist_add<kGrouped>(planes, key_n, 1.0);
        hist_add<kGrouped>(planes, key_z, 1.0);
        hist_add<kGrouped>(planes, key_ca, w);
        hist_add<kGrouped>(planes, key_cb, w);
        hist_add<kGrouped>(planes, key_cn, w);
        hist_add<kGrouped>(planes, key_cz, w);
    }
#pragma unroll
    for (int k = 0; k < kAngScalars; k++) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();                             // the tallies' partial sums and, with USE_LDS, every wave's histogram additions
    if (threadIdx.x < kAngScalars) {
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

}  // namespace

// Nangle = (int) (2 pi / dangle) as the reference forms it, or 0 when dangle gives none in 1 ... 4096
int angdist_nangle(const kr_angdist_spec* sp)
{
    const double q = 2 * kPi / sp->dangle;
    if (!(sp->dangle > 0) || !(q >= 1 && q < kAngMaxBins + 1)) return 0;
    return (int) q;
}

int angdist_validate(const kr_angdist_spec* sp, const char* who)
{
    if (!sp) return invalid_arg(who, "null spec");
    if (angdist_nangle(sp) == 0) return invalid_arg(who, "dangle must give 1 ... 4096 bins, Nangle = (int) (2 pi / dangle)");
    if (sp->labels != 0 && sp->labels != 1) return invalid_arg(who, "labels must be 0 (PointSource) or 1 (PointSourceVel)");
    return KR_OK;
}

int reduce_angdist_dev(const kr_angdist_spec* sp, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    const int nangle = angdist_nangle(sp);
    const int grid = grid_for(n, kBlock, kCapHist);
    if (nangle <= kAngLdsBins)
        hipLaunchKernelGGL((angdist_kernel<true, false>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *sp, nangle, (double*) d_out, 0.0, 0.0, 0, 0, 0, 0.0, 0.0);
    else
        hipLaunchKernelGGL((angdist_kernel<false, false>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *sp, nangle, (double*) d_out, 0.0, 0.0, 0, 0, 0, 0.0, 0.0);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int post_angdist_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_angdist_spec* sp, void* d, int64_t n, void* d_out,
                     hipStream_t st)
{
    if (n <= 0) return KR_OK;
    const int nangle = angdist_nangle(sp);
    const int grid = grid_for(n, kBlock, kCapHist);
    if (nangle <= kAngLdsBins)
        hipLaunchKernelGGL((angdist_kernel<true, true>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *sp, nangle, (double*) d_out, spin, V, reverse,
                           projradius, motion, lo, hi);
    else
        hipLaunchKernelGGL((angdist_kernel<false, true>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *sp, nangle, (double*) d_out, spin, V, reverse,
                           projradius, motion, lo, hi);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace kr
