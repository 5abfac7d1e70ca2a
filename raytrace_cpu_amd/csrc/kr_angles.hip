// kr_angles.hip -- the angle at which a photon meets the disc, in the rest frame of the orbiting gas (include/kr_trace.h, kr_angles_dev_f64): the
// momentum of each record projected on the reference's Tetrad (kerr.h:127-170) by frame_value (kr_post_device.hpp), which shares its metric, e_t and
// momentum with redshift_value.  mu = |P_th| / E is the cosine to the disc normal, chi = atan2(P_phi, P_r) the azimuth about it.
//   angles_kernel              records -> (mu, chi) per record; reads 144 B, writes 16 B, never touches the records
//   post_emissivity_mu_kernel  post_emissivity_kernel (kr_post.hip: range_phi + redshift + the radial histogram) with the histogram split by mu
// The limb-darkened line, post_line_limb_kernel, lives beside the line kernels whose bins it shares (kr_line.hip).
// Both histograms of the emissivity pass are privatised per workgroup in LDS when together they fit kMuLdsWords (ds_add_f64), flushed with one
// global atomic per non-zero word; above that the items add into the global arrays directly.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "kr_disc_pass.hpp"

namespace kr {

namespace {

// Per-workgroup LDS budget of the two privatised histograms, 5 nr + 1 and (2 nmu + 1) nr + 3 doubles: 6144 doubles = 48 KiB, below the 64 KiB a
// workgroup may ask for without an attribute.  Registers bound the residency first (-Rpass-analysis=kernel-resource-usage, gfx950:
// post_emissivity_mu 196 VGPRs -> 2 waves / SIMD = 2 workgroups / CU, angles 168 -> 3 and no LDS), and 2 x 48 KiB fit the CU's 160 KiB: the LDS
// never lowers the occupancy.  100 x 10 bins take 2 604 words, 30 x 64 take 4 024.
constexpr int kMuLdsWords = 6144;

// PLUNGE: the disc flow of KR_V_PLUNGE (DiscFlow, kr_post_device.hpp); the host picks the instance from V
template <bool PLUNGE>
__global__ void __launch_bounds__(kBlock)
angles_kernel(const kr_ray_f64* __restrict__ rays, long long n, double spin, double V, int reverse, int projradius, double* __restrict__ out, DiscFlow<PLUNGE> fl)
{
    KR_GRID_STRIDE(i, n) {
        const kr_ray_f64* ray = &rays[i];
        double mu = __builtin_nan(""), chi = __builtin_nan("");
        if (ray->steps > 0) {
            const Frame f = frame_value<PLUNGE>(geodesic_start_of(ray), spin, V, reverse, projradius, fl);
            mu = frame_mu(f);
            chi = frame_chi(f);
        }
        out[2 * i] = mu;
        out[2 * i + 1] = chi;
    }
}

// the angles to the normal of a disc surface (include/kr_trace.h, kr_angles_surface_dev_f64): mu = |P_n| / E, chi = atan2(P_phi, P_s) of every record
// with steps > 0, whatever it landed on, in the frame of the Keplerian observer at rho.  Sized freely the kernel takes 170 VGPRs, two over the three-wave
// line that angles_kernel sits on at 168; held to three waves per SIMD it takes 168 and spills two (profiles/surface_pass_ab.txt has both timed).
#ifdef KR_ANGLES_SURFACE_FREE                    // A/B builds only (scripts/surface_pass_ab.py --free-angles): no second launch bound
#define KR_ANGLES_SURFACE_BOUNDS __launch_bounds__(kBlock)
#else
#define KR_ANGLES_SURFACE_BOUNDS __launch_bounds__(kBlock, 3)
#endif
__global__ void KR_ANGLES_SURFACE_BOUNDS
angles_surface_kernel(const kr_ray_f64* __restrict__ rays, long long n, double spin, int reverse, double* __restrict__ out, DiscSurface<true> sf)
{
    KR_GRID_STRIDE(i, n) {
        const kr_ray_f64* ray = &rays[i];
        double mu = __builtin_nan(""), chi = __builtin_nan("");
        if (ray->steps > 0) {
            const kr_ray_f64 v = geodesic_start_of(ray);
            FrameCoef mc;
            const Frame f = frame_value_coef(v, spin, -1.0, reverse, 1, &mc);
            const SurfaceAngle s = surface_angle(sf, f, mc, v.r);
            mu = s.mu;
            chi = atan2(f.P_phi, s.P_s);
        }
        out[2 * i] = mu;
        out[2 * i + 1] = chi;
    }
}

// d_mu layout: [count2(nr nmu) | flux2(nr nmu) | sum_mu(nr) | disc_count, binned, bad_angle].  The radial histogram takes exactly what
// emissivity_accumulate gives it (bad-angle rays included); a ray that it binned radially goes on into (ir, im), or moves only bad_angle.
template <bool USE_LDS, bool PLUNGE>
__global__ void __launch_bounds__(kBlock)
post_emissivity_mu_kernel(kr_ray_f64* __restrict__ rays, long long n, double spin, double V, int reverse, int projradius, double lo, double hi, kr_emis_bins b,
                          int nmu, double* __restrict__ hist, double* __restrict__ out_mu, DiscFlow<PLUNGE> fl)
{
    extern __shared__ double lds[];
    const int nr = b.nr;
    const int hist_words = 5 * nr + 1, plane = nr * nmu, mu_words = 2 * plane + nr + 3;
    if (USE_LDS) {
        for (int w = threadIdx.x; w < hist_words + mu_words; w += kBlock) lds[w] = 0;
        __syncthreads();
    }
    double* acc = USE_LDS ? lds : hist;
    double* acc_mu = USE_LDS ? lds + hist_words : out_mu;
    const double log_dr = kr_log(b.dr);
    unsigned long long on_disc = 0, binned = 0, bad_angle = 0;
    KR_GRID_STRIDE(i, n) {
        kr_ray_f64* ray = &rays[i];
        const kr_ray_f64 v = geodesic_of(ray);
        const int steps = ray->steps;
        wrap_phi(ray, steps, lo, hi);
        const Frame f = frame_value<PLUNGE>(v, spin, V, reverse, projradius, fl);
        const double g = frame_redshift(f, v.emit, reverse);
        ray->redshift = g;
        emissivity_accumulate(acc, b, log_dr, steps, v.r, v.theta, g, ray->t);
        // the filter and the index rule of emissivity_accumulate, once more for the second histogram
        if (!(steps > 0) || !(v.r * kr_cos(v.theta) < 1E-2 && g > 0 && v.r >= b.r_isco)) continue;
        on_disc++;
        const double q = b.logbin ? kr_log(v.r / b.r_min) / log_dr : (v.r - b.r_min) / b.dr;
        if (!(q > -1 && q < nr)) continue;
        binned++;
        const double mu = frame_mu(f);
        if (frame_bad_angle(f, mu)) { bad_angle++; continue; }
        const int ir = (int) q, im = min((int) (mu * nmu), nmu - 1);
        atomicAdd(&acc_mu[ir * nmu + im], 1.0);
        atomicAdd(&acc_mu[plane + ir * nmu + im], 1 / (b.num_primary_rays * kr_pow(g, 1.0)));
        atomicAdd(&acc_mu[2 * plane + ir], mu);
    }
    if (on_disc) atomicAdd(&acc_mu[mu_words - 3], (double) on_disc);
    if (binned) atomicAdd(&acc_mu[mu_words - 2], (double) binned);
    if (bad_angle) atomicAdd(&acc_mu[mu_words - 1], (double) bad_angle);
    if (USE_LDS) {
        __syncthreads();
        for (int w = threadIdx.x; w < hist_words; w += kBlock)
            if (lds[w] != 0) atomicAdd(&hist[w], lds[w]);
        for (int w = threadIdx.x; w < mu_words; w += kBlock)
            if (lds[hist_words + w] != 0) atomicAdd(&out_mu[w], lds[hist_words + w]);
    }
}

}  // namespace

int angles_validate(int motion, const char* who)
{
    if (motion != 0) { set_error(std::string(who) + ": motion must be 0 (the orbiting observer)"); return KR_EINVAL; }
    return KR_OK;
}

int limb_validate(const kr_limb_law* law, const char* who)
{
    auto bad = [&](const char* why) { set_error(std::string(who) + ": " + why); return KR_EINVAL; };
    if (!law) return bad("null limb law");
    if (law->law < 0 || law->law > 2) return bad("limb law must be 0 (isotropic), 1 (1 + coeff mu) or 2 (log(1 + 1 / mu))");
    if (!std::isfinite(law->coeff)) return bad("non-finite limb coefficient");
    return KR_OK;
}

int emissivity_mu_validate(const kr_emis_bins* b, const kr_mu_bins* mb, const char* who)
{
    auto bad = [&](const char* why) { set_error(std::string(who) + ": " + why); return KR_EINVAL; };
    if (!b || !mb) return bad("null bins");
    if (b->nr <= 0) return bad("nr must be positive");
    if (mb->nmu < 1) return bad("nmu must be >= 1");
    if ((int64_t) b->nr * mb->nmu > ((int64_t) 1 << 24)) return bad("nr * nmu must not exceed 2^24");
    return KR_OK;
}

int angles_dev(double spin, double V, int reverse, int projradius, const void* d, int64_t n, void* d_angles, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    for_flow(spin, V, reverse, [&](auto flow) {
        hipLaunchKernelGGL(angles_kernel<decltype(flow)::plunge>, dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, (const kr_ray_f64*) d, (long long) n, spin, V, reverse,
                           projradius, (double*) d_angles, flow.arg);
    });
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int angles_surface_dev(const kr_disc_surface* s, double spin, int reverse, const void* d, int64_t n, void* d_angles, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    hipLaunchKernelGGL(angles_surface_kernel, dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, (const kr_ray_f64*) d, (long long) n, spin, reverse,
                       (double*) d_angles, surface_dev(s));
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int post_emissivity_mu_dev(double spin, double V, int reverse, int projradius, double lo, double hi, const kr_emis_bins* b, const kr_mu_bins* mb, void* d, int64_t n,
                           void* d_hist, void* d_mu, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    const int64_t words = (int64_t) 5 * b->nr + 1 + (2 * (int64_t) mb->nmu + 1) * b->nr + 3;
    KR_LAUNCH_LDS_OR_GLOBAL_FLOW(post_emissivity_mu_kernel, spin, V, reverse, words <= kMuLdsWords, grid_for(n, kBlock, kCapHist), (size_t) words * sizeof(double), st,
                                 (kr_ray_f64*) d, (long long) n, spin, V, reverse, projradius, lo, hi, *b, mb->nmu, (double*) d_hist, (double*) d_mu);
    return KR_OK;
}

}  // namespace kr
