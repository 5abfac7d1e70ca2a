// kr_surface.hip -- the emissivity histogram and the disc image of rays that LANDED ON A SURFACE (a RayDestination stop: KR_STATUS_DEST), binned by
// the cylindrical radius rho = r sin(theta) of the landing point.  The flat reducers of kr_post.hip hard-wire z = r cos(theta) < 1e-2 and bin by r:
// they cannot see a ray that ends on a disc of finite thickness (KR_STOP_THICKDISC).  include/kr_trace.h (kr_reduce_emissivity_surface_dev_f64,
// kr_reduce_image_surface_dev_f64) has the per-record rules and the layouts.
// One body each for the reducing form (records read only) and the fused form -- range_phi + redshift(V = -1, projradius = 1, motion = 0), the
// Keplerian observer at rho, + the sums, each record loaded once and left bit for bit as kr_range_phi_dev_f64 + kr_redshift_dev_f64 leave it.
// The six radial planes are accumulated per workgroup in LDS (ds_add_f64) when nr <= kMaxLdsBins and flushed with one global atomic per non-zero
// word; the four tallies go wave shuffle -> LDS -> one atomic per word and workgroup (as kr_return_map.hip's scalars).  The image takes global
// atomics: a ray lands in one pixel and the ray grid is about the pixel grid.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "kr_pass.hpp"

namespace kr {

namespace {

constexpr int kSurfacePlanes = 6;                // count, flux, emis, sum_redshift, sum_time, sum_z
constexpr int kSurfaceTallies = 4;               // disc_count, binned, upper, lower

// what both surface forms ask of a record before they look at where it landed
KR_DEV bool landed_on_surface(int steps, int status, double g) { return steps > 0 && (status & KR_STATUS_DEST) != 0 && g > 0; }

template <bool USE_LDS, bool FUSED>
KR_DEV void emissivity_surface_body(kr_ray_f64* __restrict__ rays, long long n, const kr_emis_bins& b, double* __restrict__ out, double spin, int reverse,
                                    double lo, double hi, double* lds, double (*part)[kSurfaceTallies])
{
    const int nr = b.nr;
    const int words = kSurfacePlanes * nr;
    if (USE_LDS) {
        for (int w = threadIdx.x; w < words; w += kBlock) lds[w] = 0;
        __syncthreads();
    }
    double* planes = USE_LDS ? lds : out;
    const double log_dr = kr_log(b.dr);
    double acc[kSurfaceTallies] = {0, 0, 0, 0};
    KR_GRID_STRIDE(i, n) {
        kr_ray_f64* ray = &rays[i];
        const int steps = ray->steps;
        const double r = ray->r, theta = ray->theta;
        double g;
        if (FUSED) {
            const kr_ray_f64 v = geodesic_of(ray);
            wrap_phi(ray, steps, lo, hi);
            g = redshift_value(v, spin, -1.0, reverse, 1, 0);
            ray->redshift = g;
        } else {
            g = ray->redshift;
        }
        if (!landed_on_surface(steps, ray->status, g)) continue;
        double sn, cs;
        kr_sincos(theta, sn, cs);
        const double rho = r * sn, z = r * cs;
        if (!(rho >= b.r_isco)) continue;
        acc[0] += 1;
        acc[2] += z > 0 ? 1 : 0;
        acc[3] += z < 0 ? 1 : 0;
        // the index rule of kr_emis_bins on the floating quotient (emissivity_accumulate, kr_post_device.hpp): NaN fails, (-1, 0] is bin 0
        const double q = b.logbin ? kr_log(rho / b.r_min) / log_dr : (rho - b.r_min) / b.dr;
        if (q > -1 && q < nr) {
            const int ir = (int) q;
            atomicAdd(&planes[ir], 1.0);
            atomicAdd(&planes[nr + ir], 1 / (b.num_primary_rays * kr_pow(g, 1.0)));
            atomicAdd(&planes[2 * nr + ir], 1 / kr_pow(g, b.gamma));
            atomicAdd(&planes[3 * nr + ir], g);
            atomicAdd(&planes[4 * nr + ir], ray->t);
            atomicAdd(&planes[5 * nr + ir], z);
            acc[1] += 1;
        }
    }
#pragma unroll
    for (int k = 0; k < kSurfaceTallies; k++) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();                             // the tallies' partial sums and, with USE_LDS, every wave's histogram additions
    if (threadIdx.x < kSurfaceTallies) {
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

template <bool USE_LDS, bool FUSED>
__global__ void __launch_bounds__(kBlock)
emissivity_surface_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_emis_bins b, double* __restrict__ out, double spin, int reverse, double lo, double hi)
{
    __shared__ double lds[USE_LDS ? kSurfacePlanes * kMaxLdsBins : 1];
    __shared__ double part[kBlock / 64][kSurfaceTallies];
    emissivity_surface_body<USE_LDS, FUSED>(rays, n, b, out, spin, reverse, lo, hi, lds, part);
}

// planes: [nrays | flux | rho | phi | enshift | time | emis](npix each) + disc_count: kr_reduce_image_dev_f64's layout and pixel rule, with the
// powerlaw3 emissivity taken at rho and the radius plane holding rho
template <bool FUSED>
__global__ void __launch_bounds__(kBlock)
image_surface_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_image_bins b, double* __restrict__ planes, double spin, int reverse, double lo, double hi)
{
    const long long npix = (long long) b.img_nx * b.img_ny;
    unsigned long long hits = 0;
    KR_GRID_STRIDE(i, n) {
        kr_ray_f64* ray = &rays[i];
        const int steps = ray->steps;
        const double r = ray->r, theta = ray->theta;
        double g, phi;
        if (FUSED) {
            const kr_ray_f64 v = geodesic_of(ray);
            g = redshift_value(v, spin, -1.0, reverse, 1, 0);
            ray->redshift = g;
            phi = wrap_phi(ray, steps, lo, hi);
        } else {
            g = ray->redshift;
            phi = ray->phi;
        }
        if (!landed_on_surface(steps, ray->status, g)) continue;
        const double rho = r * kr_sin(theta);
        if (!(rho >= b.r_isco && rho < b.r_disc)) continue;
        // the index rule of kr_image_bins per axis, on the floating quotient before the conversion (image_accumulate, kr_post.hip)
        const double qx = (ray->alpha - b.x0) / b.img_dx, qy = (ray->beta - b.y0) / b.img_dy;
        if (!(qx > -1 && qx < b.img_nx && qy > -1 && qy < b.img_ny)) continue;
        const int ix = (int) qx;
        const int iy = b.flip_image ? b.img_ny - (int) qy - 1 : (int) qy;
        const long long px = (long long) ix * b.img_ny + iy;
        const double e = powerlaw3(rho, b.q1, b.rb1, b.q2, b.rb2, b.q3);
        atomicAdd(&planes[px], 1.0);
        atomicAdd(&planes[npix + px], e / kr_pow(g, 3.0));
        atomicAdd(&planes[2 * npix + px], rho);
        atomicAdd(&planes[3 * npix + px], phi);
        atomicAdd(&planes[4 * npix + px], 1. / g);
        atomicAdd(&planes[5 * npix + px], ray->t);
        atomicAdd(&planes[6 * npix + px], e);
        hits += 1;
    }
    if (hits) atomicAdd(&planes[7 * npix], (double) hits);
}

template <bool FUSED>
int emissivity_surface_launch(const char* who, double spin, int reverse, double lo, double hi, const kr_emis_bins* b, void* d, int64_t n, void* d_hist, hipStream_t st)
{
    if (b->nr <= 0) { set_error(std::string(who) + ": nr must be positive"); return KR_EINVAL; }
    if (n <= 0) return KR_OK;
    const int grid = grid_for(n, kBlock, kCapHist);
    if (b->nr <= kMaxLdsBins)
        hipLaunchKernelGGL((emissivity_surface_kernel<true, FUSED>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *b, (double*) d_hist, spin, reverse, lo, hi);
    else
        hipLaunchKernelGGL((emissivity_surface_kernel<false, FUSED>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *b, (double*) d_hist, spin, reverse, lo, hi);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

template <bool FUSED>
int image_surface_launch(const char* who, double spin, int reverse, double lo, double hi, const kr_image_bins* b, void* d, int64_t n, void* d_planes, hipStream_t st)
{
    if (b->img_nx <= 0 || b->img_ny <= 0) { set_error(std::string(who) + ": image size must be positive"); return KR_EINVAL; }
    if (n <= 0) return KR_OK;
    hipLaunchKernelGGL(image_surface_kernel<FUSED>, dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *b, (double*) d_planes, spin,
                       reverse, lo, hi);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace

// the surface of the line, continuum and response passes: validate_run's rules for the stop_params of KR_STOP_THICKDISC (kr_trace.hip), word for word
int surface_validate(const kr_disc_surface* s, const char* who)
{
    const char* what = nullptr;
    if (!s) what = "null surface";
    else if (!std::isfinite(s->r_in) || !(s->r_in > 0)) what = "surface: r_in must be positive and finite";
    else if (!std::isfinite(s->r_out)) what = "surface: r_out must be finite (<= 0: open)";
    else if (!std::isfinite(s->slope) || s->slope < 0) what = "surface: slope must be non-negative and finite";
    else if (!std::isfinite(s->scale) || s->scale < 0) what = "surface: scale must be non-negative and finite";
    if (what) set_error(std::string(who) + ": " + what);
    return what ? KR_EINVAL : KR_OK;
}

int reduce_emissivity_surface_dev(const kr_emis_bins* b, const void* d, int64_t n, void* d_hist, hipStream_t st)
{
    return emissivity_surface_launch<false>("kr_reduce_emissivity_surface", 0.0, 0, 0.0, 0.0, b, const_cast<void*>(d), n, d_hist, st);
}

int post_emissivity_surface_dev(double spin, int reverse, double lo, double hi, const kr_emis_bins* b, void* d, int64_t n, void* d_hist, hipStream_t st)
{
    return emissivity_surface_launch<true>("kr_post_emissivity_surface", spin, reverse, lo, hi, b, d, n, d_hist, st);
}

int reduce_image_surface_dev(const kr_image_bins* b, const void* d, int64_t n, void* d_planes, hipStream_t st)
{
    return image_surface_launch<false>("kr_reduce_image_surface", 0.0, 0, 0.0, 0.0, b, const_cast<void*>(d), n, d_planes, st);
}

int post_image_surface_dev(double spin, int reverse, double lo, double hi, const kr_image_bins* b, void* d, int64_t n, void* d_planes, hipStream_t st)
{
    return image_surface_launch<true>("kr_post_image_surface", spin, reverse, lo, hi, b, d, n, d_planes, st);
}

}  // namespace kr
