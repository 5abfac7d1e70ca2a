// kr_polarisation.hip -- the polarisation of disc emission seen on a distant image plane (include/kr_trace.h, kr_pol_law): the emitted polarisation
// vector in the rest frame of the orbiting gas, carried to the observer by the Walker-Penrose constant -- conserved along the ray, so nothing is
// integrated: polar_value (kr_post_device.hpp) evaluates it at the disc from what the record holds and inverts it with the ray's image-plane
// coordinates, in the same metric and momentum evaluation that gives the redshift and mu.
//   polarisation_kernel        records -> (kappa1, kappa2, c2, s2) per record; reads 144 B, writes 32 B, never touches the records
//   post_image_stokes_kernel   post_image_kernel (kr_post.hip: redshift + range_phi + the image) with the planes [nrays | I | Q | U]
// The energy-resolved form, post_line_stokes_kernel, lives beside the line kernels whose bins it shares (kr_line.hip).
// A ray lands in one pixel and the ray grid is about the pixel grid, so contention is low: global f64 atomics, as in the image reducer.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "kr_pass.hpp"

namespace kr {

namespace {

__global__ void __launch_bounds__(kBlock)
polarisation_kernel(const kr_ray_f64* __restrict__ rays, long long n, double spin, double V, int reverse, int projradius, double sin_incl, double* __restrict__ out)
{
    KR_GRID_STRIDE(i, n) {
        const kr_ray_f64* ray = &rays[i];
        double kappa1 = __builtin_nan(""), kappa2 = kappa1, c2 = kappa1, s2 = kappa1;
        if (ray->steps > 0) {
            const Polar q = polar_value(polar_record_of(ray), spin, V, reverse, projradius, sin_incl);
            kappa1 = q.kappa1; kappa2 = q.kappa2; c2 = q.c2; s2 = q.s2;
        }
        out[4 * i] = kappa1;
        out[4 * i + 1] = kappa2;
        out[4 * i + 2] = c2;
        out[4 * i + 3] = s2;
    }
}

// the filter and the pixel rule of image_accumulate (kr_post.hip), once more for the Stokes planes: the pixel [ix img_ny + iy], or -1
KR_DEV long long stokes_pixel(const kr_image_bins& b, int steps, double r, double theta, double g, double alpha, double beta)
{
    if (!(steps > 0)) return -1;
    const double z = r * kr_cos(theta);
    if (!(z < 1E-2 && r >= b.r_isco && r < b.r_disc && g > 0)) return -1;         // disc_filter (kr_disc_pass.hpp), written out: the call changes this kernel's code
    const double qx = (alpha - b.x0) / b.img_dx, qy = (beta - b.y0) / b.img_dy;
    if (!(qx > -1 && qx < b.img_nx && qy > -1 && qy < b.img_ny)) return -1;
    const int ix = (int) qx;
    const int iy = b.flip_image ? b.img_ny - (int) qy - 1 : (int) qy;
    return (long long) ix * b.img_ny + iy;
}

// d_stokes layout: [nrays | I | Q | U](npix each) + disc_count, bad_pol, doubles
__global__ void __launch_bounds__(kBlock)
post_image_stokes_kernel(kr_ray_f64* __restrict__ rays, long long n, double spin, double V, int reverse, int projradius, double lo, double hi, double sin_incl,
                         kr_image_bins b, kr_limb_law limb, kr_pol_law pol, double* __restrict__ planes)
{
    const long long npix = (long long) b.img_nx * b.img_ny;
    unsigned long long hits = 0, bad_pol = 0;
    KR_GRID_STRIDE(i, n) {
        kr_ray_f64* ray = &rays[i];
        const kr_ray_f64 v = polar_record_of(ray);
        const int steps = ray->steps;
        const Polar q = polar_value(v, spin, V, reverse, projradius, sin_incl);
        const double g = q.redshift;
        ray->redshift = g;
        wrap_phi(ray, steps, lo, hi);
        const long long px = stokes_pixel(b, steps, v.r, v.theta, g, v.alpha, v.beta);
        if (px < 0) continue;
        hits++;
        if (q.bad) { bad_pol++; continue; }
        const double w = powerlaw3(v.r, b.q1, b.rb1, b.q2, b.rb2, b.q3) * limb_weight(limb.law, limb.coeff, q.mu) / kr_pow(g, 3.0);
        const double wd = w * pol_degree(pol.law, pol.coeff, q.mu);
        atomicAdd(&planes[px], 1.0);
        atomicAdd(&planes[npix + px], w);
        atomicAdd(&planes[2 * npix + px], wd * q.c2);
        atomicAdd(&planes[3 * npix + px], wd * q.s2);
    }
    if (hits) atomicAdd(&planes[4 * npix], (double) hits);
    if (bad_pol) atomicAdd(&planes[4 * npix + 1], (double) bad_pol);
}

}  // namespace

int polarisation_validate(int reverse, int motion, double inc_deg, const char* who)
{
    auto bad = [&](const char* why) { set_error(std::string(who) + ": " + why); return KR_EINVAL; };
    if (reverse != 1) return bad("reverse must be 1 (the rule is stated for image-plane records)");
    if (motion != 0) return bad("motion must be 0 (the orbiting observer)");
    if (!std::isfinite(inc_deg)) return bad("non-finite inclination");
    return KR_OK;
}

int pol_validate(const kr_pol_law* law, const char* who)
{
    auto bad = [&](const char* why) { set_error(std::string(who) + ": " + why); return KR_EINVAL; };
    if (!law) return bad("null pol law");
    if (law->law < 0 || law->law > 1) return bad("pol law must be 0 (constant) or 1 (coeff (1 - mu) / (1 + 3.582 mu))");
    if (!std::isfinite(law->coeff)) return bad("non-finite pol coefficient");
    if (!(std::fabs(law->coeff) <= 1)) return bad("pol coefficient must lie in [-1, 1]");
    return KR_OK;
}

// sin of the inclination with the host's C library at the image plane's own argument (plane_trig, kr_post.hip)
double sin_inclination(double inc_deg) { return std::sin(inc_deg * M_PI / 180); }

int polarisation_dev(double spin, double V, int reverse, int projradius, double inc_deg, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    hipLaunchKernelGGL(polarisation_kernel, dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, (const kr_ray_f64*) d, (long long) n, spin, V, reverse, projradius,
                       sin_inclination(inc_deg), (double*) d_out);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int post_image_stokes_dev(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_image_bins* b, const kr_limb_law* limb,
                          const kr_pol_law* pol, void* d, int64_t n, void* d_stokes, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    hipLaunchKernelGGL(post_image_stokes_kernel, dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, spin, V, reverse, projradius, lo,
                       hi, sin_inclination(inc_deg), *b, *limb, *pol, (double*) d_stokes);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace kr
