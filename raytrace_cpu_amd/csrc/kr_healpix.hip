// kr_healpix.hip -- the HEALPix point source (kr_healpix_source, include/kr_trace.h) and the fate map of its sky (kr_healpix_map): the reference's
// HealpixPointSource ctor (healpix_pointsource.cpp:11-172 over healpix.h's pixel geometry) with the radially moving emitter it folds into
// calc_consts_from_vector(..., motion = 1), and the per-pixel classification of healpix_to_disc.cpp:60-84 / healpix_disc_source_photonfrac.cpp:84-108.
// Streaming kernels beside the trace: the source writes 144-B records, ONE WORK-ITEM PER PIXEL, which computes the four corners once and writes the
// pixel's one or five records (720 B between lanes at five).  The coalesced layout, one work-item per record with the centre lane recomputing the
// four corners, measured the same at one ray per pixel and 1.5 x slower at five (profiles/healpix_ab.txt): the kernel is bound by its 256 registers
// and dependent fp64 chains, two waves per SIMD, not by its stores, and in that layout the corner lanes of every wave wait for every fifth lane's
// four corners.  The fate pass reads the centre records, writes seven planes at the pixel
// and adds six tallies: wave shuffle -> LDS -> one global atomic per word and workgroup, as in kr_return_map.hip.
// Arithmetic: sin / cos of the pixel's azimuth and atan2 are the correctly rounded routines of kr_sincos.hpp / kr_crmath.hpp, sin / cos / tan of the
// source's polar angle come from the host's C library (three scalars), everything else is a single IEEE operation under -ffp-contract=off, in the
// reference's own association -- tests/healpix_rules.py restates the same rules in numpy and the device records must equal it bit for bit.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "kr_pass.hpp"
#include "kr_crmath.hpp"
#include "kr_healpix_geom.hpp"

namespace kr {

namespace {

constexpr int kFateScalars = 6;                  // live, disc, escape, lost, self, 0
constexpr int kMaxOrder = 13;                    // 2 pix still fits the reference's int

struct SourceTrig { double sin_th, cos_th, tan_th; };   // of pos[2], from the host's C library

// the pixel geometry is kr_healpix_geom.hpp's, shared with the host class mirror; here with the strict trace's correctly rounded sin / cos pair
struct DeviceMath {
    static KR_DEV void sincos(double x, double& s, double& c) { kr_sincos_f64(x, s, c); }
};

// ---- the record of one direction: calc_consts_from_vector (healpix_pointsource.cpp:11-109) and the ctor's fields (:139-168) ----------------------
// The record of UNIT photon energy, which is what the reference's class builds (it passes E = 1), and in p[] the photon's momentum as the tetrad
// launched it, (tdot, rdot, thetadot, phidot).  healpix_record scales it to the spec's E.
KR_DEV kr_ray_f64 healpix_unit_ray(const kr_healpix_source& s, const SourceTrig& tg, const double* vec, double* p)
{
    kr_ray_f64 ray;
    memset(&ray, 0, sizeof(ray));
    ray.t = s.pos[0]; ray.r = s.pos[1]; ray.theta = s.pos[2]; ray.phi = s.pos[3];
    ray.steps = 0;
    ray.alpha = vec[2];
    ray.beta = krcr::kr_atan2_cr(vec[1], vec[0]);

    const double a = s.spin, V = s.V, E = 1, r = ray.r;
    const double st = tg.sin_th, ct = tg.cos_th, tt = tg.tan_th;
    const double rhosq = r * r + (a * ct) * (a * ct);
    const double delta = r * r - 2 * r + a * a;
    const double sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st;
    const double e2nu = rhosq * delta / sigmasq;
    const double e2psi = sigmasq * st * st / rhosq;
    const double omega = 2 * a * r / sigmasq;
    const double g00 = e2nu - omega * omega * e2psi;
    const double g03 = omega * e2psi;
    const double g11 = -rhosq / delta;
    const double g33 = -e2psi;

    const double rp0 = E, rp1 = E * vec[0], rp2 = E * vec[1], rp3 = E * vec[2];
    double tdot, rdot, thetadot, phidot;
    if (s.motion == 0) {
        const double et0 = (1 / kr_sqrt(e2nu)) / kr_sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
        const double et3 = (1 / kr_sqrt(e2nu)) * V / kr_sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
        const double e10 = (V - omega) * kr_sqrt(e2psi / e2nu) / kr_sqrt(e2nu - (V - omega) * (V - omega) * e2psi);
        const double e13 = (1 / kr_sqrt(e2nu * e2psi)) * (e2nu + V * omega * e2psi - omega * omega * e2psi) / kr_sqrt(e2nu - (V - omega) * (V - omega) * e2psi);
        tdot = rp0 * et0 + rp1 * e10;
        phidot = rp0 * et3 + rp1 * e13;
        if (s.basis == 0) {
            const double e22 = -1 / kr_sqrt(rhosq);
            const double e31 = kr_sqrt(delta / rhosq);
            rdot = rp3 * e31;
            thetadot = rp2 * e22;
        } else {
            const double e32 = -1 / kr_sqrt(rhosq);
            const double e21 = -1 * kr_sqrt(delta / rhosq);
            rdot = rp2 * e21;
            thetadot = rp3 * e32;
        }
    } else {
        const double et0 = 1 / kr_sqrt(g00 + g11 * V * V);
        const double et1 = V * et0;
        const double e12 = 1 / kr_sqrt(rhosq);
        const double e23 = kr_sqrt(g00 / (g03 * g03 - g00 * g33));
        const double e20 = -(g03 / g00) * e23;
        const double e30 = kr_sqrt(-g11 / g00) * V / kr_sqrt(g00 + g11 * V * V);
        const double e31 = kr_sqrt(-g00 / g11) / kr_sqrt(g00 + g11 * V * V);
        tdot = rp0 * et0 + rp1 * e20 + rp3 * e30;
        phidot = rp1 * e23;
        rdot = rp0 * et1 + rp3 * e31;
        thetadot = rp2 * e12;
    }

    const double k = (1 - 2 * r / rhosq) * tdot + (2 * a * r * st * st / rhosq) * phidot;
    double h = phidot * ((r * r + a * a) * (r * r + a * a * ct * ct - 2 * r) * st * st + 2 * a * a * r * st * st * st * st);
    h = h - 2 * a * r * k * st * st;
    h = h / (r * r + a * a * ct * ct - 2 * r);
    ray.k = k;
    ray.h = h;
    ray.Q = rhosq * rhosq * thetadot * thetadot - (a * k * ct + h / tt) * (a * k * ct - h / tt);
    ray.rdot_sign = (rdot > 0) ? 1 : -1;          // strict, unlike PointSource (:107)
    ray.thetadot_sign = (thetadot > 0) ? 1 : -1;
    p[0] = tdot; p[1] = rdot; p[2] = thetadot; p[3] = phidot;
    return ray;
}

// redshift_start in the frame of a source moving radially at dr/dt = V: emit_value's body (kr_post_device.hpp) with u = (u_t, V u_t, 0, 0),
// u_t = 1 / sqrt(g00 + g11 V V) as redshift_value's motion 1 forms it, and with the momentum the tetrad LAUNCHED the photon with in place of
// momentum()'s reconstruction from k, h, Q.  The reconstruction takes p^r from the null condition, and the reference's un-normalised centre
// vector is not null (1 - |v|^2 ~ 1e-2 at order 3); an orbiting emitter never reads p^r, this one does.  p . u of the launched momentum is E.
KR_DEV double emit_value_radial(const kr_ray_f64& ray, const double* launched, double a, double V, int reverse)
{
    const Metric<double> m = kerr_metric<double>(ray.r, ray.theta, a);
    double et[4] = {0, 0, 0, 0};
    et[0] = 1. / kr_sqrt(m.g00 + m.g11 * V * V);
    et[1] = V * et[0];
    double p[4] = {launched[0], launched[1], launched[2], launched[3]};
    if (reverse) { p[1] *= -1; p[2] *= -1; p[3] *= -1; }
    return energy_dot<double>(m, et, p);
}

// The record at the spec's energy: k, h and emit of the unit record times E, Q times E E -- exact at E = 1, the reference's only value, and
// exactly homogeneous in E otherwise (carrying E through calc_consts_from_vector's sums instead leaves h and Q hundreds of ulp from 2.5 x and
// 6.25 x their unit values where their terms cancel)
KR_DEV kr_ray_f64 healpix_record(const kr_healpix_source& s, const SourceTrig& tg, const double* vec, bool emit, int reverse)
{
    double launched[4];
    kr_ray_f64 ray = healpix_unit_ray(s, tg, vec, launched);
    if (emit) {
        const double a = reverse ? -1 * s.spin : s.spin;
        ray.emit = s.E * (s.motion == 0 ? emit_value(ray, s.spin, a, s.V, reverse) : emit_value_radial(ray, launched, a, s.V, reverse));
    }
    ray.k = s.E * ray.k;
    ray.h = s.E * ray.h;
    ray.Q = (s.E * s.E) * ray.Q;
    if (s.disc_source && ray.thetadot_sign > 0) ray.steps = -1;      // set_disc_source(), healpix_pointsource.h:39-43
    return ray;
}

__global__ void __launch_bounds__(kBlock)
healpix_vectors_kernel(double* __restrict__ out, long long count, int order, int unit_center, long long first, long long stride)
{
    KR_GRID_STRIDE(k, count) {
        double v[15];
        krhpx::pixel_vectors<DeviceMath, double>(order, (int) (first + k * stride), unit_center, v);
#pragma unroll
        for (int w = 0; w < 15; w++) out[k * 15 + w] = v[w];
    }
}

// one work-item per PIXEL, which writes the pixel's one or five records
template <bool EMIT>
__global__ void __launch_bounds__(kBlock)
healpix_init_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_healpix_source s, SourceTrig tg, long long first, long long stride, int reverse)
{
    const int rpp = s.rays_per_pixel;
    const long long pixels = (n + rpp - 1) / rpp;
    KR_GRID_STRIDE(k, pixels) {
        double v[15];
        krhpx::pixel_vectors<DeviceMath, double>(s.order, (int) (first + k * stride), s.unit_center, v);
        for (int i = (rpp == 1 ? 4 : 0); i < 5; i++) {
            const long long slot = rpp == 1 ? k : 5 * k + i;
            if (slot < n) rays[slot] = healpix_record(s, tg, &v[3 * i], EMIT, reverse);
        }
    }
}

// ---- the fate pass ---------------------------------------------------------------------------------------------------------------------------------
// out = [class | r | theta | phi | g | t | emis](npix each) + the six tallies; pixels: centre records in this shard
template <bool FUSED>
__global__ void __launch_bounds__(kBlock)
healpix_map_kernel(kr_ray_f64* __restrict__ rays, long long pixels, kr_healpix_map m, long long first, long long stride, double* __restrict__ out, double spin,
                   double V, int reverse, int projradius, int motion, double lo, double hi)
{
    __shared__ double part[kBlock / 64][kFateScalars];
    const long long npix = m.npix;
    const double theta_min = kPi2 - m.theta_tol;
    double acc[kFateScalars] = {0, 0, 0, 0, 0, 0};
    KR_GRID_STRIDE(k, pixels) {
        kr_ray_f64* ray = &rays[m.rays_per_pixel == 1 ? k : 5 * k + 4];
        const long long pix = first + k * stride;
        const int steps = ray->steps;
        const double r = ray->r, theta = ray->theta;
        double phi, g;
        if (FUSED) {
            const kr_ray_f64 v = geodesic_of(ray);
            phi = wrap_phi(ray, steps, lo, hi);
            g = redshift_value(v, spin, V, reverse, projradius, motion);
            ray->redshift = g;
        } else {
            phi = ray->phi;
            g = ray->redshift;
        }
        int cls = 0;
        if (steps > 0) {
            acc[0] += 1;
            if (theta >= theta_min && r >= m.r_isco && r < m.r_disc) {
                cls = (m.self_zone && kr_abs(r - m.source_r) <= 0.1 * m.source_r && kr_abs(phi - m.source_phi) <= 0.1) ? 4 : 1;
            } else if (r > m.r_esc) {
                cls = 2;
            } else {
                cls = 3;
            }
            acc[1] += cls == 1; acc[2] += cls == 2; acc[3] += cls == 3; acc[4] += cls == 4;
        }
        out[pix] = (double) cls;
        out[npix + pix] = r;
        out[2 * npix + pix] = theta;
        out[3 * npix + pix] = phi;
        out[4 * npix + pix] = g;
        out[5 * npix + pix] = ray->t;
        out[6 * npix + pix] = cls == 1 ? powerlaw3(r, m.q1, m.rb1, m.q2, m.rb2, m.q3) / kr_pow(g, 3.0) : 0.0;
    }
#pragma unroll
    for (int q = 0; q < kFateScalars; q++) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < kFateScalars) {
        double v = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) v += part[w][threadIdx.x];
        if (v != 0) atomicAdd(&out[7 * npix + threadIdx.x], v);
    }
}

SourceTrig source_trig(const kr_healpix_source* s) { return SourceTrig{std::sin(s->pos[2]), std::cos(s->pos[2]), std::tan(s->pos[2])}; }

int64_t sphere_pixels(int order) { return 12LL << (2 * order); }

// the pixels a shard of `records` records covers must lie on the sphere
int shard_check(const char* who, int64_t first, int64_t stride, int64_t records, int rpp, int64_t npix)
{
    if (first < 0 || stride < 1) return invalid_arg(who, "bad first/stride");
    if (records < 0) return invalid_arg(who, "negative count");
    if (records > 0) {
        const int64_t last = (records - 1) / rpp;
        if (first >= npix || last > (npix - 1 - first) / stride) return invalid_arg(who, "the shard's last pixel lies beyond the sphere");
    }
    return KR_OK;
}

}  // namespace

int healpix_validate(const kr_healpix_source* s, const char* who)
{
    if (!s) return invalid_arg(who, "null spec");
    if (const int rc = refuse_plunge(s->V, who)) return rc;
    if (s->order < 0 || s->order > kMaxOrder) return invalid_arg(who, "order must be 0 ... 13");
    if (s->motion != 0 && s->motion != 1) return invalid_arg(who, "motion must be 0 (orbital) or 1 (radial)");
    if (s->basis != 0 && s->basis != 1) return invalid_arg(who, "basis must be 0 or 1");
    if (s->rays_per_pixel != 1 && s->rays_per_pixel != 5) return invalid_arg(who, "rays_per_pixel must be 1 or 5");
    if (s->basis == 1 && s->motion == 1) return invalid_arg(who, "basis 1 exists for motion 0 only");
    if (!(s->E > 0)) return invalid_arg(who, "E must be positive");
    if (s->disc_source != 0 && s->disc_source != 1) return invalid_arg(who, "disc_source must be 0 or 1");
    // the metric at pos with the C library, as calc_consts_from_vector forms it
    const double r = s->pos[1], a = s->spin, V = s->V, st = std::sin(s->pos[2]), ct = std::cos(s->pos[2]);
    const double rhosq = r * r + (a * ct) * (a * ct);
    const double delta = r * r - 2 * r + a * a;
    const double sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st;
    const double e2nu = rhosq * delta / sigmasq;
    const double e2psi = sigmasq * st * st / rhosq;
    const double omega = 2 * a * r / sigmasq;
    if (s->motion == 0) {
        if (!(1 - (V - omega) * (V - omega) * e2psi / e2nu > 0)) return invalid_arg(who, "V is not the angular velocity of a timelike orbit at pos (1 - (V - omega)^2 e2psi / e2nu <= 0)");
    } else {
        const double g00 = e2nu - omega * omega * e2psi, g11 = -rhosq / delta;
        if (!(g00 + g11 * V * V > 0)) return invalid_arg(who, "V is not a timelike radial velocity at pos (g00 + g11 V^2 <= 0)");
    }
    return KR_OK;
}

int healpix_map_validate(const kr_healpix_map* m, int64_t n, int64_t first, int64_t stride, const char* who)
{
    if (!m) return invalid_arg(who, "null map");
    if (m->npix <= 0) return invalid_arg(who, "npix must be positive");
    if (m->rays_per_pixel != 1 && m->rays_per_pixel != 5) return invalid_arg(who, "rays_per_pixel must be 1 or 5");
    if (n < 0) return invalid_arg(who, "negative n");
    if (n % m->rays_per_pixel != 0) return invalid_arg(who, "n is no multiple of rays_per_pixel");
    return shard_check(who, first, stride, n, m->rays_per_pixel, m->npix);
}

int healpix_vectors_validate(int order, int64_t first, int64_t stride, int64_t count, const char* who)
{
    if (order < 0 || order > kMaxOrder) return invalid_arg(who, "order must be 0 ... 13");
    return shard_check(who, first, stride, count, 1, sphere_pixels(order));
}

int healpix_shard_validate(const kr_healpix_source* s, int64_t first, int64_t stride, int64_t count, const char* who)
{
    const int rc = healpix_validate(s, who);
    return rc != KR_OK ? rc : shard_check(who, first, stride, count, s->rays_per_pixel, sphere_pixels(s->order));
}

int healpix_vectors_dev(int order, int unit_center, int64_t first, int64_t stride, int64_t count, void* d_out, hipStream_t st)
{
    if (count <= 0) return KR_OK;
    hipLaunchKernelGGL(healpix_vectors_kernel, dim3(grid_for(count, kBlock, kCapStream)), dim3(kBlock), 0, st, (double*) d_out, (long long) count, order, unit_center,
                       (long long) first, (long long) stride);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int healpix_init_dev(const kr_healpix_source* s, void* d, int64_t n, int64_t first, int64_t stride, bool emit, int reverse, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    const SourceTrig tg = source_trig(s);
    const int64_t items = (n + s->rays_per_pixel - 1) / s->rays_per_pixel;
    const int grid = grid_for(items, kBlock, kCapStream);
    if (emit)
        hipLaunchKernelGGL(healpix_init_kernel<true>, dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *s, tg, (long long) first, (long long) stride, reverse);
    else
        hipLaunchKernelGGL(healpix_init_kernel<false>, dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *s, tg, (long long) first, (long long) stride, 0);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int reduce_healpix_map_dev(const kr_healpix_map* m, const void* d, int64_t n, int64_t first, int64_t stride, void* d_out, hipStream_t st)
{
    const int64_t pixels = n / m->rays_per_pixel;
    if (pixels <= 0) return KR_OK;
    hipLaunchKernelGGL(healpix_map_kernel<false>, dim3(grid_for(pixels, kBlock, kCapHist)), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) pixels, *m, (long long) first,
                       (long long) stride, (double*) d_out, 0.0, 0.0, 0, 0, 0, 0.0, 0.0);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int post_healpix_map_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_healpix_map* m, void* d, int64_t n, int64_t first,
                         int64_t stride, void* d_out, hipStream_t st)
{
    const int64_t pixels = n / m->rays_per_pixel;
    if (pixels <= 0) return KR_OK;
    hipLaunchKernelGGL(healpix_map_kernel<true>, dim3(grid_for(pixels, kBlock, kCapHist)), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) pixels, *m, (long long) first,
                       (long long) stride, (double*) d_out, spin, V, reverse, projradius, motion, lo, hi);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace kr
