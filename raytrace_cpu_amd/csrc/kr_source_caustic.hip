// kr_source_caustic.hip -- caustic maps of the source sphere and of a flat source plane behind the hole (include/kr_trace.h, kr_source_map): the
// reference's src/caustic/caustic_sourceplane.cpp and src/caustic/caustic_plane.cpp with the rays where they already are, in HBM.  Both programs
// gather and difference rays[] on one core; here
//   source_gather_kernel        grid mode, either kind: the six per-pixel planes and the three counts      caustic_sourceplane.cpp:180-232, caustic_plane.cpp:315-349
//   plane_bundle_kernel         plane kind, 5-ray bundles: the same from the centre rays + the Jacobian     caustic_plane.cpp:207-241, :249-299
//                               from the four satellites
//   source_jacobian_kernel      grid-neighbour Jacobian of either kind; the sphere wraps its phi differences  caustic_sourceplane.cpp:264-305, caustic_plane.cpp:357-392
// Streaming passes laid out as kr_caustic.hip's: one 144-byte record per work-item (adjacent lanes read adjacent records), the five end points of a
// bundle meet in LDS, one array per member, and the lanes that own a pixel write the planes at consecutive addresses.  The records are only read.
// There is no suppression pass: these two programs have none.  DESIGN.md 4.2.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "kr_pass.hpp"

namespace kr {

namespace {

constexpr int kBundle = 5;                 // ImagePlaneBundles::RAYS_PER_BUNDLE: centre, east, west, north, south
constexpr double kSentinel = 1e30;         // caustic_sourceplane.cpp:259, caustic_plane.cpp:161
constexpr int kPlanes = 8, kCounts = 3;
enum Plane { P_DET = 0, P_SIGN, P_ORDER, P_HIT, P_U, P_V, P_FLIPS, P_EQUAT };      // (U, V) = (THETA_S, PHI_S) or (X_S, Y_S)
enum Count { C_HIT = 0, C_CAPTURED, C_STEPLIM };
enum Kind { K_SPHERE = 0, K_PLANE = 1 };

// what one record contributes: to its own pixel when it is the ray through the pixel, to the Jacobian when it is a satellite
struct EndPoint {
    double phi, u, v;
    int hit, flips;
};

// the sphere at r_lim (caustic_sourceplane.cpp:191-219): escaped = steps > 0 && RLIM, THETA_S = theta, PHI_S = atan2(sin, cos) of the ACCUMULATED phi
// (thousands of pi on rays that wind round the axis: kr_sincos_f64 hands |phi| >= 1024 to the library's full argument reduction),
// ORDER = max(floor(|phi| / pi) - 1, 0)
KR_DEV EndPoint sphere_end(const kr_ray_f64* ray, int& order)
{
    const double phi = ray->phi;
    EndPoint e = {phi, 0, 0, (ray->steps > 0 && (ray->status & KR_STATUS_RLIM)) ? 1 : 0, ray->rdot_flips};
    order = -1;
    if (e.hit) {
        double sp, cp;
        kr_sincos_f64(phi, sp, cp);
        e.u = ray->theta;
        e.v = krcr::kr_atan2_cr(sp, cp);
        const int phi_order = (int) floor(kr_abs(phi) / kPi);
        order = phi_order > 0 ? phi_order - 1 : 0;
    }
    return e;
}

// the flat plane (caustic_plane.cpp:180-189, ray_destination.h:151-160): valid_hit = steps > 0 && DEST, (X_S, Y_S) = source_coords(r, theta, phi) in
// the reference's association, ORDER = max((int) (|phi| / 2 pi), rdot_flips / 2)
KR_DEV EndPoint plane_end(const kr_ray_f64* ray, const kr_source_map& m, int& order)
{
    const double r = ray->r, theta = ray->theta, phi = ray->phi;
    EndPoint e = {phi, 0, 0, (ray->steps > 0 && (ray->status & KR_STATUS_DEST)) ? 1 : 0, ray->rdot_flips};
    order = -1;
    if (e.hit) {
        double st, ct, sp, cp;
        kr_sincos_f64(theta, st, ct);
        kr_sincos_f64(phi, sp, cp);
        const double X = r * st * cp;
        const double Y = r * st * sp;
        const double Z = r * ct;
        e.u = -X * m.sin_phi0 + Y * m.cos_phi0;
        e.v = -X * m.cos_incl * m.cos_phi0 - Y * m.cos_incl * m.sin_phi0 + Z * m.sin_incl;
        const int phi_ord = (int) (kr_abs(phi) / (2 * kPi));
        const int r_ord = e.flips / 2;
        order = phi_ord > r_ord ? phi_ord : r_ord;
    }
    return e;
}

// the six planes and the three counts of the ray through pixel px (caustic_sourceplane.cpp:187-231, caustic_plane.cpp:213-239)
KR_DEV void write_pixel(double* __restrict__ maps, long long npix, long long px, const EndPoint& e, int order, int steps, int status, int equat, unsigned* cnt)
{
    const bool hit = e.hit != 0;
    if (hit) cnt[C_HIT]++;
    else if (status & KR_STATUS_HORIZON) cnt[C_CAPTURED]++;
    if (steps <= 0 || (status & KR_STATUS_STEPLIM)) cnt[C_STEPLIM]++;
    maps[P_ORDER * npix + px] = (double) order;
    maps[P_HIT * npix + px] = hit ? 1.0 : 0.0;
    maps[P_U * npix + px] = hit ? e.u : __builtin_nan("");
    maps[P_V * npix + px] = hit ? e.v : __builtin_nan("");
    maps[P_FLIPS * npix + px] = (double) e.flips;
    maps[P_EQUAT * npix + px] = (double) equat;
}

// the three counters: wave shuffle -> workgroup (LDS) -> one atomic per non-zero word and workgroup.  Every work-item of the workgroup calls this.
template <int WAVES>
KR_DEV void flush_counts(unsigned* cnt, unsigned (*part)[kCounts], double* __restrict__ counts)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCounts; k++) {
        unsigned v = cnt[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((t & 63) == 0) part[t >> 6][k] = v;
    }
    __syncthreads();
    if (t < kCounts) {
        unsigned v = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) v += part[w][t];
        if (v) atomicAdd(&counts[t], (double) v);
    }
}

// ---- grid mode: record px is the ray through pixel px = ix ny + iy (ImagePlane's order) ------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(kBlock)
source_gather_kernel(const kr_ray_f64* __restrict__ rays, kr_source_map m, double* __restrict__ maps)
{
    __shared__ unsigned part[kBlock / 64][kCounts];
    const long long npix = (long long) m.nx * m.ny;
    unsigned cnt[kCounts] = {0, 0, 0};
    KR_GRID_STRIDE(px, npix) {
        const kr_ray_f64* ray = &rays[px];
        int order;
        const EndPoint e = KIND == K_SPHERE ? sphere_end(ray, order) : plane_end(ray, m, order);
        write_pixel(maps, npix, px, e, order, ray->steps, ray->status, ray->equatorial_crossings, cnt);
    }
    flush_counts<kBlock / 64>(cnt, part, maps + kPlanes * npix);
}

// ---- plane kind, bundles: record 5 px + k is member k of the bundle of pixel px; BPB pixels per workgroup pass -------------------------------
// ... one array per member in LDS: the gather reads members 5 t + k of lane t, 40 bytes apart as doubles (a 2-way bank conflict) instead of 160 as records (8-way)
template <int N>
struct EndPoints {
    double phi[N], u[N], v[N];
    int hit[N], flips[N];
    KR_DEV void put(int i, const EndPoint& e) { phi[i] = e.phi; u[i] = e.u; v[i] = e.v; hit[i] = e.hit; flips[i] = e.flips; }
    KR_DEV EndPoint get(int i) const { return EndPoint{phi[i], u[i], v[i], hit[i], flips[i]}; }
};
struct Centre {
    int order, steps, status, equat;
};

template <int BPB>
__global__ void __launch_bounds__(kBundle * BPB)
plane_bundle_kernel(const kr_ray_f64* __restrict__ rays, kr_source_map m, double* __restrict__ maps)
{
    constexpr int kThreads = kBundle * BPB;
    constexpr int kWaves = (kThreads + 63) / 64;
    __shared__ EndPoints<kThreads> ends;
    __shared__ Centre centres[BPB];
    __shared__ unsigned part[kWaves][kCounts];
    const long long npix = (long long) m.nx * m.ny;
    const long long n = kBundle * npix;                                            // records from here on are not pixels
    const long long chunks = (n + kThreads - 1) / kThreads;
    const int t = threadIdx.x;
    unsigned cnt[kCounts] = {0, 0, 0};
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {       // uniform per workgroup: the barriers below are safe
        const long long i = chunk * kThreads + t;
        if (i < n) {
            const kr_ray_f64* ray = &rays[i];
            int order;
            ends.put(t, plane_end(ray, m, order));
            if (t % kBundle == 0) centres[t / kBundle] = Centre{order, ray->steps, ray->status, ray->equatorial_crossings};
        }
        __syncthreads();
        const long long px = chunk * BPB + t;
        if (t < BPB && px < npix) {
            const Centre c = centres[t];
            const EndPoint ec = ends.get(t * kBundle);
            write_pixel(maps, npix, px, ec, c.order, c.steps, c.status, c.equat, cnt);
            // Jacobian from the satellites, caustic_plane.cpp:249-299
            double det = __builtin_nan(""), sign = 0;
            const EndPoint ee = ends.get(t * kBundle + 1), ew = ends.get(t * kBundle + 2), en = ends.get(t * kBundle + 3), es = ends.get(t * kBundle + 4);
            if (ec.hit && ee.hit && ew.hit && en.hit && es.hit) {
                const bool order_match = ee.flips == ec.flips && ew.flips == ec.flips && en.flips == ec.flips && es.flips == ec.flips &&
                                         kr_abs(ee.phi - ec.phi) < kPi2 && kr_abs(ew.phi - ec.phi) < kPi2 && kr_abs(en.phi - ec.phi) < kPi2 &&
                                         kr_abs(es.phi - ec.phi) < kPi2;
                if (!order_match) {
                    det = kSentinel;
                } else {
                    const double dxs_da = (ee.u - ew.u) / (2 * m.eps_x);
                    const double dxs_db = (en.u - es.u) / (2 * m.eps_y);
                    const double dys_da = (ee.v - ew.v) / (2 * m.eps_x);
                    const double dys_db = (en.v - es.v) / (2 * m.eps_y);
                    det = dxs_da * dys_db - dxs_db * dys_da;
                    sign = (det > 0) ? 1.0 : (det < 0) ? -1.0 : 0.0;
                }
            }
            maps[P_DET * npix + px] = det;
            maps[P_SIGN * npix + px] = sign;
        }
        __syncthreads();
    }
    flush_counts<kWaves>(cnt, part, maps + kPlanes * npix);
}

// ---- grid-neighbour Jacobian: one pixel per work-item over the HIT / ORDER / U / V planes.  The sphere's V is an angle in [-pi, pi]: its differences
//      are wrapped back into that range as wrap_dphi does (caustic_sourceplane.cpp:68-73; |d| <= 2 pi, so each of its loops runs at most once) -------
template <int KIND>
KR_DEV double wrapped(double d)
{
    if (KIND == K_SPHERE) {
        if (d > kPi) d -= 2 * kPi;
        if (d < -kPi) d += 2 * kPi;
    }
    return d;
}

template <int KIND>
__global__ void __launch_bounds__(kBlock)
source_jacobian_kernel(kr_source_map m, double* __restrict__ maps)
{
    const int nx = m.nx, ny = m.ny;
    const long long npix = (long long) nx * ny;
    const double* hit = maps + P_HIT * npix;
    const double* order = maps + P_ORDER * npix;
    const double* u = maps + P_U * npix;
    const double* v = maps + P_V * npix;
    KR_GRID_STRIDE(px, npix) {
        const int ix = (int) (px / ny), iy = (int) (px % ny);
        double det = __builtin_nan(""), sign = 0;
        if (hit[px] != 0 && !(ix == 0 || ix == nx - 1 || iy == 0 || iy == ny - 1)) {
            const long long e = px + ny, w = px - ny, nn = px + 1, s = px - 1;      // [ix + 1][iy], [ix - 1][iy], [ix][iy + 1], [ix][iy - 1]
            if (hit[e] != 0 && hit[w] != 0 && hit[nn] != 0 && hit[s] != 0) {
                const double ord = order[px];
                if (!(order[e] == ord && order[w] == ord && order[nn] == ord && order[s] == ord)) {
                    det = kSentinel;
                } else {
                    const double du_dx = (u[e] - u[w]) / (2 * m.eps_x);
                    const double du_dy = (u[nn] - u[s]) / (2 * m.eps_y);
                    const double dv_dx = wrapped<KIND>(v[e] - v[w]) / (2 * m.eps_x);
                    const double dv_dy = wrapped<KIND>(v[nn] - v[s]) / (2 * m.eps_y);
                    det = du_dx * dv_dy - du_dy * dv_dx;
                    sign = (det > 0) ? 1.0 : (det < 0) ? -1.0 : 0.0;
                }
            }
        }
        maps[P_DET * npix + px] = det;
        maps[P_SIGN * npix + px] = sign;
    }
}

}  // namespace

int source_map_validate(const kr_source_map* m, int64_t n, const char* who)
{
    auto bad = [&](const char* why) { set_error(std::string(who) + ": " + why); return KR_EINVAL; };
    if (!m) return bad("null map description");
    if (m->nx < 1 || m->ny < 1) return bad("nx and ny must be >= 1");
    if (!std::isfinite(m->eps_x) || !std::isfinite(m->eps_y) || !(m->eps_x > 0) || !(m->eps_y > 0)) return bad("eps_x and eps_y must be positive and finite");
    if (m->kind != K_SPHERE && m->kind != K_PLANE) return bad("unknown kind (0: source sphere, 1: flat source plane)");
    if (m->kind == K_SPHERE && m->bundles) return bad("the source sphere has no bundle mode");
    if (m->kind == K_PLANE && !(std::isfinite(m->sin_incl) && std::isfinite(m->cos_incl) && std::isfinite(m->sin_phi0) && std::isfinite(m->cos_phi0)))
        return bad("non-finite sine or cosine of incl / phi0");
    if (n < (m->bundles ? kBundle : 1) * (int64_t) m->nx * m->ny) return bad(m->bundles ? "n smaller than 5 nx ny" : "n smaller than nx ny");
    return KR_OK;
}

int post_caustic_source_dev(const kr_source_map* m, const void* d, void* d_maps, hipStream_t st)
{
    const long long npix = (long long) m->nx * m->ny;
    const kr_ray_f64* rays = (const kr_ray_f64*) d;
    double* maps = (double*) d_maps;
    KR_HIP(hipMemsetAsync(maps + kPlanes * npix, 0, kCounts * sizeof(double), st));
    if (m->bundles) {
        constexpr int kPixels = 64;                 // 320 work-items: five waves, one pixel per lane of the first in the gather
        hipLaunchKernelGGL((plane_bundle_kernel<kPixels>), dim3(grid_for(kBundle * npix, kBundle * kPixels, kCapStream)), dim3(kBundle * kPixels), 0, st, rays, *m, maps);
        KR_LAUNCH_CHECK();
        return KR_OK;
    }
    const int grid = grid_for(npix, kBlock, kCapStream);
    if (m->kind == K_SPHERE) {
        hipLaunchKernelGGL((source_gather_kernel<K_SPHERE>), dim3(grid), dim3(kBlock), 0, st, rays, *m, maps);
        KR_LAUNCH_CHECK();
        hipLaunchKernelGGL((source_jacobian_kernel<K_SPHERE>), dim3(grid), dim3(kBlock), 0, st, *m, maps);
    } else {
        hipLaunchKernelGGL((source_gather_kernel<K_PLANE>), dim3(grid), dim3(kBlock), 0, st, rays, *m, maps);
        KR_LAUNCH_CHECK();
        hipLaunchKernelGGL((source_jacobian_kernel<K_PLANE>), dim3(grid), dim3(kBlock), 0, st, *m, maps);
    }
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace kr
