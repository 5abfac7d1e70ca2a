// kr_caustic.hip -- critical-curve (caustic) maps of the lens map image plane -> a surface, per image-plane pixel (include/kr_trace.h): of the disc
// (kr_caustic_map; the reference's src/caustic/caustic_discplane.cpp), of the source sphere and of a flat source plane behind the hole (kr_source_map;
// src/caustic/caustic_sourceplane.cpp, src/caustic/caustic_plane.cpp), with the rays where they already are, in HBM.  The reference builds the 5-ray
// bundles in a serial host loop (imageplane_bundles.h:150-199), and gathers, differences and filters rays[] on one core; here
//   bundles_init_emit_kernel   ImagePlaneBundles ctor + redshift_start(0, reverse = true)                 imageplane_bundles.h:150-199, raytracer.cpp:342-417
//   bundle_gather_kernel       5-ray bundles: the per-pixel planes and counts from the centre rays and     caustic_discplane.cpp:217-334, caustic_plane.cpp:207-299
//                              the Jacobian from the four satellites
//   grid_gather_kernel         one ray per pixel: the per-pixel planes and counts                          caustic_discplane.cpp:349-401, caustic_sourceplane.cpp:180-232,
//                                                                                                          caustic_plane.cpp:315-349
//   neighbour_jacobian_kernel  grid-neighbour mode: central differences of the two coordinate planes;      caustic_discplane.cpp:403-439, caustic_sourceplane.cpp:264-305,
//                              the sphere wraps its phi differences                                        caustic_plane.cpp:357-392
//   suppress_mark_kernel, suppress_clear_kernel   the disc's branch-boundary filter on a snapshot of SIGN_J  caustic_discplane.cpp:455-493
// What differs between the three maps is a "surface" (DiscSurface, SphereSurface, PlaneSurface below): what a record becomes, what the pixel's own ray
// keeps, the planes and counts of a pixel, and whether the pass stores to the records -- a property of the surface's type: the disc computes
// redshift(dest, reverse) and stores it, the other two take const records.
// All of them are streaming passes.  Records are read ONE PER WORK-ITEM, like every other pass over the 144-byte records (adjacent lanes read
// adjacent records: a wave covers 9216 contiguous bytes, every 128-byte line it touches is used whole), NOT one bundle (720 bytes) per work-item:
// the per-ray work -- redshift_dest_value, sincos, atan2, sincos -- is what the pass computes, so it gets five times the lanes; the five end points
// of a bundle meet in LDS (32 bytes per ray), and the lanes that own a pixel then write the planes at consecutive addresses.  DESIGN.md 4.2.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "kr_pass.hpp"

namespace kr {

namespace {

constexpr int kBundle = 5;                 // ImagePlaneBundles::RAYS_PER_BUNDLE: centre, east, west, north, south
constexpr double kSentinel = 1e30;         // caustic_discplane.cpp:152, caustic_sourceplane.cpp:259, caustic_plane.cpp:161
enum Plane { P_DET = 0, P_SIGN, P_ORDER, P_HIT };          // the first four planes of every map; a surface names the rest
enum Kind { K_SPHERE = 0, K_PLANE = 1 };                   // kr_source_map::kind

// the pixel grid of either map description
struct Pixels {
    int nx, ny;
    double eps_x, eps_y;
};
template <typename M>
Pixels pixels_of(const M& m) { return Pixels{m.nx, m.ny, m.eps_x, m.eps_y}; }

// ---- ImagePlaneBundles ctor (imageplane_bundles.h:150-199) + redshift_start(0, true) in one pass: slot s is member s % 5 of bundle s / 5 ------
KR_DEV kr_ray_f64 bundle_ray(const kr_imageplane& s, const PlaneTrig& tr, long long n_grid, int Ny, double eps_x, double eps_y, double a, long long slot)
{
    const long long b = slot / kBundle;
    if (!(b < n_grid)) return dead_ray();
    const int m = (int) (slot - b * kBundle);
    const int i = (int) (b / Ny), j = (int) (b % Ny);
    const double x = s.x0 + i * s.dy;                // sic: dy on both axes, imageplane_bundles.h:169-172
    const double y = s.y0 + j * s.dy;
    const double xs = m == 1 ? x + eps_x : (m == 2 ? x - eps_x : x);
    const double ys = m == 3 ? y + eps_y : (m == 4 ? y - eps_y : y);
    return camera_ray<true>(tr, a, s.dist, s.phi0, xs, ys);
}

__global__ void __launch_bounds__(kBlock)
bundles_init_emit_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_imageplane s, PlaneTrig tr, int Nx, int Ny, double eps_x, double eps_y, double spin, double V,
                         int reverse, int projradius)
{
    const long long n_grid = (long long) Nx * Ny;
    const double a = -1 * s.spin;
    const double am = reverse ? -1 * spin : spin;
    if (V == -1) {
        const kr_ray_f64 r0 = bundle_ray(s, tr, n_grid, Ny, eps_x, eps_y, a, 0);      // record 0 of the source (raytracer.cpp:389-393)
        V = keplerian_V<double>(am, r0.r, r0.theta, projradius != 0);
    }
    KR_GRID_STRIDE(slot, n) {
        kr_ray_f64 ray = bundle_ray(s, tr, n_grid, Ny, eps_x, eps_y, a, slot);
        ray.emit = emit_value(ray, spin, am, V, reverse);
        rays[slot] = ray;
    }
}

// ---- the surfaces ---------------------------------------------------------------------------------------------------------------------------
// what one record contributes: to its own pixel when it is the ray through the pixel, to the Jacobian when it is a satellite
struct EndPoint {
    double phi, u, v;
    int hit, flips;
};

// the disc (caustic_discplane.cpp:170-202, :255-276): (u, v) = (X_DISC, Y_DISC)
struct DiscSurface {
    using Ray = kr_ray_f64;                // redshift is stored back
    static constexpr int kPlanes = 9, kCounts = 7, kU = 6, kV = 7;
    static constexpr bool kHasBundles = true, kWrapsV = false;
    enum { P_RADIUS = 4, P_PHI, P_X, P_Y, P_REDSHIFT };
    enum { C_DISC = 0, C_HORIZON, C_RLIM, C_STEPLIM, C_OUT_OF_RANGE, C_OTHER, C_SUPPRESSED };
    struct Centre {
        double r, phi_s, g;
        int order, cls;           // cls: 0 none, else the count of its failure mode
    };
    double spin, r_isco, r_disc;
    int reverse;

    // (the centre's order and failure mode are worked out here, by every lane beside its neighbours, not by the one wave that writes the pixels)
    KR_DEV EndPoint end(Ray* ray, Centre& c) const
    {
        const double r = ray->r, phi = ray->phi;
        const int steps = ray->steps, status = ray->status, flips = ray->rdot_flips;
        const double g = redshift_dest_value<double>(r, ray->theta, ray->k, ray->h, ray->Q, ray->rdot_sign, ray->thetadot_sign, ray->emit, spin, reverse);
        ray->redshift = g;
        // valid_hit, caustic_discplane.cpp:177-182
        const bool valid = steps > 0 && r >= r_isco && r < r_disc && g > 0;
        EndPoint e = {phi, 0, 0, valid ? 1 : 0, flips};
        c = Centre{r, 0, g, -1, 0};
        if (valid) {
            // disc_xy, :170-174: phi_s = atan2(sin phi, cos phi) of the ACCUMULATED phi, then r cos / r sin of phi_s
            double sp, cp;
            kr_sincos_f64(phi, sp, cp);
            c.phi_s = krcr::kr_atan2_cr(sp, cp);
            kr_sincos_f64(c.phi_s, sp, cp);
            e.u = r * cp;
            e.v = r * sp;
            // disc_order, :198-202
            const int phi_ord = (int) (kr_abs(phi) / (2 * kPi));
            const int r_ord = flips / 2;
            c.order = phi_ord > r_ord ? phi_ord : r_ord;
        }
        // the failure modes of the centre rays, :255-276
        if (steps > 0 && (r < r_isco || r >= r_disc || g <= 0)) {
            c.cls = C_OUT_OF_RANGE;
        } else if (steps <= 0 || !(status & KR_STATUS_DEST)) {
            if (status & KR_STATUS_HORIZON) c.cls = C_HORIZON;
            else if (status & KR_STATUS_RLIM) c.cls = C_RLIM;
            else if (status & KR_STATUS_STEPLIM) c.cls = C_STEPLIM;
            else c.cls = C_OTHER;
        }
        return e;
    }

    KR_DEV void write_pixel(double* __restrict__ maps, long long npix, long long px, const EndPoint& e, const Centre& c, unsigned* cnt) const
    {
        const bool hit = e.hit != 0;
        cnt[C_DISC] += hit;
#pragma unroll
        for (int k = C_HORIZON; k <= C_OTHER; k++) cnt[k] += c.cls == k;         // every index a constant: the counters stay in registers
        maps[P_ORDER * npix + px] = (double) c.order;
        maps[P_HIT * npix + px] = hit ? 1.0 : 0.0;
        maps[P_RADIUS * npix + px] = hit ? c.r : 0.0;
        maps[P_PHI * npix + px] = hit ? c.phi_s : 0.0;
        maps[P_X * npix + px] = hit ? e.u : 0.0;
        maps[P_Y * npix + px] = hit ? e.v : 0.0;
        maps[P_REDSHIFT * npix + px] = hit ? c.g : 0.0;
    }
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

// what the two source maps share: (u, v) = (THETA_S, PHI_S) or (X_S, Y_S), the six planes and the three counts of the ray through pixel px
// (caustic_sourceplane.cpp:187-231, caustic_plane.cpp:213-239)
struct SourceSurface {
    using Ray = const kr_ray_f64;          // the records are only read
    static constexpr int kPlanes = 8, kCounts = 3, kU = 4, kV = 5;
    enum { P_U = 4, P_V, P_FLIPS, P_EQUAT };
    enum { C_HIT = 0, C_CAPTURED, C_STEPLIM };
    struct Centre {
        int order, steps, status, equat;
    };
    static KR_DEV Centre centre_of(Ray* ray, int order) { return Centre{order, ray->steps, ray->status, ray->equatorial_crossings}; }

    KR_DEV void write_pixel(double* __restrict__ maps, long long npix, long long px, const EndPoint& e, const Centre& c, unsigned* cnt) const
    {
        const bool hit = e.hit != 0;
        if (hit) cnt[C_HIT]++;
        else if (c.status & KR_STATUS_HORIZON) cnt[C_CAPTURED]++;
        if (c.steps <= 0 || (c.status & KR_STATUS_STEPLIM)) cnt[C_STEPLIM]++;
        maps[P_ORDER * npix + px] = (double) c.order;
        maps[P_HIT * npix + px] = hit ? 1.0 : 0.0;
        maps[P_U * npix + px] = hit ? e.u : __builtin_nan("");
        maps[P_V * npix + px] = hit ? e.v : __builtin_nan("");
        maps[P_FLIPS * npix + px] = (double) e.flips;
        maps[P_EQUAT * npix + px] = (double) c.equat;
    }
};
struct SphereSurface : SourceSurface {
    static constexpr bool kHasBundles = false, kWrapsV = true;         // V is an angle in [-pi, pi]
    KR_DEV EndPoint end(Ray* ray, Centre& c) const
    {
        int order;
        const EndPoint e = sphere_end(ray, order);
        c = centre_of(ray, order);
        return e;
    }
};
struct PlaneSurface : SourceSurface {
    static constexpr bool kHasBundles = true, kWrapsV = false;
    kr_source_map m;
    KR_DEV EndPoint end(Ray* ray, Centre& c) const
    {
        int order;
        const EndPoint e = plane_end(ray, m, order);
        c = centre_of(ray, order);
        return e;
    }
};

// COUNTS counters per work-item: wave shuffle -> workgroup (LDS) -> one atomic per non-zero word and workgroup.  Every work-item of the workgroup calls this.
template <int WAVES, int COUNTS>
KR_DEV void flush_counts(const unsigned* cnt, unsigned (*part)[COUNTS], double* __restrict__ counts)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < COUNTS; k++) {
        const unsigned v = wave_sum(cnt[k]);
        if ((t & 63) == 0) part[t >> 6][k] = v;
    }
    __syncthreads();
    if (t < COUNTS) {
        unsigned v = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) v += part[w][t];
        if (v) atomicAdd(&counts[t], (double) v);
    }
}

// ---- grid mode: record px is the ray through pixel px = ix ny + iy (ImagePlane's order); records from npix on are not pixels ----------------------
template <typename S>
__global__ void __launch_bounds__(kBlock)
grid_gather_kernel(typename S::Ray* __restrict__ rays, long long n, S s, long long npix, double* __restrict__ maps)
{
    __shared__ unsigned part[kBlock / 64][S::kCounts];
    unsigned cnt[S::kCounts] = {};
    KR_GRID_STRIDE(i, n) {
        typename S::Centre c;
        const EndPoint e = s.end(&rays[i], c);
        if (i < npix) s.write_pixel(maps, npix, i, e, c, cnt);
    }
    flush_counts<kBlock / 64, S::kCounts>(cnt, part, maps + S::kPlanes * npix);
}

// ---- bundles: record 5 px + k is member k of the bundle of pixel px; BPB pixels per workgroup pass ----------------------------------------------
// ... one array per member in LDS: the gather reads members 5 t + k of lane t, 40 bytes apart as doubles (a 2-way bank conflict) instead of 160 as records (8-way)
template <int N>
struct EndPoints {
    double phi[N], u[N], v[N];
    int hit[N], flips[N];
    KR_DEV void put(int i, const EndPoint& e) { phi[i] = e.phi; u[i] = e.u; v[i] = e.v; hit[i] = e.hit; flips[i] = e.flips; }
    KR_DEV EndPoint get(int i) const { return EndPoint{phi[i], u[i], v[i], hit[i], flips[i]}; }
};

// Jacobian from the satellites (caustic_discplane.cpp:279-334, caustic_plane.cpp:249-299)
KR_DEV void satellite_jacobian(const EndPoint& ec, const EndPoint& ee, const EndPoint& ew, const EndPoint& en, const EndPoint& es, double eps_x, double eps_y,
                               double& det, double& sign)
{
    det = __builtin_nan("");
    sign = 0;
    if (ec.hit && ee.hit && ew.hit && en.hit && es.hit) {
        const bool order_match = ee.flips == ec.flips && ew.flips == ec.flips && en.flips == ec.flips && es.flips == ec.flips &&
                                 kr_abs(ee.phi - ec.phi) < kPi2 && kr_abs(ew.phi - ec.phi) < kPi2 && kr_abs(en.phi - ec.phi) < kPi2 &&
                                 kr_abs(es.phi - ec.phi) < kPi2;
        if (!order_match) {
            det = kSentinel;
        } else {
            const double du_da = (ee.u - ew.u) / (2 * eps_x);
            const double du_db = (en.u - es.u) / (2 * eps_y);
            const double dv_da = (ee.v - ew.v) / (2 * eps_x);
            const double dv_db = (en.v - es.v) / (2 * eps_y);
            det = du_da * dv_db - du_db * dv_da;
            sign = (det > 0) ? 1.0 : (det < 0) ? -1.0 : 0.0;
        }
    }
}

template <typename S, int BPB>
__global__ void __launch_bounds__(kBundle * BPB)
bundle_gather_kernel(typename S::Ray* __restrict__ rays, long long n, S s, Pixels g, double* __restrict__ maps)
{
    constexpr int kThreads = kBundle * BPB;
    constexpr int kWaves = (kThreads + 63) / 64;
    __shared__ EndPoints<kThreads> ends;
    __shared__ typename S::Centre centres[BPB];
    __shared__ unsigned part[kWaves][S::kCounts];
    const long long npix = (long long) g.nx * g.ny;
    const long long chunks = (n + kThreads - 1) / kThreads;
    const int t = threadIdx.x;
    unsigned cnt[S::kCounts] = {};
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {       // uniform per workgroup: the barriers below are safe
        const long long i = chunk * kThreads + t;
        if (i < n) {
            typename S::Centre c;
            ends.put(t, s.end(&rays[i], c));
            if (t % kBundle == 0) centres[t / kBundle] = c;
        }
        __syncthreads();
        const long long px = chunk * BPB + t;
        if (t < BPB && px < npix) {
            const EndPoint ec = ends.get(t * kBundle);
            s.write_pixel(maps, npix, px, ec, centres[t], cnt);
            double det, sign;
            satellite_jacobian(ec, ends.get(t * kBundle + 1), ends.get(t * kBundle + 2), ends.get(t * kBundle + 3), ends.get(t * kBundle + 4), g.eps_x, g.eps_y, det, sign);
            maps[P_DET * npix + px] = det;
            maps[P_SIGN * npix + px] = sign;
        }
        __syncthreads();
    }
    flush_counts<kWaves, S::kCounts>(cnt, part, maps + S::kPlanes * npix);
}

// ---- grid-neighbour Jacobian: one pixel per work-item over the HIT / ORDER planes and the two coordinate planes pu, pv.  WRAP: v is an angle in
//      [-pi, pi], its differences are wrapped back into that range as wrap_dphi does (caustic_sourceplane.cpp:68-73; |d| <= 2 pi, so each of its loops
//      runs at most once) ------------------------------------------------------------------------------------------------------------------------
template <bool WRAP>
KR_DEV double wrapped(double d)
{
    if (WRAP) {
        if (d > kPi) d -= 2 * kPi;
        if (d < -kPi) d += 2 * kPi;
    }
    return d;
}

template <bool WRAP>
__global__ void __launch_bounds__(kBlock)
neighbour_jacobian_kernel(Pixels g, int pu, int pv, double* __restrict__ maps)
{
    const int nx = g.nx, ny = g.ny;
    const long long npix = (long long) nx * ny;
    const double* hit = maps + P_HIT * npix;
    const double* order = maps + P_ORDER * npix;
    const double* u = maps + pu * npix;
    const double* v = maps + pv * npix;
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
                    const double du_dx = (u[e] - u[w]) / (2 * g.eps_x);
                    const double du_dy = (u[nn] - u[s]) / (2 * g.eps_y);
                    const double dv_dx = wrapped<WRAP>(v[e] - v[w]) / (2 * g.eps_x);
                    const double dv_dy = wrapped<WRAP>(v[nn] - v[s]) / (2 * g.eps_y);
                    det = du_dx * dv_dy - du_dy * dv_dx;
                    sign = (det > 0) ? 1.0 : (det < 0) ? -1.0 : 0.0;
                }
            }
        }
        maps[P_DET * npix + px] = det;
        maps[P_SIGN * npix + px] = sign;
    }
}

// ---- branch-boundary suppression (caustic_discplane.cpp:455-493).  The reference works on a copy of SIGN_J; here the snapshot stays in the plane
//      itself: the first pass only DOUBLES the sign of a pixel it suppresses (+-1 -> +-2: whoever reads it meanwhile still sees the sign it had) and
//      writes its DET_J, the second pass turns the +-2 into 0.  No scratch buffer, so nothing to allocate or free around the launches. -------------
__global__ void __launch_bounds__(kBlock)
suppress_mark_kernel(kr_caustic_map m, double* __restrict__ maps)
{
    __shared__ unsigned part[kBlock / 64][1];
    const int nx = m.nx, ny = m.ny;
    const long long npix = (long long) nx * ny;
    double* sign = maps + P_SIGN * npix;
    unsigned suppressed = 0;
    KR_GRID_STRIDE(px, npix) {
        const double s = sign[px];
        if (s == 0.0) continue;
        const int ix = (int) (px / ny), iy = (int) (px % ny);
        int n_same = 0, n_opp = 0;
        const bool inside[4] = {ix > 0, ix < nx - 1, iy > 0, iy < ny - 1};
        const long long at[4] = {px - ny, px + ny, px - 1, px + 1};
#pragma unroll
        for (int d = 0; d < 4; d++) {
            if (!inside[d]) continue;
            const double sn = sign[at[d]];
            if (sn == 0.0) continue;
            if (sn * s > 0) ++n_same;
            else ++n_opp;
        }
        if (n_opp > n_same && n_opp >= 2) {
            maps[P_DET * npix + px] = kSentinel;
            sign[px] = 2 * s;
            ++suppressed;
        }
    }
    flush_counts<kBlock / 64, 1>(&suppressed, part, maps + DiscSurface::kPlanes * npix + DiscSurface::C_SUPPRESSED);
}

__global__ void __launch_bounds__(kBlock)
suppress_clear_kernel(long long npix, double* __restrict__ sign)
{
    KR_GRID_STRIDE(px, npix) {
        const double s = sign[px];
        if (s == 2.0 || s == -2.0) sign[px] = 0.0;
    }
}

// the counts cleared, then the gather of surface s over the n records and, in grid mode, the neighbour Jacobian
template <typename S>
int gather(const S& s, Pixels g, bool bundles, typename S::Ray* rays, long long n, double* maps, hipStream_t st)
{
    const long long npix = (long long) g.nx * g.ny;
    KR_HIP(hipMemsetAsync(maps + S::kPlanes * npix, 0, S::kCounts * sizeof(double), st));
    if constexpr (S::kHasBundles) {
        if (bundles) {
            constexpr int kPixels = 64;             // 320 work-items: five waves, one pixel per lane of the first in the gather
            hipLaunchKernelGGL((bundle_gather_kernel<S, kPixels>), dim3(grid_for(n, kBundle * kPixels, kCapStream)), dim3(kBundle * kPixels), 0, st, rays, n, s, g, maps);
            KR_LAUNCH_CHECK();
            return KR_OK;
        }
    }
    hipLaunchKernelGGL((grid_gather_kernel<S>), dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, rays, n, s, npix, maps);
    KR_LAUNCH_CHECK();
    hipLaunchKernelGGL((neighbour_jacobian_kernel<S::kWrapsV>), dim3(grid_for(npix, kBlock, kCapStream)), dim3(kBlock), 0, st, g, (int) S::kU, (int) S::kV, maps);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

// what the two map descriptions have in common; `rest` answers for the fields of its own (nullptr, or what is wrong).  n: the records the caller has
template <typename M, typename Rest>
int map_validate(const M* m, int64_t n, const char* who, Rest rest)
{
    auto bad = [&](const char* why) { set_error(std::string(who) + ": " + why); return KR_EINVAL; };
    if (!m) return bad("null map description");
    if (m->nx < 1 || m->ny < 1) return bad("nx and ny must be >= 1");
    if (!std::isfinite(m->eps_x) || !std::isfinite(m->eps_y) || !(m->eps_x > 0) || !(m->eps_y > 0)) return bad("eps_x and eps_y must be positive and finite");
    if (const char* why = rest(*m)) return bad(why);
    if (n < (m->bundles ? kBundle : 1) * (int64_t) m->nx * m->ny) return bad(m->bundles ? "n smaller than 5 nx ny" : "n smaller than nx ny");
    return KR_OK;
}

}  // namespace

int caustic_validate(const kr_caustic_map* m, int64_t n, const char* who)
{
    return map_validate(m, n, who, [](const kr_caustic_map& c) -> const char* {
        return !std::isfinite(c.r_isco) || !std::isfinite(c.r_disc) ? "non-finite disc radius" : nullptr;
    });
}

int source_map_validate(const kr_source_map* m, int64_t n, const char* who)
{
    return map_validate(m, n, who, [](const kr_source_map& s) -> const char* {
        if (s.kind != K_SPHERE && s.kind != K_PLANE) return "unknown kind (0: source sphere, 1: flat source plane)";
        if (s.kind == K_SPHERE && s.bundles) return "the source sphere has no bundle mode";
        if (s.kind == K_PLANE && !(std::isfinite(s.sin_incl) && std::isfinite(s.cos_incl) && std::isfinite(s.sin_phi0) && std::isfinite(s.cos_phi0)))
            return "non-finite sine or cosine of incl / phi0";
        return nullptr;
    });
}

int bundles_init_emit_dev(const kr_imageplane* s, int nx, int ny, double eps_frac, double V, int reverse, int projradius, void* d, int64_t n, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    hipLaunchKernelGGL(bundles_init_emit_kernel, dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *s, plane_trig(s), nx, ny,
                       eps_frac * s->dx, eps_frac * s->dy, -1 * s->spin, V, reverse, projradius);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

// every one of the n records gets its redshift, whether or not it belongs to a pixel
int post_caustic_dev(double spin, int reverse, const kr_caustic_map* m, void* d, int64_t n, void* d_maps, hipStream_t st)
{
    DiscSurface s;
    s.spin = spin; s.r_isco = m->r_isco; s.r_disc = m->r_disc; s.reverse = reverse;
    return gather(s, pixels_of(*m), m->bundles != 0, (kr_ray_f64*) d, (long long) n, (double*) d_maps, st);
}

int caustic_suppress_dev(const kr_caustic_map* m, void* d_maps, hipStream_t st)
{
    const long long npix = (long long) m->nx * m->ny;
    double* maps = (double*) d_maps;
    KR_HIP(hipMemsetAsync(maps + DiscSurface::kPlanes * npix + DiscSurface::C_SUPPRESSED, 0, sizeof(double), st));
    hipLaunchKernelGGL(suppress_mark_kernel, dim3(grid_for(npix, kBlock, kCapStream)), dim3(kBlock), 0, st, *m, maps);
    KR_LAUNCH_CHECK();
    hipLaunchKernelGGL(suppress_clear_kernel, dim3(grid_for(npix, kBlock, kCapStream)), dim3(kBlock), 0, st, npix, maps + P_SIGN * npix);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

// only the records of the pixels are read
int post_caustic_source_dev(const kr_source_map* m, const void* d, void* d_maps, hipStream_t st)
{
    const long long npix = (long long) m->nx * m->ny;
    const kr_ray_f64* rays = (const kr_ray_f64*) d;
    if (m->kind == K_SPHERE) return gather(SphereSurface(), pixels_of(*m), false, rays, npix, (double*) d_maps, st);
    PlaneSurface s;
    s.m = *m;
    return gather(s, pixels_of(*m), m->bundles != 0, rays, (m->bundles ? kBundle : 1) * npix, (double*) d_maps, st);
}

}  // namespace kr
