// kr_caustic.hip -- critical-curve (caustic) maps of the disc seen on an image plane (include/kr_trace.h, kr_caustic_map): the reference's
// src/caustic/caustic_discplane.cpp with the rays where they already are, in HBM.  The reference builds the 5-ray bundles in a serial host loop
// (imageplane_bundles.h:150-199), and gathers, differences and filters rays[] on one core (caustic_discplane.cpp:219-493); here
//   bundles_init_emit_kernel   ImagePlaneBundles ctor + redshift_start(0, reverse = true)                 imageplane_bundles.h:150-199, raytracer.cpp:342-417
//   post_caustic_kernel        redshift(dest, reverse) + the seven per-pixel planes + the diagnostic counts  caustic_discplane.cpp:217-276 / :349-401
//                              and, for bundles, the Jacobian from the four satellites                        :279-334
//   grid_jacobian_kernel       grid-neighbour mode: central differences of the X_DISC / Y_DISC planes         :403-439
//   suppress_mark_kernel, suppress_clear_kernel   the branch-boundary filter on a snapshot of SIGN_J        :455-493
// All of them are streaming passes.  Records are read ONE PER WORK-ITEM, like every other pass over the 144-byte records (adjacent lanes read
// adjacent records: a wave covers 9216 contiguous bytes, every 128-byte line it touches is used whole), NOT one bundle (720 bytes) per work-item:
// the per-ray work -- redshift_dest_value, sincos, atan2, sincos -- is what the pass computes, so it gets five times the lanes; the five end points
// of a bundle meet in LDS (32 bytes per ray), and the lanes that own a pixel then write the nine planes at consecutive addresses.  DESIGN.md 4.2.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "kr_pass.hpp"

namespace kr {

namespace {

constexpr int kBundle = 5;                 // ImagePlaneBundles::RAYS_PER_BUNDLE: centre, east, west, north, south
constexpr double kSentinel = 1e30;         // caustic_discplane.cpp:152
constexpr int kPlanes = 9, kCounts = 7;
enum Plane { P_DET = 0, P_SIGN, P_ORDER, P_HIT, P_RADIUS, P_PHI, P_X, P_Y, P_REDSHIFT };
enum Count { C_DISC = 0, C_HORIZON, C_RLIM, C_STEPLIM, C_OUT_OF_RANGE, C_OTHER, C_SUPPRESSED };

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

// ---- the epilogue.  RPB rays per pixel (5: bundles, 1: the plain ImagePlane grid), BPB pixels per workgroup pass -----------------------------
// what a satellite contributes to the Jacobian, and the centre to everything else
struct EndPoint {
    double phi, x, y;
    int valid, flips;
};
// ... one array per member in LDS: the gather reads members 5 t + k of lane t, 40 bytes apart as doubles (a 2-way bank conflict) instead of 160 as records (8-way)
template <int N>
struct EndPoints {
    double phi[N], x[N], y[N];
    int valid[N], flips[N];
    KR_DEV void put(int i, const EndPoint& e) { phi[i] = e.phi; x[i] = e.x; y[i] = e.y; valid[i] = e.valid; flips[i] = e.flips; }
    KR_DEV EndPoint get(int i) const { return EndPoint{phi[i], x[i], y[i], valid[i], flips[i]}; }
};
struct Centre {
    double r, phi_s, g;
    int order, cls;           // cls: 0 none, else the Count of its failure mode
};

template <int RPB, int BPB>
__global__ void __launch_bounds__(RPB * BPB)
post_caustic_kernel(kr_ray_f64* __restrict__ rays, long long n, double spin, int reverse, kr_caustic_map m, double* __restrict__ maps)
{
    constexpr int kThreads = RPB * BPB;
    __shared__ EndPoints<kThreads> ends;
    __shared__ Centre centres[BPB];
    __shared__ unsigned part[(BPB + 63) / 64][C_SUPPRESSED];
    const long long npix = (long long) m.nx * m.ny;
    const long long chunks = (n + kThreads - 1) / kThreads;
    const int t = threadIdx.x;
    unsigned cnt[C_SUPPRESSED] = {0, 0, 0, 0, 0, 0};
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {       // uniform per workgroup: the barriers below are safe
        const long long i = chunk * kThreads + t;
        if (i < n) {
            kr_ray_f64* ray = &rays[i];
            const double r = ray->r, phi = ray->phi;
            const int steps = ray->steps, status = ray->status, flips = ray->rdot_flips;
            const double g = redshift_dest_value<double>(r, ray->theta, ray->k, ray->h, ray->Q, ray->rdot_sign, ray->thetadot_sign, ray->emit, spin, reverse);
            ray->redshift = g;
            // valid_hit, caustic_discplane.cpp:177-182
            const bool valid = steps > 0 && r >= m.r_isco && r < m.r_disc && g > 0;
            EndPoint e = {phi, 0, 0, valid ? 1 : 0, flips};
            double phi_s = 0;
            if (valid) {
                // disc_xy, :170-174: phi_s = atan2(sin phi, cos phi) of the ACCUMULATED phi, then r cos / r sin of phi_s
                double sp, cp;
                kr_sincos_f64(phi, sp, cp);
                phi_s = krcr::kr_atan2_cr(sp, cp);
                kr_sincos_f64(phi_s, sp, cp);
                e.x = r * cp;
                e.y = r * sp;
            }
            ends.put(t, e);
            if (t % RPB == 0) {
                Centre c = {r, phi_s, g, -1, 0};
                if (valid) {
                    // disc_order, :198-202
                    const int phi_ord = (int) (kr_abs(phi) / (2 * kPi));
                    const int r_ord = flips / 2;
                    c.order = phi_ord > r_ord ? phi_ord : r_ord;
                }
                // the failure modes of the centre rays, :255-276
                if (steps > 0 && (r < m.r_isco || r >= m.r_disc || g <= 0)) {
                    c.cls = C_OUT_OF_RANGE;
                } else if (steps <= 0 || !(status & KR_STATUS_DEST)) {
                    if (status & KR_STATUS_HORIZON) c.cls = C_HORIZON;
                    else if (status & KR_STATUS_RLIM) c.cls = C_RLIM;
                    else if (status & KR_STATUS_STEPLIM) c.cls = C_STEPLIM;
                    else c.cls = C_OTHER;
                }
                centres[t / RPB] = c;
            }
        }
        __syncthreads();
        const long long px = chunk * BPB + t;
        if (t < BPB && px < npix) {
            const Centre c = centres[t];
            const EndPoint ec = ends.get(t * RPB);
            const bool hit = ec.valid != 0;
            if (hit) cnt[C_DISC]++;
            if (c.cls) cnt[c.cls]++;
            maps[P_ORDER * npix + px] = hit ? (double) c.order : -1.0;
            maps[P_HIT * npix + px] = hit ? 1.0 : 0.0;
            maps[P_RADIUS * npix + px] = hit ? c.r : 0.0;
            maps[P_PHI * npix + px] = hit ? c.phi_s : 0.0;
            maps[P_X * npix + px] = hit ? ec.x : 0.0;
            maps[P_Y * npix + px] = hit ? ec.y : 0.0;
            maps[P_REDSHIFT * npix + px] = hit ? c.g : 0.0;
            if (RPB == kBundle) {
                // Jacobian from the satellites, :279-334
                double det = __builtin_nan(""), sign = 0;
                const EndPoint ee = ends.get(t * RPB + 1), ew = ends.get(t * RPB + 2), en = ends.get(t * RPB + 3), es = ends.get(t * RPB + 4);
                if (hit && ee.valid && ew.valid && en.valid && es.valid) {
                    const bool order_match = ee.flips == ec.flips && ew.flips == ec.flips && en.flips == ec.flips && es.flips == ec.flips &&
                                             kr_abs(ee.phi - ec.phi) < kPi2 && kr_abs(ew.phi - ec.phi) < kPi2 && kr_abs(en.phi - ec.phi) < kPi2 &&
                                             kr_abs(es.phi - ec.phi) < kPi2;
                    if (!order_match) {
                        det = kSentinel;
                    } else {
                        const double dxd_da = (ee.x - ew.x) / (2 * m.eps_x);
                        const double dxd_db = (en.x - es.x) / (2 * m.eps_y);
                        const double dyd_da = (ee.y - ew.y) / (2 * m.eps_x);
                        const double dyd_db = (en.y - es.y) / (2 * m.eps_y);
                        det = dxd_da * dyd_db - dxd_db * dyd_da;
                        sign = (det > 0) ? 1.0 : (det < 0) ? -1.0 : 0.0;
                    }
                }
                maps[P_DET * npix + px] = det;
                maps[P_SIGN * npix + px] = sign;
            }
        }
        __syncthreads();
    }
    // the six counters: wave shuffle -> workgroup (LDS) -> one atomic per non-zero word and workgroup (only the first BPB lanes hold any)
    if (t < BPB) {
#pragma unroll
        for (int k = 0; k < C_SUPPRESSED; k++) {
            unsigned v = cnt[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((t & 63) == 0) part[t >> 6][k] = v;
        }
    }
    __syncthreads();
    if (t < C_SUPPRESSED) {
        unsigned v = 0;
#pragma unroll
        for (int w = 0; w < (BPB + 63) / 64; w++) v += part[w][t];
        if (v) atomicAdd(&maps[kPlanes * npix + t], (double) v);
    }
}

// ---- grid-neighbour Jacobian (caustic_discplane.cpp:403-439): one pixel per work-item over the HIT / ORDER / X_DISC / Y_DISC planes ------------
__global__ void __launch_bounds__(kBlock)
grid_jacobian_kernel(kr_caustic_map m, double* __restrict__ maps)
{
    const int nx = m.nx, ny = m.ny;
    const long long npix = (long long) nx * ny;
    const double* hit = maps + P_HIT * npix;
    const double* order = maps + P_ORDER * npix;
    const double* xd = maps + P_X * npix;
    const double* yd = maps + P_Y * npix;
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
                    const double dxd_dx = (xd[e] - xd[w]) / (2 * m.eps_x);
                    const double dxd_dy = (xd[nn] - xd[s]) / (2 * m.eps_y);
                    const double dyd_dx = (yd[e] - yd[w]) / (2 * m.eps_x);
                    const double dyd_dy = (yd[nn] - yd[s]) / (2 * m.eps_y);
                    det = dxd_dx * dyd_dy - dxd_dy * dyd_dx;
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
    __shared__ unsigned part[kBlock / 64];
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
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) suppressed += __shfl_down(suppressed, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = suppressed;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned v = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) v += part[w];
        if (v) atomicAdd(&maps[kPlanes * npix + C_SUPPRESSED], (double) v);
    }
}

__global__ void __launch_bounds__(kBlock)
suppress_clear_kernel(long long npix, double* __restrict__ sign)
{
    KR_GRID_STRIDE(px, npix) {
        const double s = sign[px];
        if (s == 2.0 || s == -2.0) sign[px] = 0.0;
    }
}

}  // namespace

int caustic_validate(const kr_caustic_map* m, const char* who)
{
    auto bad = [&](const char* why) { set_error(std::string(who) + ": " + why); return KR_EINVAL; };
    if (!m) return bad("null map description");
    if (m->nx < 1 || m->ny < 1) return bad("nx and ny must be >= 1");
    if (!std::isfinite(m->eps_x) || !std::isfinite(m->eps_y) || !(m->eps_x > 0) || !(m->eps_y > 0)) return bad("eps_x and eps_y must be positive and finite");
    if (!std::isfinite(m->r_isco) || !std::isfinite(m->r_disc)) return bad("non-finite disc radius");
    return KR_OK;
}

int bundles_init_emit_dev(const kr_imageplane* s, int nx, int ny, double eps_frac, double V, int reverse, int projradius, void* d, int64_t n, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    hipLaunchKernelGGL(bundles_init_emit_kernel, dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *s, plane_trig(s), nx, ny,
                       eps_frac * s->dx, eps_frac * s->dy, -1 * s->spin, V, reverse, projradius);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int post_caustic_dev(double spin, int reverse, const kr_caustic_map* m, void* d, int64_t n, void* d_maps, hipStream_t st)
{
    const long long npix = (long long) m->nx * m->ny;
    double* maps = (double*) d_maps;
    KR_HIP(hipMemsetAsync(maps + kPlanes * npix, 0, kCounts * sizeof(double), st));
    if (m->bundles) {
        constexpr int kPixels = 64;                 // 320 work-items: five waves, one pixel per lane of the first in the gather
        hipLaunchKernelGGL((post_caustic_kernel<kBundle, kPixels>), dim3(grid_for(n, kBundle * kPixels, kCapStream)), dim3(kBundle * kPixels), 0, st, (kr_ray_f64*) d,
                           (long long) n, spin, reverse, *m, maps);
        KR_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL((post_caustic_kernel<1, kBlock>), dim3(grid_for(n, kBlock, kCapStream)), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, spin, reverse, *m, maps);
        KR_LAUNCH_CHECK();
        hipLaunchKernelGGL(grid_jacobian_kernel, dim3(grid_for(npix, kBlock, kCapStream)), dim3(kBlock), 0, st, *m, maps);
        KR_LAUNCH_CHECK();
    }
    return KR_OK;
}

int caustic_suppress_dev(const kr_caustic_map* m, void* d_maps, hipStream_t st)
{
    const long long npix = (long long) m->nx * m->ny;
    double* maps = (double*) d_maps;
    KR_HIP(hipMemsetAsync(maps + kPlanes * npix + C_SUPPRESSED, 0, sizeof(double), st));
    hipLaunchKernelGGL(suppress_mark_kernel, dim3(grid_for(npix, kBlock, kCapStream)), dim3(kBlock), 0, st, *m, maps);
    KR_LAUNCH_CHECK();
    hipLaunchKernelGGL(suppress_clear_kernel, dim3(grid_for(npix, kBlock, kCapStream)), dim3(kBlock), 0, st, npix, maps + P_SIGN * npix);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace kr
