// hotspot_ray_per_lane.hip -- the obvious alternative to raytrace_cpu_amd/csrc/kr_hotspot.hip, for scripts/hotspot_ab.py only: the shape of the line
// kernels (kr_line.hip) stretched over the time axis.  One RECORD per lane; a lane whose ray is in the spot's ring loops over all nt observer times and
// adds each non-zero term into the light curve privatised per workgroup in LDS (ds_add_f64: flux, sx, sy), flushed with one global atomic per non-zero
// word at the end; the spectrogram cell of a non-zero term is added to global memory.  Same rule, same records (already redshifted: the reduce form),
// same grid of workgroups.  Built as a small shared library:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -shared -o libhotspot_alt.so hotspot_ray_per_lane.hip
#include <hip/hip_runtime.h>

#include "../../include/kr_trace.h"

namespace {

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) ray_per_lane_kernel(const kr_ray_f64* __restrict__ rays, long long n, kr_hotspot h, double ring, double rs2, double m_inv,
                                                             double floor_s, double log_de, double* __restrict__ out)
{
    extern __shared__ double lds[];                      // [3 nt]: flux, sx, sy
    const int nt = h.nt, ne = h.ne;
    for (int w = threadIdx.x; w < 3 * nt; w += kBlock) lds[w] = 0;
    __syncthreads();
    double* const g_spec = out + 3 * (size_t) nt;
    unsigned long long on_disc = 0, used = 0;
    for (long long i = blockIdx.x * (long long) kBlock + threadIdx.x; i < n; i += (long long) gridDim.x * kBlock) {
        const kr_ray_f64* ray = &rays[i];
        const double r = ray->r, g = ray->redshift;
        if (!(ray->steps > 0)) continue;
        if (!(r * cos(ray->theta) < 1E-2 && r >= h.r_isco && r < h.r_disc && g > 0)) continue;
        on_disc++;
        if (!(fabs(r - h.r_spot) < ring)) continue;
        used++;
        const double Om = h.shear ? 1 / (h.a_orbit + r * sqrt(r)) : h.omega;
        const double c = pow(g, -1 * h.g_index), cx = c * ray->alpha, cy = c * ray->beta;
        const double A = r * r + rs2, B = 2 * r * h.r_spot, phi = ray->phi, t = ray->t;
        int ie = -1;
        if (ne > 0) {
            const double E = h.line_energy / g;
            const double fe = h.log_e ? log(E / h.e_min) / log_de : (E - h.e_min) / h.de;
            if (fe >= 0 && fe < ne) ie = (int) fe;
        }
        for (int k = 0; k < nt; k++) {
            const double T = h.t0 + k * h.dt;
            const double d2 = A - B * cos(phi - (h.phi0 + Om * (T - t)));
            const double s = exp(d2 * m_inv) - floor_s;
            if (!(s > 0)) continue;
            atomicAdd(&lds[k], c * s);
            atomicAdd(&lds[nt + k], cx * s);
            atomicAdd(&lds[2 * nt + k], cy * s);
            if (ie >= 0) atomicAdd(&g_spec[(size_t) k * ne + ie], c * s);
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < 3 * nt; w += kBlock)
        if (lds[w] != 0) atomicAdd(&out[w], lds[w]);
    double* const tallies = out + (size_t) nt * (3 + ne);
    if (on_disc) atomicAdd(&tallies[0], (double) on_disc);
    if (used) atomicAdd(&tallies[1], (double) used);
}

}  // namespace

// adds into d_out (nt (3 + ne) + 4 doubles), the layout of kr_reduce_hotspot_dev_f64
extern "C" int alt_hotspot(const kr_hotspot* h, const void* d_rays, long long n, void* d_out, int blocks)
{
    const double ring = h->cut * h->sigma;
    hipLaunchKernelGGL(ray_per_lane_kernel, dim3(blocks), dim3(kBlock), 3 * (size_t) h->nt * sizeof(double), nullptr, (const kr_ray_f64*) d_rays, n, *h, ring,
                       h->r_spot * h->r_spot, -1 / (2 * h->sigma * h->sigma), exp(-1 * h->cut * h->cut / 2), h->ne > 0 && h->log_e ? log(h->de) : 0.0, (double*) d_out);
    return (int) hipGetLastError();
}
