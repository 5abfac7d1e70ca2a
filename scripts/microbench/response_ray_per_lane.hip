// response_ray_per_lane.hip -- the naive alternative to raytrace_cpu_amd/csrc/kr_response.hip, for scripts/response_ab.py only and never in the product: one
// RECORD per lane; a lane whose ray passes the filter and falls inside the time window loops over all ne energies and issues ONE global atomic per
// (ray, energy) into resp[j ne + e].  Same rule (powerlaw3 with q = 3 throughout, no tables, isotropic), same records (already redshifted: the reduce
// form), same grid of workgroups.  Built as a small shared library:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -shared -o libresponse_alt.so response_ray_per_lane.hip
#include <hip/hip_runtime.h>

#include "../../include/kr_trace.h"

namespace {

constexpr int kBlock = 256;

struct Alt {
    double e_min, de, r_isco, r_disc, log_sde, log_semin, log_span, s_e_min, s_e_last, t0, dt;
    const double* s;
    int ne, log_e, s_ne, nz, nt;
};

__global__ void __launch_bounds__(kBlock) ray_per_lane_kernel(const kr_ray_f64* __restrict__ rays, long long n, Alt A, double* __restrict__ out)
{
    extern __shared__ double lds[];                      // [ne] the energies, then [ne] u_i
    double* E = lds;
    double* U = E + A.ne;
    for (int e = threadIdx.x; e < A.ne; e += kBlock) {
        E[e] = A.log_e ? A.e_min * pow(A.de, e + 0.5) : A.e_min + (e + 0.5) * A.de;
        U[e] = (log(E[e]) - A.log_semin) / A.log_sde;
    }
    __syncthreads();
    for (long long i = blockIdx.x * (long long) kBlock + threadIdx.x; i < n; i += (long long) gridDim.x * kBlock) {
        const kr_ray_f64* ray = &rays[i];
        const double r = ray->r, g = ray->redshift;
        if (!(ray->steps > 0)) continue;
        if (!(r * cos(ray->theta) < 1E-2 && r >= A.r_isco && r < A.r_disc && g > 0)) continue;
        const double ft = (ray->t - A.t0) / A.dt;
        if (!(ft >= 0 && ft < A.nt)) continue;
        double* row = out + (size_t) (int) ft * A.ne;
        const double g3 = 1 / (g * g * g);
        const double fz = A.nz * log(r / A.r_isco) / A.log_span;
        const double* Sz = A.s + (size_t) (int) fmin(fmax(fz, 0.0), (double) (A.nz - 1)) * A.s_ne;
        const double q = log(g) / A.log_sde, w = g3 / (r * r * r);
        for (int e = 0; e < A.ne; e++) {
            const double Ep = g * E[e];
            if (!(Ep >= A.s_e_min && Ep <= A.s_e_last)) continue;
            const double p = fmin(fmax(q + U[e], 0.0), (double) (A.s_ne - 1));
            const int k = min((int) p, A.s_ne - 2);
            const double v0 = Sz[k], v1 = Sz[k + 1];
            atomicAdd(&row[e], w * (v0 + (p - k) * (v1 - v0)));
        }
    }
}

}  // namespace

// d_s: the table S on the device; r: the model as the library takes it (its host pointers are not read).  Adds into d_out[0 .. nt ne).
extern "C" int alt_response(const kr_response_model* r, const double* d_s, const void* d_rays, long long n, void* d_out, int blocks)
{
    const kr_spectrum_model* m = &r->spec;
    Alt A;
    A.e_min = m->e_min; A.de = m->de; A.r_isco = m->r_isco; A.r_disc = m->r_disc;
    A.log_sde = log(m->s_de); A.log_semin = log(m->s_e_min); A.log_span = log(m->r_disc / m->r_isco);
    A.s_e_min = m->s_e_min; A.s_e_last = m->s_e_min * pow(m->s_de, (double) (m->s_ne - 1));
    A.t0 = r->t0; A.dt = r->dt; A.nt = r->nt;
    A.s = d_s;
    A.ne = m->ne; A.log_e = m->log_e; A.s_ne = m->s_ne; A.nz = m->nz;
    hipLaunchKernelGGL(ray_per_lane_kernel, dim3(blocks), dim3(kBlock), 2 * (size_t) m->ne * sizeof(double), nullptr, (const kr_ray_f64*) d_rays, n, A, (double*) d_out);
    return (int) hipGetLastError();
}
