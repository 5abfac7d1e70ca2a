// spectrum_ray_per_lane.hip -- the obvious alternative to raytrace_cpu_amd/csrc/kr_spectrum.hip, for scripts/disc_spectrum_ab.py only: the shape of the
// line kernels (kr_line.hip) stretched over the continuum.  One RECORD per lane; a lane whose ray passes the filter loops over all ne energies and adds
// each term into a spectrum privatised per workgroup in LDS (ds_add_f64), flushed with one global atomic per non-zero word at the end.  Same rule, same
// records (already redshifted: the reduce form), same grid of workgroups.  Built as a small shared library:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -shared -o libspectrum_alt.so spectrum_ray_per_lane.hip
#include <hip/hip_runtime.h>

#include "../../include/kr_trace.h"

namespace {

constexpr int kBlock = 256;

struct Alt {
    double e_min, de, r_isco, r_disc, f_col, fcol_m4, table_r_min, table_dr, log_tdr, log_sde, log_semin, log_span, s_e_min, s_e_last;
    const double* t_kt;
    const double* s;
    int ne, log_e, table_nr, s_ne, nz;
};

template <bool THERMAL>
__global__ void __launch_bounds__(kBlock) ray_per_lane_kernel(const kr_ray_f64* __restrict__ rays, long long n, Alt A, double* __restrict__ out)
{
    extern __shared__ double lds[];                      // [ne] the spectrum, then [ne] the energies, then [ne] u_i
    double* E = lds + A.ne;
    double* U = E + A.ne;
    for (int e = threadIdx.x; e < A.ne; e += kBlock) {
        lds[e] = 0;
        E[e] = A.log_e ? A.e_min * pow(A.de, e + 0.5) : A.e_min + (e + 0.5) * A.de;
        U[e] = THERMAL ? 0 : (log(E[e]) - A.log_semin) / A.log_sde;
    }
    __syncthreads();
    for (long long i = blockIdx.x * (long long) kBlock + threadIdx.x; i < n; i += (long long) gridDim.x * kBlock) {
        const kr_ray_f64* ray = &rays[i];
        const double r = ray->r, g = ray->redshift;
        if (!(ray->steps > 0)) continue;
        if (!(r * cos(ray->theta) < 1E-2 && r >= A.r_isco && r < A.r_disc && g > 0)) continue;
        const double g3 = 1 / (g * g * g);
        if (THERMAL) {
            const double fi = log(r / A.table_r_min) / A.log_tdr;
            if (!(fi > -1 && fi < A.table_nr)) continue;
            const double kT = A.t_kt[(int) fi];
            if (!(__builtin_isfinite(kT) && kT > 0)) continue;
            const double q = 1 / (A.f_col * kT), w = g3 * A.fcol_m4;
            for (int e = 0; e < A.ne; e++) {
                const double Ep = g * E[e];
                atomicAdd(&lds[e], w * (Ep * Ep * Ep) / expm1(Ep * q));
            }
        } else {
            const double fz = A.nz * log(r / A.r_isco) / A.log_span;
            const double* Sz = A.s + (size_t) (int) fmin(fmax(fz, 0.0), (double) (A.nz - 1)) * A.s_ne;
            const double q = log(g) / A.log_sde, w = g3 / (r * r * r);
            for (int e = 0; e < A.ne; e++) {
                const double Ep = g * E[e];
                if (!(Ep >= A.s_e_min && Ep <= A.s_e_last)) continue;
                const double p = fmin(fmax(q + U[e], 0.0), (double) (A.s_ne - 1));
                const int k = min((int) p, A.s_ne - 2);
                const double v0 = Sz[k], v1 = Sz[k + 1];
                atomicAdd(&lds[e], w * (v0 + (p - k) * (v1 - v0)));
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < A.ne; e += kBlock)
        if (lds[e] != 0) atomicAdd(&out[e], lds[e]);
}

}  // namespace

// d_kt (thermal) or d_s (table): device arrays; m: the model as the library takes it (its host pointers are not read).  Adds into d_out[0 .. ne).
extern "C" int alt_spectrum(const kr_spectrum_model* m, const double* d_kt, const double* d_s, const void* d_rays, long long n, void* d_out, int blocks)
{
    Alt A;
    A.e_min = m->e_min; A.de = m->de; A.r_isco = m->r_isco; A.r_disc = m->r_disc; A.f_col = m->f_col;
    A.fcol_m4 = 1 / (m->f_col * m->f_col * m->f_col * m->f_col);
    A.table_r_min = m->table_r_min; A.table_dr = m->table_dr; A.log_tdr = log(m->table_dr);
    A.log_sde = m->model ? log(m->s_de) : 0; A.log_semin = m->model ? log(m->s_e_min) : 0; A.log_span = log(m->r_disc / m->r_isco);
    A.s_e_min = m->s_e_min; A.s_e_last = m->model ? m->s_e_min * pow(m->s_de, (double) (m->s_ne - 1)) : 0;
    A.t_kt = d_kt; A.s = d_s;
    A.ne = m->ne; A.log_e = m->log_e; A.table_nr = m->table_nr; A.s_ne = m->s_ne; A.nz = m->nz;
    const size_t lds = 3 * (size_t) m->ne * sizeof(double);
    if (m->model == 0) hipLaunchKernelGGL(ray_per_lane_kernel<true>, dim3(blocks), dim3(kBlock), lds, nullptr, (const kr_ray_f64*) d_rays, n, A, (double*) d_out);
    else hipLaunchKernelGGL(ray_per_lane_kernel<false>, dim3(blocks), dim3(kBlock), lds, nullptr, (const kr_ray_f64*) d_rays, n, A, (double*) d_out);
    return (int) hipGetLastError();
}
