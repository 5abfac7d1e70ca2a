// kr_illum.hip -- the (r, phi) illumination map of the disc (kr_illum_bins, include/kr_trace.h): the emissivity histogram of kr_post.hip with the
// azimuth of the landing point kept, for sources that are not on the axis.  One body for the reducing form (records read only) and the fused form
// (range_phi + redshift + the map, each record loaded once and left byte for byte as kr_post_emissivity_dev_f64 leaves it).
// The rays of a source's grid that are neighbours in the record array land in neighbouring cells, so many lanes of a wave add to the same cell.  Two
// accumulation paths:
//   LDS      ncell <= kIllumLdsCells: the five planes of a workgroup in LDS (ds_add_f64; 5 x 1024 doubles, the 40 KB of the emissivity reducer),
//            flushed with one global atomic per non-zero word and workgroup.
//   global   above that: global f64 atomics, the lanes of a wave that share a cell summed first (for_lane_groups, kr_recorder.hpp: hist_add of
//            kr_angdist.hip with ONE group search for the five planes) and their leader adding once.
// profiles/illum_map_ab.txt has both paths on either side of the crossover.  The cell index is formed and tested against ncell before any add on
// either path.  The two tallies go wave shuffle -> LDS -> one atomic per word and workgroup, as in kr_angdist.hip.

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "kr_disc_pass.hpp"
#include "kr_recorder.hpp"

namespace kr {

namespace {

constexpr int kIllumPlanes = 5;                  // count, flux, emis, sum_redshift, sum_time
constexpr int kIllumScalars = 2;                 // disc_count, binned
constexpr int kIllumMaxCells = 1 << 20;
// The crossover between the two paths.  The LDS path is the faster one wherever it exists (profiles/illum_map_ab.txt), so the
// crossover is the LDS budget itself: the planes of a workgroup stay within the emissivity reducer's 40 KB.  KR_ILLUM_LDS_CELLS = 0 builds the
// global path alone, for that A/B.
#ifndef KR_ILLUM_LDS_CELLS
#define KR_ILLUM_LDS_CELLS kMaxLdsBins
#endif
constexpr int kIllumLdsCells = KR_ILLUM_LDS_CELLS;
static_assert(kIllumLdsCells <= kMaxLdsBins, "the LDS planes stay within the emissivity reducer's budget");

template <bool USE_LDS, bool FUSED>
__global__ void __launch_bounds__(kBlock)
illum_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_illum_bins m, double dphi, double* __restrict__ out, double spin, double V, int reverse, int projradius,
             int motion, double lo, double hi)
{
    __shared__ double lds[USE_LDS && kIllumLdsCells > 0 ? kIllumPlanes * kIllumLdsCells : 1];
    __shared__ double part[kBlock / 64][kIllumScalars];
    const kr_emis_bins& b = m.rad;
    const int nr = b.nr, nphi = m.nphi;
    const int ncell = nr * nphi;
    const int words = kIllumPlanes * ncell;
    if (USE_LDS) {
        for (int w = threadIdx.x; w < words; w += kBlock) lds[w] = 0;
        __syncthreads();
    }
    double* planes = USE_LDS ? lds : out;
    const double log_dr = kr_log(b.dr);
    double n_disc = 0, n_binned = 0;
    // whole workgroups stride over the records, so that all 64 lanes of a wave reach the grouped adds together; a lane beyond n adds nothing
    for (long long base = blockIdx.x * (long long) kBlock; base < n; base += (long long) gridDim.x * kBlock) {
        const long long i = base + threadIdx.x;
        int32_t cell = -1;
        double g = 0, t = 0;
        if (i < n) {
            kr_ray_f64* ray = &rays[i];
            const int steps = ray->steps;
            double r, theta, phi;
            if (FUSED) {
                const kr_ray_f64 v = geodesic_of(ray);
                phi = wrap_phi(ray, steps, lo, hi);
                g = redshift_value(v, spin, V, reverse, projradius, motion);
                ray->redshift = g;
                r = v.r; theta = v.theta;
            } else {
                r = ray->r; theta = ray->theta; phi = ray->phi;
                g = ray->redshift;
            }
            t = ray->t;
            // the filter and the radial rule of emissivity_accumulate (kr_post_device.hpp), word for word
            if (steps > 0) {
                const double z = r * kr_cos(theta);
                if (z < 1E-2 && g > 0 && r >= b.r_isco) {
                    n_disc += 1;
                    const double q = b.logbin ? kr_log(r / b.r_min) / log_dr : (r - b.r_min) / b.dr;
                    if (q > -1 && q < nr) {
                        int32_t ip = 0;
                        bool ok = true;
                        if (nphi != 1) {
                            // the wrap of CellGrid::cell_of (kr_recorder.hpp); q_ph can round up to nphi itself: the last cell
                            const double p = phi + m.phi_shift;
                            const double phi_w = p - (2 * kPi) * floor((p + kPi) / (2 * kPi));
                            const double q_ph = (phi_w + kPi) / dphi;
                            ok = q_ph >= 0;                      // (a NaN fails; an infinite phi gives a NaN phi_w)
                            if (ok) ip = q_ph < nphi ? (int32_t) q_ph : nphi - 1;
                        }
                        if (ok) {
                            const int32_t c = (int32_t) q * nphi + ip;
                            if (c >= 0 && c < ncell) { cell = c; n_binned += 1; }
                        }
                    }
                }
            }
        }
        double flux = 0, emis = 0;
        if (cell >= 0) {
            flux = 1 / (b.num_primary_rays * kr_pow(g, 1.0));
            emis = 1 / kr_pow(g, b.gamma);
        }
        if (!USE_LDS) {
            int32_t key = cell;
            for_lane_groups<kAggRounds>(key, [&](int32_t k, bool same, int lanes) {
                const double s_flux = wave_sum(same ? flux : 0.0), s_emis = wave_sum(same ? emis : 0.0);
                const double s_g = wave_sum(same ? g : 0.0), s_t = wave_sum(same ? t : 0.0);
                if ((threadIdx.x & 63) == 0) {
                    atomicAdd(&planes[k], (double) lanes);
                    atomicAdd(&planes[ncell + k], s_flux);
                    atomicAdd(&planes[2 * ncell + k], s_emis);
                    atomicAdd(&planes[3 * ncell + k], s_g);
                    atomicAdd(&planes[4 * ncell + k], s_t);
                }
            });
            cell = key;                                  // (>= 0 only in the lanes that add for themselves)
        }
        if (cell >= 0) {
            atomicAdd(&planes[cell], 1.0);
            atomicAdd(&planes[ncell + cell], flux);
            atomicAdd(&planes[2 * ncell + cell], emis);
            atomicAdd(&planes[3 * ncell + cell], g);
            atomicAdd(&planes[4 * ncell + cell], t);
        }
    }
    double acc[kIllumScalars] = {n_disc, n_binned};
#pragma unroll
    for (int k = 0; k < kIllumScalars; k++) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();                             // the tallies' partial sums and, with USE_LDS, every wave's additions
    if (threadIdx.x < kIllumScalars) {
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

template <bool FUSED>
int illum_launch(const kr_illum_bins* m, void* d, int64_t n, void* d_out, hipStream_t st, double spin, double V, int reverse, int projradius, int motion, double lo,
                 double hi)
{
    if (n <= 0) return KR_OK;
    const int ncell = m->rad.nr * m->nphi;
    const double dphi = 2 * M_PI / m->nphi;
    const int grid = grid_for(n, kBlock, kCapHist);
    if (ncell <= kIllumLdsCells)
        hipLaunchKernelGGL((illum_kernel<true, FUSED>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *m, dphi, (double*) d_out, spin, V, reverse,
                           projradius, motion, lo, hi);
    else
        hipLaunchKernelGGL((illum_kernel<false, FUSED>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *m, dphi, (double*) d_out, spin, V, reverse,
                           projradius, motion, lo, hi);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace

int illum_validate(const kr_illum_bins* m, const char* who)
{
    if (!m) return invalid_arg(who, "null bins");
    if (m->rad.nr < 1) return invalid_arg(who, "nr must be positive");
    if (m->nphi < 1) return invalid_arg(who, "nphi must be positive");
    if ((int64_t) m->rad.nr * m->nphi > kIllumMaxCells) return invalid_arg(who, "nr * nphi must not exceed 2^20");
    if (!std::isfinite(m->phi_shift)) return invalid_arg(who, "phi_shift must be finite");
    return KR_OK;
}

int64_t illum_words(const kr_illum_bins* m) { return (int64_t) kIllumPlanes * m->rad.nr * m->nphi + kIllumScalars; }

// ---- the map as a table of the line and the response (kr_illum_table; the device side is IllumTab, kr_disc_pass.hpp) ------------------------------
int illum_table_validate(const kr_illum_table* t, const char* who)
{
    if (!t) return invalid_arg(who, "null table");
    if (!t->emis) return invalid_arg(who, "the table needs emis");
    if (t->nr < 1) return invalid_arg(who, "table nr must be positive");
    if (t->nphi < 1) return invalid_arg(who, "table nphi must be positive");
    if ((int64_t) t->nr * t->nphi > kIllumMaxCells) return invalid_arg(who, "table nr * nphi must not exceed 2^20");
    if (!std::isfinite(t->r_min) || !std::isfinite(t->dr) || !std::isfinite(t->phi_shift)) return invalid_arg(who, "non-finite table r_min, dr or phi_shift");
    return KR_OK;
}

int illum_table_dev(const kr_illum_table* t, TablePins& pins, IllumTab<true>* T)
{
    const size_t ncell = (size_t) t->nr * t->nphi;
    T->r_min = t->r_min; T->dr = t->dr; T->phi_shift = t->phi_shift;
    T->log_dr = t->logbin ? std::log(t->dr) : 0;
    T->dphi = 2 * M_PI / t->nphi;
    T->nr = t->nr; T->nphi = t->nphi; T->logbin = t->logbin;
    T->time = nullptr;
    auto plane = [&](TableKind kind, const double* host, const double** dev) {
        const std::string key((const char*) host, ncell * sizeof(double));
        return pins.lookup(kind, key, [&](std::vector<double>& h) { h.assign(host, host + ncell); }, dev);
    };
    int rc = plane(kIllumEmisTable, t->emis, &T->emis);
    if (rc == KR_OK && t->time) rc = plane(kIllumTimeTable, t->time, &T->time);
    return rc;
}

int reduce_illum_dev(const kr_illum_bins* m, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return illum_launch<false>(m, const_cast<void*>(d), n, d_out, st, 0.0, 0.0, 0, 0, 0, 0.0, 0.0);
}

int post_illum_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_illum_bins* m, void* d, int64_t n, void* d_out,
                   hipStream_t st)
{
    return illum_launch<true>(m, d, n, d_out, st, spin, V, reverse, projradius, motion, lo, hi);
}

}  // namespace kr
