// kr_return_map.hip -- the landing map of the returning radiation (kr_return_map, include/kr_trace.h): per source radius the classification of
// disc_source_photonfrac_r.cpp:97-126 and, in the same pass over the records, a weighted radial histogram of the rays that come back to the
// disc -- where they land, with which energy shift (the program's redshift(-1), :94, which it computes and never reads) and after how long.
// One body for the reducing form (records read only) and the fused form (range_phi + redshift + classification + histogram, each record loaded
// once and left bit for bit as kr_range_phi_dev_f64 + kr_redshift_dev_f64 leave it); a single-item kernel and a multi-item one (items in the
// kernel arguments, blockIdx.y picks the item) for the hundred radii of a sweep.
// The five planes are accumulated per workgroup in LDS (ds_add_f64) when nr <= kMaxLdsBins and flushed with one global atomic per non-zero
// word; the six scalars go wave shuffle -> LDS -> one atomic per word and workgroup, as in reduce_return_body (kr_post.hip).

#include <hip/hip_runtime.h>

#include <string>

#include "kr_pass.hpp"
#include "kr_crmath.hpp"

namespace kr {

namespace {

constexpr int kMapScalars = 6;                   // ray_count, return, escape, lost, on_disc, binned

// out = [count | weight | flux | emis | time](nr each) + the six scalars.  lds: 5 * kMaxLdsBins doubles of the workgroup when USE_LDS (unused otherwise);
// part: the workgroup's scratch of the scalar reduction
template <bool USE_LDS, bool FUSED>
KR_DEV void return_map_body(kr_ray_f64* __restrict__ rays, long long n, const kr_return_map& m, double* __restrict__ out, double spin, double V, int reverse,
                            int projradius, int motion, double lo, double hi, double* lds, double (*part)[kMapScalars])
{
    const kr_return_bins& b = m.cls;
    const int nr = m.nr;
    const int words = 5 * nr;
    if (USE_LDS) {
        for (int w = threadIdx.x; w < words; w += kBlock) lds[w] = 0;
        __syncthreads();
    }
    double* planes = USE_LDS ? lds : out;
    const double log_dr = kr_log(m.dr);
    double acc[kMapScalars] = {0, 0, 0, 0, 0, 0};
    KR_GRID_STRIDE(i, n) {
        kr_ray_f64* ray = &rays[i];
        const int steps = ray->steps;
        double phi, g;
        const double r = ray->r, theta = ray->theta;
        if (FUSED) {
            const kr_ray_f64 v = geodesic_of(ray);
            phi = wrap_phi(ray, steps, lo, hi);
            g = redshift_value(v, spin, V, reverse, projradius, motion);
            ray->redshift = g;
        } else {
            phi = ray->phi;
            g = ray->redshift;
        }
        if (!(steps > 0)) continue;
        const double alpha = krcr::kr_acos_cr(ray->alpha);  // rays[].alpha holds cos(alpha)
        const double sasb = kr_abs(kr_sin(alpha) * kr_sin(ray->beta));
        double w = b.plane_iso ? sasb : 1;
        if (b.limb) w *= 1 + 2.06 * sasb;
        acc[0] += b.weight_norm ? w : 1;
        if (theta >= kPi2 && r >= b.r_isco && r < b.r_disc) {
            if (kr_abs(r - b.source_r) > 0.1 * b.source_r || kr_abs(phi - b.source_phi) > 0.1) {
                acc[1] += w;
                acc[4] += 1;
                // the index rule of kr_emis_bins on the floating quotient (emissivity_accumulate, kr_post_device.hpp): NaN fails, (-1, 0] is bin 0
                const double q = m.logbin ? kr_log(r / m.r_min) / log_dr : (r - m.r_min) / m.dr;
                if (g > 0 && q > -1 && q < nr) {
                    const int ir = (int) q;
                    atomicAdd(&planes[ir], 1.0);
                    atomicAdd(&planes[nr + ir], w);
                    atomicAdd(&planes[2 * nr + ir], w / g);
                    atomicAdd(&planes[3 * nr + ir], w / kr_pow(g, m.gamma));
                    atomicAdd(&planes[4 * nr + ir], w * ray->t);
                    acc[5] += 1;
                }
            }
        } else if (r > b.r_esc) {
            acc[2] += w;
        } else if (r < b.r_isco) {
            acc[3] += w;
        }
    }
#pragma unroll
    for (int k = 0; k < kMapScalars; k++) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();                             // the scalars' partial sums and, with USE_LDS, every wave's histogram additions
    if (threadIdx.x < kMapScalars) {
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
return_map_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_return_map m, double* __restrict__ out, double spin, double V, int reverse, int projradius,
                  int motion, double lo, double hi)
{
    __shared__ double lds[USE_LDS ? 5 * kMaxLdsBins : 1];
    __shared__ double part[kBlock / 64][kMapScalars];
    return_map_body<USE_LDS, FUSED>(rays, n, m, out, spin, V, reverse, projradius, motion, lo, hi, lds, part);
}

// several radii in one launch.  24 items of 88 + 24 bytes and the scalars stay below the 4 KB a kernel's arguments may take (32 would not).
struct MapItem {
    kr_return_map m;
    kr_ray_f64* rays;
    long long n;
    double* out;
};
constexpr int kMapChunk = 24;
struct MapChunk { MapItem item[kMapChunk]; };

// The items of a chunk may have different nr: each workgroup takes the LDS body when ITS item fits and the global one otherwise (a branch that
// is uniform over the workgroup), so one item beyond the capacity costs the others of its chunk nothing.
__global__ void __launch_bounds__(kBlock)
return_map_multi_kernel(MapChunk c, double spin, double V, int reverse, int projradius, int motion, double lo, double hi)
{
    __shared__ double lds[5 * kMaxLdsBins];
    __shared__ double part[kBlock / 64][kMapScalars];
    const MapItem& it = c.item[blockIdx.y];
    const kr_return_map m = it.m;
    if (m.nr <= kMaxLdsBins) return_map_body<true, true>(it.rays, it.n, m, it.out, spin, V, reverse, projradius, motion, lo, hi, lds, part);
    else return_map_body<false, true>(it.rays, it.n, m, it.out, spin, V, reverse, projradius, motion, lo, hi, lds, part);
}

}  // namespace

int return_map_validate(const kr_return_map* m, const char* who)
{
    if (!m) { set_error(std::string(who) + ": null map"); return KR_EINVAL; }
    if (m->nr <= 0) { set_error(std::string(who) + ": nr must be positive"); return KR_EINVAL; }
    return KR_OK;
}

int reduce_return_map_dev(const kr_return_map* m, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    const int grid = grid_for(n, kBlock, kCapHist);
    if (m->nr <= kMaxLdsBins)
        hipLaunchKernelGGL((return_map_kernel<true, false>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *m, (double*) d_out, 0.0, 0.0, 0, 0, 0, 0.0, 0.0);
    else
        hipLaunchKernelGGL((return_map_kernel<false, false>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *m, (double*) d_out, 0.0, 0.0, 0, 0, 0, 0.0, 0.0);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int post_return_map_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_return_map* m, void* d, int64_t n, void* d_out,
                        hipStream_t st)
{
    if (n <= 0) return KR_OK;
    const int grid = grid_for(n, kBlock, kCapHist);
    if (m->nr <= kMaxLdsBins)
        hipLaunchKernelGGL((return_map_kernel<true, true>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *m, (double*) d_out, spin, V, reverse, projradius,
                           motion, lo, hi);
    else
        hipLaunchKernelGGL((return_map_kernel<false, true>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *m, (double*) d_out, spin, V, reverse, projradius,
                           motion, lo, hi);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int post_return_map_batch_dev(int count, double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_return_map* m, void* const* d,
                              const int64_t* n, void* const* d_out, hipStream_t st)
{
    static_assert(sizeof(MapItem) == 112 && sizeof(MapChunk) + 48 <= 3840, "kernel arguments are limited to 4 KB");
    // 4096 workgroups over a chunk: the 1024 that 40 KB of LDS each let the GPU hold at once, four times over; every one flushes its histogram
    return launch_chunked<MapChunk>(count, n, 4096, st, [&](int i, TablePins&, MapItem* it) {
        *it = MapItem{m[i], (kr_ray_f64*) d[i], (long long) n[i], (double*) d_out[i]};
        return (int) KR_OK;
    }, return_map_multi_kernel, spin, V, reverse, projradius, motion, lo, hi);
}

}  // namespace kr
