// kr_line.hip -- emission-line profiles and reverberation transfer functions from image-plane traces (include/kr_trace.h, kr_line_bins).
// The reference builds the line outside its C++ (python/line_from_image.ipynb: ENSHIFT and RADIUS planes of the image FITS file, weight
// emis(r) enshift^3, summed into energy bins); here the rays (or the raw image planes) are binned where they already are, in HBM, and only
// the 2 nt ne + 2 doubles of the histogram leave the device.
//   reduce_line_kernel      records after redshift(-1, reverse=1) -> line bins
//   post_line_kernel        redshift + range_phi + line bins in one pass (the sibling of post_image_kernel; same per-ray functions)
//   post_line_limb_kernel   the same with the weight times a limb law of the emission angle mu in the disc frame (kr_limb_law; frame_value)
//                           ILLUM: emis and the source -> disc time from an (r, phi) table (kr_illum_table; IllumTab, kr_disc_pass.hpp), here and
//                           in reduce_line_kernel
//   post_line_stokes_kernel the limb-law line with the Stokes parameters I, Q, U of the polarised emission per bin (kr_pol_law; polar_value)
//   line_from_image_kernel  raw-sum image planes (kr_reduce_image_dev_f64 layout) -> line bins, per pixel
// All of them are streaming passes, one record / pixel per work-item.  The histogram is privatised per workgroup in LDS when it fits
// kLineLdsWords (ds_add_f64), flushed with one global atomic per non-zero word; above that the items add into the global histogram directly.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "kr_disc_pass.hpp"

namespace kr {

namespace {

// Per-workgroup LDS budget of the privatised histogram: 4096 doubles = 32 KiB, i.e. ne nt <= 2047.  Registers bound the residency first
// (-Rpass-analysis=kernel-resource-usage, gfx950: post_line and post_line_limb 194 VGPRs -> 2 waves / SIMD = 2 workgroups / CU, reduce_line 144 -> 3,
// line_from_image 109 -> 4), and 4 x 32 KiB fit the CU's 160 KiB: the LDS never lowers the occupancy of any of the three; a 64-KiB
// budget would halve line_from_image's.
constexpr int kLineLdsWords = 4096;

// what the kernels need besides the records: the bins by value (their host table pointers are never dereferenced on the device), the
// device copy of the table, and the two logarithms of the bin ratios (taken once, on the host)
struct LineDev {
    kr_line_bins b;
    const double* t_emis;      // [table_nr] on the device, or null: powerlaw3
    const double* t_time;      // [table_nr] on the device, or null
    double log_de, log_tdr;
    int time_axis;             // 0: j = 0 for every item (nt == 1, dt <= 0)
    int words;                 // 2 nt ne + 2
};

// one item that passed the filter -> at most one bin k = j ne + i and its weight w; false: the item is not binned.  PIXEL: x is the pixel's mean 1/g
// (E = line_energy x, w = emis x^g_index); otherwise x is g (E = line_energy / g, w = emis g^-g_index).  LIMB: w times `limb`.
// ILLUM: emis and tt from the cell of the (r, phi) table T that holds the record (the bins carry no radial table then)
template <bool PIXEL, bool LIMB, bool ILLUM = false>
KR_DEV bool line_item(const LineDev& L, double r, double x, double t, double limb, int* k, double* w, [[maybe_unused]] const IllumTab<ILLUM>& T = IllumTab<ILLUM>{},
                      [[maybe_unused]] double phi = 0)
{
    const kr_line_bins& b = L.b;
    double emis, tt = 0;
    if constexpr (ILLUM) {
        if (!illum_table_entry(T, r, phi, &emis, &tt)) return false;
    } else if (L.t_emis) {
        int ir;
        if (!radial_table_index(b.table_logbin, b.table_r_min, b.table_dr, L.log_tdr, b.table_nr, r, &ir)) return false;
        emis = L.t_emis[ir];
        if (!__builtin_isfinite(emis)) return false;
        if (L.t_time) tt = L.t_time[ir];
    } else {
        emis = powerlaw3(r, b.q1, b.rb1, b.q2, b.rb2, b.q3);
    }
    const double E = PIXEL ? b.line_energy * x : b.line_energy / x;
    const double w0 = emis * (PIXEL ? kr_pow(x, b.g_index) : kr_pow(x, -1 * b.g_index));
    *w = LIMB ? w0 * limb : w0;
    const double fe = energy_bin_coord(b.log_e, b.e_min, b.de, L.log_de, E);
    if (!(fe >= 0 && fe < b.ne)) return false;          // NaN fails too
    int j = 0;
    if (L.time_axis) {
        const double ft = (t + tt - b.t0) / b.dt;
        if (!(ft >= 0 && ft < b.nt)) return false;
        j = (int) ft;
    }
    *k = j * b.ne + (int) fe;
    return true;
}

// the item into [count | flux].  Returns 1 if the item was binned.
template <bool PIXEL, bool LIMB = false, bool ILLUM = false>
KR_DEV unsigned line_accumulate(double* acc, const LineDev& L, double r, double x, double t, double limb = 1, const IllumTab<ILLUM>& T = IllumTab<ILLUM>{}, double phi = 0)
{
    int k;
    double w;
    if (!line_item<PIXEL, LIMB, ILLUM>(L, r, x, t, limb, &k, &w, T, phi)) return 0;
    atomicAdd(&acc[k], 1.0);
    atomicAdd(&acc[L.b.nt * L.b.ne + k], w);
    return 1;
}

template <bool USE_LDS>
KR_DEV double* line_begin(double* lds, double* out, int words)
{
    if (!USE_LDS) return out;
    for (int w = threadIdx.x; w < words; w += kBlock) lds[w] = 0;
    __syncthreads();
    return lds;
}

// the tallies close the histogram: on_disc, binned and -- the limb pass, whose `words` count one more -- bad_angle
template <bool USE_LDS, bool LIMB = false>
KR_DEV void line_end(double* lds, double* out, int words, unsigned long long on_disc, unsigned long long binned, unsigned long long bad_angle = 0)
{
    double* acc = USE_LDS ? lds : out;
    const int tallies = words - (LIMB ? 3 : 2);
    if (on_disc) atomicAdd(&acc[tallies], (double) on_disc);
    if (binned) atomicAdd(&acc[tallies + 1], (double) binned);
    if (LIMB && bad_angle) atomicAdd(&acc[tallies + 2], (double) bad_angle);
    if (USE_LDS) {
        __syncthreads();
        for (int w = threadIdx.x; w < words; w += kBlock)
            if (lds[w] != 0) atomicAdd(&out[w], lds[w]);
    }
}

// SURFACE: the records landed on a surface (disc_filter_surface, kr_disc_pass.hpp), the radius is rho, and the layout is the limb line's with a
// bad_angle word that stays 0 (the records carry no emission angle)
template <bool USE_LDS, bool SURFACE = false, bool ILLUM = false>
__global__ void __launch_bounds__(kBlock)
reduce_line_kernel(const kr_ray_f64* __restrict__ rays, long long n, LineDev L, double* __restrict__ out, IllumTab<ILLUM> T)
{
    extern __shared__ double lds[];
    const int words = SURFACE ? L.words + 1 : L.words;
    double* acc = line_begin<USE_LDS>(lds, out, words);
    unsigned long long on_disc = 0, binned = 0;
    KR_GRID_STRIDE(i, n) {
        const kr_ray_f64* ray = &rays[i];
        const double g = ray->redshift;
        double r = ray->r;
        if constexpr (SURFACE) {
            r = r * kr_sin(ray->theta);
            if (!disc_filter_surface(L.b.r_isco, L.b.r_disc, ray->steps, ray->status, r, g)) continue;
        } else {
            if (!disc_filter(L.b.r_isco, L.b.r_disc, ray->steps, r, ray->theta, g)) continue;
        }
        on_disc++;
        if constexpr (ILLUM) binned += line_accumulate<false, false, true>(acc, L, r, g, ray->t, 1, T, ray->phi);
        else binned += line_accumulate<false>(acc, L, r, g, ray->t);
    }
    line_end<USE_LDS, SURFACE>(lds, out, words, on_disc, binned);
}

// redshift(V, reverse, projradius, motion) + range_phi(lo, hi) + the line bins: the per-ray code of post_image_kernel (kr_post.hip) with the
// seven planes replaced by the line, so rays[] ends bit-identical to the separate passes
// PLUNGE: the disc flow of KR_V_PLUNGE (DiscFlow, kr_post_device.hpp), here and in the limb-darkened line; the host picks the instance from V
template <bool USE_LDS, bool PLUNGE>
__global__ void __launch_bounds__(kBlock)
post_line_kernel(kr_ray_f64* __restrict__ rays, long long n, double spin, double V, int reverse, int projradius, int motion, double lo, double hi,
                 LineDev L, double* __restrict__ out, DiscFlow<PLUNGE> fl)
{
    extern __shared__ double lds[];
    double* acc = line_begin<USE_LDS>(lds, out, L.words);
    unsigned long long on_disc = 0, binned = 0;
    KR_GRID_STRIDE(i, n) {
        kr_ray_f64* ray = &rays[i];
        const kr_ray_f64 v = geodesic_of(ray);
        const int steps = ray->steps;
        const double g = redshift_value<PLUNGE>(v, spin, V, reverse, projradius, motion, fl);
        ray->redshift = g;
        wrap_phi(ray, steps, lo, hi);
        if (!disc_filter(L.b.r_isco, L.b.r_disc, steps, v.r, v.theta, g)) continue;
        on_disc++;
        binned += line_accumulate<false>(acc, L, v.r, g, ray->t);
    }
    line_end<USE_LDS>(lds, out, L.words, on_disc, binned);
}

// post_line_kernel with w *= limb(mu): disc_ray (kr_disc_pass.hpp) in its fused form for the orbiting observer, so rays[] ends as after
// post_line_kernel and a bad-angle ray is counted and binned by that function's rule.  Layout: post_line_kernel's, then bad_angle.
// SURFACE: the line of a disc with a surface (DiscSurface, kr_post_device.hpp): the filter, the radius and the angle of disc_ray's surface flavour
template <bool USE_LDS, bool PLUNGE, bool SURFACE = false, bool ILLUM = false>
__global__ void __launch_bounds__(kBlock)
post_line_limb_kernel(kr_ray_f64* __restrict__ rays, long long n, double spin, double V, int reverse, int projradius, double lo, double hi, LineDev L,
                      kr_limb_law law, double* __restrict__ out, DiscFlow<PLUNGE> fl, DiscSurface<SURFACE> sf, IllumTab<ILLUM> T)
{
    extern __shared__ double lds[];
    const int words = L.words + 1;
    double* acc = line_begin<USE_LDS>(lds, out, words);
    unsigned long long on_disc = 0, binned = 0, bad_angle = 0;
    KR_GRID_STRIDE(i, n) {
        kr_ray_f64* ray = &rays[i];
        DiscRay d;
        if (!disc_ray<true, PLUNGE, SURFACE>(ray, L.b.r_isco, L.b.r_disc, spin, V, reverse, projradius, 0, lo, hi, law, &d, on_disc, bad_angle, fl, sf)) continue;
        if constexpr (ILLUM) binned += line_accumulate<false, true, true>(acc, L, d.r, d.g, ray->t, d.limb, T, d.phi);
        else binned += line_accumulate<false, true>(acc, L, d.r, d.g, ray->t, d.limb);
    }
    line_end<USE_LDS, true>(lds, out, words, on_disc, binned, bad_angle);
}

// post_line_limb_kernel with the Stokes parameters of the polarised line (include/kr_trace.h, kr_pol_law): g, mu and the polarisation angle at the
// observer come from ONE metric and momentum evaluation (polar_value; its E is redshift_value's recv to the bit, so rays[] ends as after
// post_line_kernel).  An item adds 1, w, w delta c2, w delta s2 to its bin.  A bad-pol ray that passed the filter counts in on_disc and bad_pol and is
// never binned, whatever the limb law.  Layout: [count | I | Q | U](nt ne each) + on_disc, binned, bad_pol.
template <bool USE_LDS>
__global__ void __launch_bounds__(kBlock)
post_line_stokes_kernel(kr_ray_f64* __restrict__ rays, long long n, double spin, double V, int reverse, int projradius, double lo, double hi, double sin_incl,
                        LineDev L, kr_limb_law limb, kr_pol_law pol, double* __restrict__ out)
{
    extern __shared__ double lds[];
    const int plane = L.b.nt * L.b.ne, words = 4 * plane + 3;
    double* acc = line_begin<USE_LDS>(lds, out, words);
    unsigned long long on_disc = 0, binned = 0, bad_pol = 0;
    KR_GRID_STRIDE(i, n) {
        kr_ray_f64* ray = &rays[i];
        const kr_ray_f64 v = polar_record_of(ray);
        const int steps = ray->steps;
        const Polar q = polar_value(v, spin, V, reverse, projradius, sin_incl);
        const double g = q.redshift;
        ray->redshift = g;
        wrap_phi(ray, steps, lo, hi);
        if (!disc_filter(L.b.r_isco, L.b.r_disc, steps, v.r, v.theta, g)) continue;
        on_disc++;
        if (q.bad) { bad_pol++; continue; }
        int k;
        double w;
        if (!line_item<false, true>(L, v.r, g, ray->t, limb_weight(limb.law, limb.coeff, q.mu), &k, &w)) continue;
        binned++;
        const double wd = w * pol_degree(pol.law, pol.coeff, q.mu);
        atomicAdd(&acc[k], 1.0);
        atomicAdd(&acc[plane + k], w);
        atomicAdd(&acc[2 * plane + k], wd * q.c2);
        atomicAdd(&acc[3 * plane + k], wd * q.s2);
    }
    line_end<USE_LDS, true>(lds, out, words, on_disc, binned, bad_pol);
}

// planes: [nrays | flux | r | phi | enshift | time | emis](npix each) + disc_count, raw sums (kr_reduce_image_dev_f64)
template <bool USE_LDS>
__global__ void __launch_bounds__(kBlock)
line_from_image_kernel(const double* __restrict__ planes, long long npix, LineDev L, double* __restrict__ out)
{
    extern __shared__ double lds[];
    double* acc = line_begin<USE_LDS>(lds, out, L.words);
    unsigned long long on_disc = 0, binned = 0;
    KR_GRID_STRIDE(p, npix) {
        const double nrays = planes[p];
        if (!(nrays > 0)) continue;
        on_disc++;
        const double e = planes[4 * npix + p] / nrays, r = planes[2 * npix + p] / nrays, t = planes[5 * npix + p] / nrays;
        binned += line_accumulate<true>(acc, L, r, e, t);
    }
    line_end<USE_LDS>(lds, out, L.words, on_disc, binned);
}

// ---- the radial table on the device: one array [emis | time] per distinct contents in the device table store (TablePins, kr_common.hpp), built by
//      the first call that needs it (hipMalloc and a blocking copy), kept while the device's store has room, freed only when no call holds it and
//      the device has drained.  Pinned in `pins`: keep it until the kernel that reads the table has been enqueued. ------------------------------
int line_dev(const kr_line_bins* b, TablePins& pins, LineDev* L)
{
    L->b = *b;
    L->log_de = b->log_e ? std::log(b->de) : 0;
    L->log_tdr = b->table_emis && b->table_logbin ? std::log(b->table_dr) : 0;
    L->time_axis = !(b->nt == 1 && b->dt <= 0);
    L->words = 2 * b->nt * b->ne + 2;
    L->t_emis = L->t_time = nullptr;
    if (!b->table_emis) return KR_OK;
    const size_t nr = (size_t) b->table_nr;
    std::string key((const char*) b->table_emis, nr * sizeof(double));
    if (b->table_time) key.append((const char*) b->table_time, nr * sizeof(double));
    key.push_back(b->table_time ? 2 : 1);
    const int rc = pins.lookup(kLineTable, key, [&](std::vector<double>& h) {
        h.assign(b->table_emis, b->table_emis + nr);
        if (b->table_time) h.insert(h.end(), b->table_time, b->table_time + nr);
    }, &L->t_emis);
    if (rc == KR_OK && b->table_time) L->t_time = L->t_emis + nr;
    return rc;
}

}  // namespace

int line_validate(const kr_line_bins* b, const char* who)
{
    auto bad = [&](const char* why) { set_error(std::string(who) + ": " + why); return KR_EINVAL; };
    if (!b) return bad("null bins");
    const double params[] = {b->line_energy, b->e_min, b->de, b->t0, b->dt, b->r_isco, b->r_disc, b->q1, b->rb1, b->q2, b->rb2, b->q3, b->g_index};
    for (double v : params)
        if (!std::isfinite(v)) return bad("non-finite bin parameter");
    if (b->ne < 1 || b->nt < 1) return bad("ne and nt must be >= 1");
    if ((int64_t) b->ne * b->nt > ((int64_t) 1 << 24)) return bad("ne * nt must not exceed 2^24");
    if (const int rc = energy_axis_validate(bad, b->de, b->log_e, b->e_min)) return rc;
    if (b->nt > 1 && !(b->dt > 0)) return bad("nt > 1 needs dt > 0");
    if (b->table_time && !b->table_emis) return bad("table_time given without table_emis");
    if (b->table_emis) {
        if (b->table_nr < 1) return bad("table_nr must be >= 1 with a table");
        if (!std::isfinite(b->table_r_min) || !std::isfinite(b->table_dr)) return bad("non-finite bin parameter");
    }
    return KR_OK;
}

int reduce_line_dev(const kr_line_bins* b, const void* d, int64_t n, void* d_line, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    LineDev L;
    int rc = line_dev(b, pins, &L);
    if (rc != KR_OK) return rc;
    KR_LAUNCH_LDS_OR_GLOBAL(reduce_line_kernel, L.words <= kLineLdsWords, grid_for(n, kBlock, kCapHist), L.words * sizeof(double), st, (const kr_ray_f64*) d,
                            (long long) n, L, (double*) d_line, IllumTab<false>{});
    return KR_OK;
}

int post_line_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_line_bins* b, void* d, int64_t n,
                  void* d_line, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    LineDev L;
    int rc = line_dev(b, pins, &L);
    if (rc != KR_OK) return rc;
    KR_LAUNCH_LDS_OR_GLOBAL_FLOW(post_line_kernel, spin, V, reverse, L.words <= kLineLdsWords, grid_for(n, kBlock, kCapHist), L.words * sizeof(double), st, (kr_ray_f64*) d,
                                 (long long) n, spin, V, reverse, projradius, motion, lo, hi, L, (double*) d_line);
    return KR_OK;
}

int post_line_limb_dev(double spin, double V, int reverse, int projradius, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law, void* d, int64_t n,
                       void* d_line, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    LineDev L;
    int rc = line_dev(b, pins, &L);
    if (rc != KR_OK) return rc;
    const int grid = grid_for(n, kBlock, kCapHist);
    for_flow(spin, V, reverse, [&](auto flow) {
        constexpr bool P = decltype(flow)::plunge;
        if (L.words + 1 <= kLineLdsWords)
            hipLaunchKernelGGL((post_line_limb_kernel<true, P>), dim3(grid), dim3(kBlock), (L.words + 1) * sizeof(double), st, (kr_ray_f64*) d, (long long) n, spin, V, reverse,
                               projradius, lo, hi, L, *law, (double*) d_line, flow.arg, DiscSurface<false>{}, IllumTab<false>{});
        else
            hipLaunchKernelGGL((post_line_limb_kernel<false, P>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, spin, V, reverse, projradius, lo, hi, L, *law,
                               (double*) d_line, flow.arg, DiscSurface<false>{}, IllumTab<false>{});
    });
    KR_LAUNCH_CHECK();
    return KR_OK;
}

// the surface forms (kr_post_line_surface_dev_f64, kr_reduce_line_surface_dev_f64): the Keplerian observer at rho, whatever the flat form's V would say
int post_line_surface_dev(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law, void* d, int64_t n,
                          void* d_line, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    LineDev L;
    int rc = line_dev(b, pins, &L);
    if (rc != KR_OK) return rc;
    const int grid = grid_for(n, kBlock, kCapHist);
    const DiscSurface<true> sf = surface_dev(s);
    if (L.words + 1 <= kLineLdsWords)
        hipLaunchKernelGGL((post_line_limb_kernel<true, false, true>), dim3(grid), dim3(kBlock), (L.words + 1) * sizeof(double), st, (kr_ray_f64*) d, (long long) n, spin, -1.0,
                           reverse, 1, lo, hi, L, *law, (double*) d_line, DiscFlow<false>{}, sf, IllumTab<false>{});
    else
        hipLaunchKernelGGL((post_line_limb_kernel<false, false, true>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, spin, -1.0, reverse, 1, lo, hi, L, *law,
                           (double*) d_line, DiscFlow<false>{}, sf, IllumTab<false>{});
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int reduce_line_surface_dev(const kr_line_bins* b, const void* d, int64_t n, void* d_line, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    LineDev L;
    int rc = line_dev(b, pins, &L);
    if (rc != KR_OK) return rc;
    const int grid = grid_for(n, kBlock, kCapHist);
    if (L.words + 1 <= kLineLdsWords)
        hipLaunchKernelGGL((reduce_line_kernel<true, true>), dim3(grid), dim3(kBlock), (L.words + 1) * sizeof(double), st, (const kr_ray_f64*) d, (long long) n, L, (double*) d_line,
                           IllumTab<false>{});
    else
        hipLaunchKernelGGL((reduce_line_kernel<false, true>), dim3(grid), dim3(kBlock), 0, st, (const kr_ray_f64*) d, (long long) n, L, (double*) d_line, IllumTab<false>{});
    KR_LAUNCH_CHECK();
    return KR_OK;
}

// the forms with an (r, phi) illumination table (kr_post_line_illum_dev_f64, kr_reduce_line_illum_dev_f64): the limb-law line and the reducing line with
// emis and the source -> disc time read from the table's cell
int post_line_illum_dev(double spin, double V, int reverse, int projradius, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law, const kr_illum_table* t,
                        void* d, int64_t n, void* d_line, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    LineDev L;
    IllumTab<true> T;
    int rc = line_dev(b, pins, &L);
    if (rc == KR_OK) rc = illum_table_dev(t, pins, &T);
    if (rc != KR_OK) return rc;
    const int grid = grid_for(n, kBlock, kCapHist);
    if (L.words + 1 <= kLineLdsWords)
        hipLaunchKernelGGL((post_line_limb_kernel<true, false, false, true>), dim3(grid), dim3(kBlock), (L.words + 1) * sizeof(double), st, (kr_ray_f64*) d, (long long) n, spin, V,
                           reverse, projradius, lo, hi, L, *law, (double*) d_line, DiscFlow<false>{}, DiscSurface<false>{}, T);
    else
        hipLaunchKernelGGL((post_line_limb_kernel<false, false, false, true>), dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, spin, V, reverse, projradius, lo,
                           hi, L, *law, (double*) d_line, DiscFlow<false>{}, DiscSurface<false>{}, T);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int reduce_line_illum_dev(const kr_line_bins* b, const kr_illum_table* t, const void* d, int64_t n, void* d_line, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    LineDev L;
    IllumTab<true> T;
    int rc = line_dev(b, pins, &L);
    if (rc == KR_OK) rc = illum_table_dev(t, pins, &T);
    if (rc != KR_OK) return rc;
    const int grid = grid_for(n, kBlock, kCapHist);
    if (L.words <= kLineLdsWords)
        hipLaunchKernelGGL((reduce_line_kernel<true, false, true>), dim3(grid), dim3(kBlock), L.words * sizeof(double), st, (const kr_ray_f64*) d, (long long) n, L, (double*) d_line, T);
    else
        hipLaunchKernelGGL((reduce_line_kernel<false, false, true>), dim3(grid), dim3(kBlock), 0, st, (const kr_ray_f64*) d, (long long) n, L, (double*) d_line, T);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

int post_line_stokes_dev(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_line_bins* b, const kr_limb_law* limb,
                         const kr_pol_law* pol, void* d, int64_t n, void* d_out, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    LineDev L;
    int rc = line_dev(b, pins, &L);
    if (rc != KR_OK) return rc;
    const int64_t words = 4 * (int64_t) b->nt * b->ne + 3;
    KR_LAUNCH_LDS_OR_GLOBAL(post_line_stokes_kernel, words <= kLineLdsWords, grid_for(n, kBlock, kCapHist), (size_t) words * sizeof(double), st, (kr_ray_f64*) d,
                            (long long) n, spin, V, reverse, projradius, lo, hi, sin_inclination(inc_deg), L, *limb, *pol, (double*) d_out);
    return KR_OK;
}

int line_from_image_dev(const kr_line_bins* b, const kr_image_bins* ib, const void* d_planes, void* d_line, hipStream_t st)
{
    const long long npix = (long long) ib->img_nx * ib->img_ny;
    TablePins pins;
    LineDev L;
    int rc = line_dev(b, pins, &L);
    if (rc != KR_OK) return rc;
    KR_LAUNCH_LDS_OR_GLOBAL(line_from_image_kernel, L.words <= kLineLdsWords, grid_for(npix, kBlock, kCapHist), L.words * sizeof(double), st,
                            (const double*) d_planes, npix, L, (double*) d_line);
    return KR_OK;
}

}  // namespace kr
