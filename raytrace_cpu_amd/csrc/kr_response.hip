// kr_response.hip -- the reverberation response of the disc from image-plane traces (include/kr_trace.h, kr_response_model): the energy-time impulse
// response of a whole tabulated rest-frame spectrum.  Every disc ray adds to EVERY output energy of ONE time row, so neither two-phase kernel fits as it
// stands: in kr_spectrum.hip a lane's sum never leaves its register until the launch ends, in kr_hotspot.hip the lane owns a time sample.  Here, per tile
// of kBlock records:
//   phase A  kr_spectrum.hip's, plus the time row: one RECORD per lane, disc_ray (kr_disc_pass.hpp), then the item {g, u_g, w g^-3, zone, j} placed by
//            tile_compact and then ordered by j (a stable rank over the tile's at most kBlock keys, in LDS).  A used record outside the time window
//            is counted and not made live.
//   phase B  one ENERGY per lane and slot walks the tile's items.  An item's row j is uniform across the workgroup, so a lane keeps sum[SLOTS] and the
//            current row j_cur in registers: while the items stay in one row nothing leaves the registers.  When an item's j differs from j_cur the
//            lane adds its non-zero sums into resp[j_cur ne + e] -- one f64 global atomic per lane and slot, the lanes of a wave on consecutive
//            addresses -- and starts the new row.  The last row is flushed at kernel exit; j_cur lives across the tiles, which a workgroup takes as one
//            contiguous run, so the last row of a tile is often the first of the next.
//   response_kernel<MODEL, FUSED, SLOTS>   SLOTS <= 8 energies per lane: a launch covers the energies [e0, e1), at most 2048 of them.  MODEL 1: S in
//                                          LDS; 2: S in global memory (the budget of kr_spectrum.hip).  FUSED: redshift + range_phi + response (rays[]
//                                          ends as after post_line_kernel); otherwise the records carry their redshift and are only read.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "kr_spectrum_dev.hpp"

namespace kr {

namespace {

// The two design questions of the pass, settled by measurement (profiles/reverb_response_ab.txt): a tile's items are ordered by time row in LDS before
// phase B, and a workgroup takes a contiguous run of tiles, so that a row's run goes on across the tiles of neighbouring pixels.
#ifdef KR_RESPONSE_SORT                          // A/B builds only (scripts/response_ab.py): 0 leaves the items in traced order
constexpr bool kSortTile = KR_RESPONSE_SORT != 0;
#else
constexpr bool kSortTile = true;
#endif
#ifdef KR_RESPONSE_CHUNK                         // A/B builds only: 0 gives a workgroup the grid-stride tiles of kr_spectrum.hip
constexpr bool kChunkTiles = KR_RESPONSE_CHUNK != 0;
#else
constexpr bool kChunkTiles = true;
#endif

// A lane owns at most this many energies in one launch.  The sixteen-slot instance that kr_spectrum.hip compiles is not built here: it held 256 VGPRs
// and 79 AGPRs, its slot loop stayed rolled behind indexed register moves, and its one run on the device ended in a memory fault whose cause the
// compiled code did not give away; ne > kLaunchSlots kBlock takes two launches instead.
constexpr int kLaunchSlots = 8;

// the time axis and the device copy of the source -> disc time table
struct RespDev {
    double t0, dt;
    const double* t_time;      // [table_nr] on the device, or null
    int nt;
    int e0, e1;                // the energies [e0, e1) of this launch; the launch with e0 == 0 adds the tallies
};

// what both item functions end with: the item of a used record from its emissivity and source -> disc time
KR_DEV void response_item_tail(const SpecDev& D, const RespDev& R, double r, double g, double t, double limb, double emis, double tt, double g3, double* a, double* b, double* c,
                               int* zone, double* ft)
{
    const kr_spectrum_model& m = D.m;
    const double fz = m.nz * kr_log(r / m.r_isco) / D.log_span;
    *a = g;
    *zone = (int) fmin(fmax(fz, 0.0), (double) (m.nz - 1));         // (a NaN becomes zone 0)
    *b = kr_log(g) / D.log_sde;
    *c = emis * limb * g3;
    *ft = (t + tt - R.t0) / R.dt;
}

// one ray that passed the filter (and, under a law that needs it, has its angle) -> its item {a, b, c, zone} as spectrum_item<false> gives it, and the
// coordinate of its time row; false: the ray is not used.  (spectrum_item's table branch written out: ir also serves table_time, without table_emis too.)
KR_DEV bool response_item(const SpecDev& D, const RespDev& R, double r, double g, double t, double limb, double* a, double* b, double* c, int* zone, double* ft)
{
    const kr_spectrum_model& m = D.m;
    const double g3 = 1 / (g * g * g);
    int ir = 0;
    if (D.t_emis || R.t_time) {
        if (!table_index(D, r, &ir)) return false;
    }
    double emis, tt = 0;
    if (D.t_emis) {
        emis = D.t_emis[ir];
        if (!__builtin_isfinite(emis)) return false;
    } else {
        emis = powerlaw3(r, m.q1, m.rb1, m.q2, m.rb2, m.q3);
    }
    if (R.t_time) {
        tt = R.t_time[ir];
        if (!__builtin_isfinite(tt)) return false;
    }
    response_item_tail(D, R, r, g, t, limb, emis, tt, g3, a, b, c, zone, ft);
    return true;
}

// ILLUM (include/kr_trace.h, kr_illum_table): emis and the source -> disc time from the cell of an (r, phi) table that holds the record, in place of
// powerlaw3 and the radial tables, which the model then does not carry.  The table rides behind the time axis in the kernel argument R: RespArg<false>
// is RespDev itself in size and layout, so the instances without a table are the kernels they were (profiles/illum_pass_resources.txt).
template <bool ILLUM> struct RespArg : RespDev {};
template <> struct RespArg<true> : RespDev { IllumTab<true> tab; };

KR_DEV bool response_item_illum(const SpecDev& D, const RespDev& R, const IllumTab<true>& T, double r, double phi, double g, double t, double limb, double* a, double* b,
                                double* c, int* zone, double* ft)
{
    const kr_spectrum_model& m = D.m;
    const double g3 = 1 / (g * g * g);
    double emis, tt;
    if (!illum_table_entry(T, r, phi, &emis, &tt)) return false;
    response_item_tail(D, R, r, g, t, limb, emis, tt, g3, a, b, c, zone, ft);
    return true;
}

// PLUNGE: the disc flow of KR_V_PLUNGE (DiscFlow, kr_post_device.hpp), fused form only; the host picks the instance from V
// SURFACE: the response of a disc with a surface (DiscSurface, kr_post_device.hpp): the filter, the radius and the angle of disc_ray's surface flavour
template <int MODEL, bool FUSED, int SLOTS, bool PLUNGE, bool SURFACE = false, bool ILLUM = false>
__global__ void __launch_bounds__(kBlock)
response_kernel(typename std::conditional<FUSED, kr_ray_f64, const kr_ray_f64>::type* __restrict__ rays, long long n, double spin, double V, int reverse,
                int projradius, int motion, double lo, double hi, SpecDev D, RespArg<ILLUM> R, kr_limb_law law, double* __restrict__ out, DiscFlow<PLUNGE> fl,
                DiscSurface<SURFACE> sf)
{
    static_assert(!(SURFACE && PLUNGE), "the surface passes keep the Keplerian observer at rho");
    extern __shared__ double lds_s[];                    // MODEL 1: the table
    __shared__ double it_a[kBlock], it_b[kBlock], it_c[kBlock];
    __shared__ int it_z[kBlock], it_j[kBlock];
    __shared__ int it_key[kSortTile ? kBlock : 1];
    __shared__ int wave_count[kBlock / 64];
    const kr_spectrum_model& m = D.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ne = m.ne;

    // phase B's registers: the energies this lane owns (slot s: energy e0 + s kBlock + tid), their per-energy term, their sums and the row the sums belong to
    double E[SLOTS], U[SLOTS], sum[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int e = R.e0 + s * kBlock + tid;
        E[s] = e < R.e1 ? (m.log_e ? m.e_min * kr_pow(m.de, e + 0.5) : m.e_min + (e + 0.5) * m.de) : 0;      // (0: an energy beyond e1 adds nothing, and is never flushed)
        U[s] = e < R.e1 ? (kr_log(E[s]) - D.log_semin) / D.log_sde : 0;
        sum[s] = 0;
    }
    int j_cur = 0;                                       // (every sum is 0 until an item has set the row)
    // slots in which this wave owns an energy at all (wave-uniform)
    const int first = wave * 64, mine = R.e1 - R.e0;
    const int my_slots = mine > first ? min(SLOTS, (mine - first + kBlock - 1) / kBlock) : 0;
    const double* S = D.s;
    if (MODEL == 1) {
        const int words = m.nz * m.s_ne;
        for (int w = tid; w < words; w += kBlock) lds_s[w] = D.s[w];
        S = lds_s;                                       // (the first barrier of the tile loop orders these stores before phase B)
    }
    // the sums of row j_cur into the response: one atomic per lane and slot with a non-zero sum, consecutive lanes on consecutive words
    auto flush = [&]() {
#pragma unroll
        for (int s = 0; s < SLOTS; s++) {
            const int e = R.e0 + s * kBlock + tid;
            if (e < R.e1 && sum[s] != 0) atomicAdd(&out[(size_t) j_cur * ne + e], sum[s]);
            sum[s] = 0;
        }
    };

    unsigned long long on_disc = 0, used = 0, bad_angle = 0, outside = 0;
    const long long tiles = (n + kBlock - 1) / kBlock, per_group = (tiles + gridDim.x - 1) / gridDim.x;
    const long long tile0 = kChunkTiles ? blockIdx.x * per_group : blockIdx.x, tile1 = kChunkTiles ? min(tiles, tile0 + per_group) : tiles;
    const long long step = kChunkTiles ? 1 : gridDim.x;
    for (long long tile = tile0; tile < tile1; tile += step) {
        // ---- phase A: one record per lane
        const long long i = tile * kBlock + tid;
        bool live = false;
        double a = 0, b = 0, c = 0;
        int zone = 0, j = 0;
        if (i < n) {
            DiscRay d;
            double ft = 0;
            if (disc_ray<FUSED, PLUNGE, SURFACE>(&rays[i], m.r_isco, m.r_disc, spin, V, reverse, projradius, motion, lo, hi, law, &d, on_disc, bad_angle, fl, sf)) {
                if constexpr (ILLUM) live = response_item_illum(D, R, R.tab, d.r, d.phi, d.g, rays[i].t, d.limb, &a, &b, &c, &zone, &ft);
                else live = response_item(D, R, d.r, d.g, rays[i].t, d.limb, &a, &b, &c, &zone, &ft);
            }
            if (live) {
                used++;
                if (ft >= 0 && ft < R.nt) {              // (a NaN fails)
                    j = (int) ft;
                } else {
                    outside++;
                    live = false;
                }
            }
        }
        int at, items;
        tile_compact(live, wave_count, &at, &items);
        if (kSortTile) {
            // the place of an item among the tile's, by row and then by its compacted place: a stable rank over at most kBlock keys
            if (live) it_key[at] = j;
            __syncthreads();
            if (live) {
                int rank = 0;
                for (int k = 0; k < items; k++) {
                    const int key = it_key[k];
                    rank += (key < j || (key == j && k < at)) ? 1 : 0;
                }
                at = rank;
            }
        }
        if (live) { it_a[at] = a; it_b[at] = b; it_c[at] = c; it_z[at] = zone; it_j[at] = j; }
        __syncthreads();
        // ---- phase B: one energy per lane and slot, over the tile's live items; the row changes for the whole workgroup at once
        for (int k = 0; k < items; k++) {
            const int row = it_j[k];
            if (row != j_cur) {
                flush();
                j_cur = row;
            }
            const double g = it_a[k], q = it_b[k], w = it_c[k];
            const double* Sz = S + (size_t) it_z[k] * m.s_ne;
#pragma unroll
            for (int s = 0; s < SLOTS; s++) {
                if (s >= my_slots) break;
                const double Ep = g * E[s];
                if (Ep >= m.s_e_min && Ep <= D.s_e_last) {           // the table sample of spectrum_kernel (kr_spectrum.hip), written out
                    const double p = fmin(fmax(q + U[s], 0.0), (double) (m.s_ne - 1));
                    const int kn = min((int) p, m.s_ne - 2);
                    const double v0 = Sz[kn], v1 = Sz[kn + 1];
                    sum[s] += w * (v0 + (p - kn) * (v1 - v0));
                }
            }
        }
        // (no barrier here: tile_compact; with kSortTile it_key is written only after the next tile's first barrier, like the items)
    }

    // ---- the last row, and the tallies
    flush();
    on_disc = wave_sum(on_disc); used = wave_sum(used); bad_angle = wave_sum(bad_angle); outside = wave_sum(outside);
    if (lane == 0 && R.e0 == 0) {
        double* tally = out + (size_t) R.nt * ne;
        if (on_disc) atomicAdd(&tally[0], (double) on_disc);
        if (used) atomicAdd(&tally[1], (double) used);
        if (bad_angle) atomicAdd(&tally[2], (double) bad_angle);
        if (outside) atomicAdd(&tally[3], (double) outside);
    }
}

template <bool FUSED, bool SURFACE = false, bool ILLUM = false, typename Rays>
int response_launch(const kr_response_model* r, const kr_limb_law& law, Rays* d, int64_t n, double spin, double V, int reverse, int projradius, int motion, double lo,
                    double hi, void* d_out, hipStream_t st, DiscSurface<SURFACE> sf = DiscSurface<SURFACE>{}, const kr_illum_table* table = nullptr)
{
    if (n <= 0) return KR_OK;
    const kr_spectrum_model* m = &r->spec;
    TablePins pins;
    SpecDev D;
    int rc = spectrum_dev(m, pins, &D);
    if (rc != KR_OK) return rc;
    RespArg<ILLUM> R;
    R.t0 = r->t0; R.dt = r->dt; R.nt = r->nt; R.t_time = nullptr;
    if (r->table_time) {
        if (m->table_logbin) D.log_tdr = std::log(m->table_dr);         // (spectrum_dev takes it only with table_emis)
        rc = table_on_device(pins, kResponseTimeTable, r->table_time, (size_t) m->table_nr, &R.t_time);
        if (rc != KR_OK) return rc;
    }
    if constexpr (ILLUM) {
        rc = illum_table_dev(table, pins, &R.tab);
        if (rc != KR_OK) return rc;
    }
    const int grid = grid_for(n, kBlock, kCapHist);
    const bool in_lds = spectrum_table_in_lds(m);
    // one launch per kLaunchSlots kBlock energies: ne <= 2048 is one launch, a larger ne two over the same records (the fused form then writes rays[]
    // twice with the same values; only the first launch adds the tallies)
    for (R.e0 = 0; R.e0 < m->ne; R.e0 += kLaunchSlots * kBlock) {
        R.e1 = std::min(m->ne, R.e0 + kLaunchSlots * kBlock);
        auto with_flow = [&](auto flow) {
            constexpr bool P = decltype(flow)::plunge;
            for_slots((R.e1 - R.e0 + kBlock - 1) / kBlock, [&](auto K) {
                if constexpr (K.value <= kLaunchSlots) {
                    auto launch = [&](auto kernel, size_t lds) {
                        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, d, (long long) n, spin, V, reverse, projradius, motion, lo, hi, D, R, law, (double*) d_out,
                                           flow.arg, sf);
                    };
                    if (in_lds) launch(response_kernel<1, FUSED, K.value, P, SURFACE, ILLUM>, (size_t) m->nz * m->s_ne * sizeof(double));
                    else launch(response_kernel<2, FUSED, K.value, P, SURFACE, ILLUM>, 0);
                }
            });
        };
        if constexpr (FUSED && !SURFACE && !ILLUM) for_flow(spin, V, reverse, with_flow);
        else with_flow(FlowChoice<false>{});
        KR_LAUNCH_CHECK();
    }
    return KR_OK;
}

}  // namespace

int response_validate(const kr_response_model* r, const char* who)
{
    auto bad = [&](const char* why) { return invalid_arg(who, why); };
    if (!r) return bad("null model");
    const int rc = spectrum_validate(&r->spec, who);
    if (rc != KR_OK) return rc;
    const kr_spectrum_model& m = r->spec;
    if (m.model != 1) return bad("the response needs the table model (spec.model == 1)");
    if (r->nt < 1) return bad("nt must be >= 1");
    if (!positive_finite(r->dt)) return bad("dt must be positive and finite");
    if (!std::isfinite(r->t0)) return bad("non-finite t0");
    if ((int64_t) r->nt * m.ne > ((int64_t) 1 << 24)) return bad("nt * ne must not exceed 2^24");
    if (r->table_time) {
        if (m.table_nr < 1) return bad("table_nr must be >= 1 with a table");
        if (!std::isfinite(m.table_r_min) || !std::isfinite(m.table_dr)) return bad("non-finite model parameter");
    }
    return KR_OK;
}

int post_response_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r, const kr_limb_law* law, void* d,
                      int64_t n, void* d_out, hipStream_t st)
{
    return response_launch<true>(r, *law, (kr_ray_f64*) d, n, spin, V, reverse, projradius, motion, lo, hi, d_out, st);
}

int reduce_response_dev(const kr_response_model* r, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return response_launch<false>(r, isotropic_limb(), (const kr_ray_f64*) d, n, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, d_out, st);
}

// the forms with an (r, phi) illumination table (kr_post_response_illum_dev_f64, kr_reduce_response_illum_dev_f64)
int post_response_illum_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r, const kr_limb_law* law,
                            const kr_illum_table* t, void* d, int64_t n, void* d_out, hipStream_t st)
{
    return response_launch<true, false, true>(r, *law, (kr_ray_f64*) d, n, spin, V, reverse, projradius, motion, lo, hi, d_out, st, DiscSurface<false>{}, t);
}

int reduce_response_illum_dev(const kr_response_model* r, const kr_illum_table* t, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return response_launch<false, false, true>(r, isotropic_limb(), (const kr_ray_f64*) d, n, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, d_out, st, DiscSurface<false>{}, t);
}

// the surface forms (kr_post_response_surface_dev_f64, kr_reduce_response_surface_dev_f64): the Keplerian observer at rho
int post_response_surface_dev(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_response_model* r, const kr_limb_law* law, void* d,
                              int64_t n, void* d_out, hipStream_t st)
{
    return response_launch<true, true>(r, *law, (kr_ray_f64*) d, n, spin, -1.0, reverse, 1, 0, lo, hi, d_out, st, surface_dev(s));
}

int reduce_response_surface_dev(const kr_response_model* r, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    DiscSurface<true> none;
    none.r_in = none.slope = none.scale = 0;             // (the reduce form reads no angle)
    return response_launch<false, true>(r, isotropic_limb(), (const kr_ray_f64*) d, n, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, d_out, st, none);
}

}  // namespace kr
