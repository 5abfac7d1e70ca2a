// kr_spectrum.hip -- continuum spectra of the disc from image-plane traces (include/kr_trace.h, kr_spectrum_model): a multicolour blackbody or a
// tabulated rest-frame spectrum, smeared by the rays.  Unlike the line (kr_line.hip), where a ray lands in ONE energy bin and an LDS histogram with one
// atomic per ray does the job, every disc ray adds to EVERY output energy: n_disc x ne evaluations, each an expm1 or a table interpolation.  So the
// kernel turns the work round between two phases, per tile of kBlock records:
//   phase A  one RECORD per lane: disc_ray (kr_disc_pass.hpp: redshift, range_phi, filter, mu, limb law); a ray that survives leaves one compact item
//            {g, 1 / (f_col kT) or u_g and its zone, w g^-3} in LDS, placed by tile_compact;
//   phase B  one ENERGY per lane: lane e keeps E_e and its running sum in registers and walks the tile's items -- every lane reads the same LDS
//            address, a broadcast.  With ne > kBlock a lane owns SLOTS energies.
// No atomic sits in either inner loop: at the end of the launch a workgroup adds each non-zero sum it owns into the global spectrum, once.
//   spectrum_kernel<MODEL, FUSED, SLOTS>   MODEL 0: thermal; 1: table, S in LDS; 2: table, S in global memory.  FUSED: redshift + range_phi + spectrum
//                                          (rays[] ends as after post_line_kernel); otherwise the records carry their redshift and are only read.
// STOKES: the Stokes spectra Q(E), U(E) beside I(E) (include/kr_trace.h, STOKES SPECTRA under kr_spectrum_model).  Phase A is written out, as in
// kr_hotspot.hip (disc_ray is shared with kernels that must keep their code): polar_value (kr_post_device.hpp) in place of frame_value -- its E and mu
// are frame_value's to the bit, so the stored redshift keeps its value --, the filter, and for EVERY disc record the item gains cq = c delta c2 and cu = c delta s2; a bad-pol
// disc record is tallied and leaves no item, whatever the limb law.  Phase B forms ONE X = I_rest(g E) per (item, energy) and feeds three register sums
// with it; the flush adds up to three words per owned energy.  Everything of it sits behind if constexpr: the instances without STOKES compile to what
// they were (profiles/spectrum_stokes_resources.txt).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>

#include "kr_spectrum_dev.hpp"

namespace kr {

namespace {

// Per-workgroup LDS budget of the table S in doubles: 4096 = 32 KiB, next to the 7 KiB of the items.  Registers bound the residency first
// (-Rpass-analysis=kernel-resource-usage, gfx950: the fused kernels take 172 ... 248 VGPRs (thermal) and 201 ... 256 (table) -> 2 waves / SIMD = 2
// workgroups / CU, the sixteen-slot table kernels 1; the reduce forms 122 ... 198 and 151 ... 256 -> 4 ... 1), and 4 x 39 KiB fit the CU's 160 KiB:
// the table never lowers the occupancy of any of them.  A 64-KiB budget would cap the one- and two-slot reduce forms at 2 workgroups / CU.  Above
// the budget S is read from global memory (a table that size is L2-resident, and every lane of a wave reads near the same node).
constexpr int kSpecLdsWords = 4096;

// what the Stokes instances take besides: the sine of the plane's inclination, taken once on the host, and the degree law.  The other instances take
// an empty struct in its place, so their code stays what it was.
struct StokesDev {
    double sin_incl;
    kr_pol_law pol;
};
struct NoStokes {};

// The Stokes instances' register bound, in waves per SIMD (the second launch bound); 1 leaves the compiler free, as the instances without STOKES are.
// A Stokes slot holds E, (U,) and three sums, 8 ... 10 VGPRs against 4 ... 6, and polar_value is live across phase A beside them.  Sized freely every
// form still reaches two waves per SIMD up to four slots EXCEPT the fused table forms at four slots (256 VGPRs + 8 AGPRs: one wave); held to two waves
// those spill 8 VGPRs and run 6.4 against 10.7 ms (1024 energies, profiles/spectrum_stokes_ab.txt).  Everywhere else the bound changes no residency and
// was a tie or a loss -- the one-slot table forms ran 11 ... 13 % slower under it at the same register count -- so only those forms carry it.
#ifdef KR_SPECTRUM_STOKES_TWO_WAVE_SLOTS         // A/B builds only (scripts/spectrum_stokes_ab.py): hold EVERY Stokes kernel to two waves per SIMD up to this many slots (0: none)
constexpr int kStokesTwoWaveSlots = KR_SPECTRUM_STOKES_TWO_WAVE_SLOTS;
#else
constexpr int kStokesTwoWaveSlots = -1;          // by form: the fused table forms at four slots
#endif
// Phase A of the fused Stokes form: polar_value for EVERY record in place of frame_value (as the Stokes image and line passes do), or frame_value for
// every record and polar_value for the on-disc ones.  With a fifth of the records on the disc nearly every wave near it takes both branches of the second
// order; measured, the first is 0.6 ... 2 % faster in four cases of four, about the scatter between builds (profiles/spectrum_stokes_ab.txt).
#ifdef KR_SPECTRUM_STOKES_FRAME_FIRST            // A/B builds only
constexpr bool kStokesPolarFirst = false;
#else
constexpr bool kStokesPolarFirst = true;
#endif
constexpr int stokes_wave_bound(bool stokes, int model, bool fused, int slots)
{
    if (!stokes) return 1;
    if (kStokesTwoWaveSlots >= 0) return slots <= kStokesTwoWaveSlots ? 2 : 1;
    return fused && model != 0 && slots == 4 ? 2 : 1;
}

// PLUNGE: the disc flow of KR_V_PLUNGE (DiscFlow, kr_post_device.hpp), fused form only; the host picks the instance from V (never with STOKES)
// SURFACE: the continuum of a disc with a surface (DiscSurface, kr_post_device.hpp): the filter, the radius and the angle of disc_ray's surface flavour,
// in both forms (never with PLUNGE or STOKES)
template <int MODEL, bool FUSED, int SLOTS, bool PLUNGE, bool STOKES, bool SURFACE = false>
__global__ void __launch_bounds__(kBlock, stokes_wave_bound(STOKES, MODEL, FUSED, SLOTS))
spectrum_kernel(typename std::conditional<FUSED, kr_ray_f64, const kr_ray_f64>::type* __restrict__ rays, long long n, double spin, double V, int reverse,
                int projradius, int motion, double lo, double hi, SpecDev D, kr_limb_law law, double* __restrict__ out, DiscFlow<PLUNGE> fl,
                typename std::conditional<STOKES, StokesDev, NoStokes>::type P, DiscSurface<SURFACE> sf)
{
    static_assert(!(STOKES && PLUNGE), "polar_value has no plunging form");
    static_assert(!(SURFACE && (PLUNGE || STOKES)), "the surface passes keep the Keplerian observer at rho and carry no polarisation");
    constexpr bool THERMAL = MODEL == 0;
    extern __shared__ double lds_s[];                    // MODEL 1: the table
    __shared__ double it_a[kBlock], it_b[kBlock], it_c[kBlock];
    __shared__ int it_z[kBlock];
    __shared__ int wave_count[kBlock / 64];
    __shared__ double it_cq[STOKES ? kBlock : 1], it_cu[STOKES ? kBlock : 1];       // (one unused word each without STOKES: the compiler drops them)
    const kr_spectrum_model& m = D.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ne = m.ne;

    // phase B's registers: the energies this lane owns (slot s: energy s kBlock + tid), their per-energy term and their sums
    double E[SLOTS], U[SLOTS], sum[SLOTS];
    double sq[STOKES ? SLOTS : 1], su[STOKES ? SLOTS : 1];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int e = s * kBlock + tid;
        E[s] = e < ne ? (m.log_e ? m.e_min * kr_pow(m.de, e + 0.5) : m.e_min + (e + 0.5) * m.de) : 0;      // (0: an energy beyond ne adds nothing, and is never flushed)
        U[s] = (!THERMAL && e < ne) ? (kr_log(E[s]) - D.log_semin) / D.log_sde : 0;
        sum[s] = 0;
        if constexpr (STOKES) sq[s] = su[s] = 0;
    }
    // slots in which this wave owns an energy at all (wave-uniform)
    const int first = wave * 64;
    const int my_slots = ne > first ? min(SLOTS, (ne - first + kBlock - 1) / kBlock) : 0;
    const double* S = D.s;
    if (MODEL == 1) {
        const int words = m.nz * m.s_ne;
        for (int w = tid; w < words; w += kBlock) lds_s[w] = D.s[w];
        S = lds_s;                                       // (the first barrier of the tile loop orders these stores before phase B)
    }

    unsigned long long on_disc = 0, used = 0, bad_angle = 0;      // (STOKES: bad_angle holds the bad-pol tally)
    for (long long base = blockIdx.x * (long long) kBlock; base < n; base += (long long) gridDim.x * kBlock) {
        // ---- phase A: one record per lane
        const long long i = base + tid;
        bool live = false;
        double a = 0, b = 0, c = 0;
        int zone = 0;
        [[maybe_unused]] double cq = 0, cu = 0;
        if constexpr (STOKES) {
            // the Stokes rule: the front end of disc_ray written out (motion is 0: the validator refuses the rest), polar_value for the disc records
            if (i < n) {
                auto* ray = &rays[i];
                const int steps = ray->steps;
                kr_ray_f64 v;
                Polar pq;
                bool have_pq = false;
                double r, theta, g;
                if constexpr (FUSED) {
                    v = polar_record_of(ray);
                    if constexpr (kStokesPolarFirst) {
                        pq = polar_value(v, spin, V, reverse, projradius, P.sin_incl);
                        have_pq = true;
                        g = pq.redshift;
                    } else {
                        const Frame f = frame_value(v, spin, V, reverse, projradius);
                        g = frame_redshift(f, v.emit, reverse);
                    }
                    r = v.r; theta = v.theta;
                    ray->redshift = g;
                    wrap_phi(ray, steps, lo, hi);
                } else {
                    r = ray->r; theta = ray->theta; g = ray->redshift;
                }
                if (disc_filter(m.r_isco, m.r_disc, steps, r, theta, g)) {
                    on_disc++;
                    if constexpr (!FUSED) v = polar_record_of(ray);
                    if (!have_pq) pq = polar_value(v, spin, V, reverse, projradius, P.sin_incl);
                    if (pq.bad) {
                        bad_angle++;
                    } else {
                        live = spectrum_item<THERMAL>(D, r, g, limb_weight(law.law, law.coeff, pq.mu), &a, &b, &c, &zone);
                        const double cd = c * pol_degree(P.pol.law, P.pol.coeff, pq.mu);
                        cq = cd * pq.c2;
                        cu = cd * pq.s2;
                    }
                }
                if (live) used++;
            }
        } else if (i < n) {
            DiscRay d;
            if (disc_ray<FUSED, PLUNGE, SURFACE>(&rays[i], m.r_isco, m.r_disc, spin, V, reverse, projradius, motion, lo, hi, law, &d, on_disc, bad_angle, fl, sf))
                live = spectrum_item<THERMAL>(D, d.r, d.g, d.limb, &a, &b, &c, &zone);
            if (live) used++;
        }
        int at, items;
        tile_compact(live, wave_count, &at, &items);
        if (live) { it_a[at] = a; it_b[at] = b; it_c[at] = c; it_z[at] = zone; }
        if constexpr (STOKES) {
            if (live) { it_cq[at] = cq; it_cu[at] = cu; }
        }
        __syncthreads();
        // ---- phase B: one energy per lane and slot, over the tile's live items
        for (int j = 0; j < items; j++) {
            const double g = it_a[j], q = it_b[j], w = it_c[j];
            const double* Sz = THERMAL ? nullptr : S + (size_t) it_z[j] * m.s_ne;
            [[maybe_unused]] double wq = 0, wu = 0;
            if constexpr (STOKES) { wq = it_cq[j]; wu = it_cu[j]; }
#pragma unroll
            for (int s = 0; s < SLOTS; s++) {
                if (s >= my_slots) break;
                const double Ep = g * E[s];
                if (THERMAL) {
                    if constexpr (STOKES) {              // one X per (item, energy): X = E'^3 / expm1(E' q), then three products and three sums
                        const double X = (Ep * Ep * Ep) / expm1(Ep * q);
                        sum[s] += w * X;
                        sq[s] += wq * X;
                        su[s] += wu * X;
                    } else {
                        sum[s] += w * (Ep * Ep * Ep) / expm1(Ep * q);
                    }
                } else if (Ep >= m.s_e_min && Ep <= D.s_e_last) {
                    const double p = fmin(fmax(q + U[s], 0.0), (double) (m.s_ne - 1));
                    const int k = min((int) p, m.s_ne - 2);
                    const double v0 = Sz[k], v1 = Sz[k + 1];
                    if constexpr (STOKES) {
                        const double X = v0 + (p - k) * (v1 - v0);
                        sum[s] += w * X;
                        sq[s] += wq * X;
                        su[s] += wu * X;
                    } else {
                        sum[s] += w * (v0 + (p - k) * (v1 - v0));
                    }
                }
            }
        }
        // (no barrier here: tile_compact)
    }

    // ---- the flush: one global atomic per energy with a non-zero sum, and the tallies
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int e = s * kBlock + tid;
        if (e < ne && sum[s] != 0) atomicAdd(&out[e], sum[s]);
        if constexpr (STOKES) {
            if (e < ne && sq[s] != 0) atomicAdd(&out[ne + e], sq[s]);
            if (e < ne && su[s] != 0) atomicAdd(&out[2 * ne + e], su[s]);
        }
    }
    double* const tallies = out + (STOKES ? 3 : 1) * ne;
    on_disc = wave_sum(on_disc); used = wave_sum(used); bad_angle = wave_sum(bad_angle);
    if (lane == 0) {
        if (on_disc) atomicAdd(&tallies[0], (double) on_disc);
        if (used) atomicAdd(&tallies[1], (double) used);
        if (bad_angle) atomicAdd(&tallies[2], (double) bad_angle);
    }
}

}  // namespace

// ---- the tables on the device: one array per distinct contents in the device table store (TablePins, kr_common.hpp), each under a kind of its own --
int table_on_device(TablePins& pins, TableKind kind, const double* host, size_t count, const double** dev)
{
    const std::string key((const char*) host, count * sizeof(double));
    return pins.lookup(kind, key, [&](std::vector<double>& h) { h.assign(host, host + count); }, dev);
}

int spectrum_dev(const kr_spectrum_model* m, TablePins& pins, SpecDev* D)
{
    std::memset(D, 0, sizeof *D);
    D->m = *m;
    D->log_de = m->log_e ? std::log(m->de) : 0;
    const bool table = m->model == 0 || m->table_emis;
    D->log_tdr = table && m->table_logbin ? std::log(m->table_dr) : 0;
    if (m->model == 0) {
        D->fcol_m4 = 1 / (m->f_col * m->f_col * m->f_col * m->f_col);
        return table_on_device(pins, kSpectrumKtTable, m->table_kt, (size_t) m->table_nr, &D->t_kt);
    }
    D->log_sde = std::log(m->s_de);
    D->log_semin = std::log(m->s_e_min);
    D->log_span = std::log(m->r_disc / m->r_isco);
    D->s_e_last = m->s_e_min * std::pow(m->s_de, (double) (m->s_ne - 1));
    if (m->table_emis) {
        const int rc = table_on_device(pins, kSpectrumEmisTable, m->table_emis, (size_t) m->table_nr, &D->t_emis);
        if (rc != KR_OK) return rc;
    }
    return table_on_device(pins, kSpectrumTable, m->s, (size_t) m->nz * m->s_ne, &D->s);
}

bool spectrum_table_in_lds(const kr_spectrum_model* m)
{
    return (int64_t) m->nz * m->s_ne <= kSpecLdsWords;
}

namespace {

template <bool FUSED, bool STOKES, bool SURFACE = false, typename Rays, typename Extra>
int spectrum_launch(const kr_spectrum_model* m, const kr_limb_law& law, Rays* d, int64_t n, double spin, double V, int reverse, int projradius, int motion, double lo,
                    double hi, void* d_out, hipStream_t st, Extra extra, DiscSurface<SURFACE> sf = DiscSurface<SURFACE>{})
{
    if (n <= 0) return KR_OK;
    TablePins pins;
    SpecDev D;
    const int rc = spectrum_dev(m, pins, &D);
    if (rc != KR_OK) return rc;
    const int slots = (m->ne + kBlock - 1) / kBlock, grid = grid_for(n, kBlock, kCapHist);
    const int64_t s_words = (int64_t) m->nz * m->s_ne;
    auto with_flow = [&](auto flow) {
        constexpr bool P = decltype(flow)::plunge;
        for_slots(slots, [&](auto K) {
            auto launch = [&](auto kernel, size_t lds) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, d, (long long) n, spin, V, reverse, projradius, motion, lo, hi, D, law, (double*) d_out, flow.arg, extra, sf);
            };
            if (m->model == 0) launch(spectrum_kernel<0, FUSED, K.value, P, STOKES, SURFACE>, 0);
            else if (s_words <= kSpecLdsWords) launch(spectrum_kernel<1, FUSED, K.value, P, STOKES, SURFACE>, (size_t) s_words * sizeof(double));
            else launch(spectrum_kernel<2, FUSED, K.value, P, STOKES, SURFACE>, 0);
        });
    };
    if constexpr (FUSED && !STOKES && !SURFACE) for_flow(spin, V, reverse, with_flow);
    else with_flow(FlowChoice<false>{});               // (the Stokes forms: KR_V_PLUNGE is refused before this; the surface forms have no V)
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace

int spectrum_validate(const kr_spectrum_model* m, const char* who)
{
    auto bad = [&](const char* why) { return invalid_arg(who, why); };
    if (!m) return bad("null model");
    if (m->model != 0 && m->model != 1) return bad("model must be 0 (thermal) or 1 (table)");
    const double params[] = {m->e_min, m->de, m->r_isco, m->r_disc, m->q1, m->rb1, m->q2, m->rb2, m->q3, m->f_col, m->s_e_min, m->s_de};
    for (double v : params)
        if (!std::isfinite(v)) return bad("non-finite model parameter");
    if (m->ne < 1 || m->ne > kMaxSlots * kBlock) return bad("ne must be in 1 ... 4096");
    if (const int rc = energy_axis_validate(bad, m->de, m->log_e, m->e_min)) return rc;
    const bool table = m->model == 0 ? true : m->table_emis != nullptr;
    if (m->model == 0) {
        if (!m->table_kt) return bad("the thermal model needs table_kt");
        if (!(m->f_col > 0)) return bad("f_col must be positive");
    } else {
        if (!m->s) return bad("the table model needs s");
        if (m->s_ne < 2) return bad("s_ne must be >= 2");
        if (!(m->s_de > 1)) return bad("s_de (the ratio between nodes) must be > 1");
        if (!(m->s_e_min > 0)) return bad("s_e_min must be positive");
        if (m->nz < 1) return bad("nz must be >= 1");
        if ((int64_t) m->nz * m->s_ne > ((int64_t) 1 << 20)) return bad("nz * s_ne must not exceed 2^20");
    }
    if (table) {
        if (m->table_nr < 1) return bad("table_nr must be >= 1 with a table");
        if (!std::isfinite(m->table_r_min) || !std::isfinite(m->table_dr)) return bad("non-finite model parameter");
    }
    return KR_OK;
}

int spectrum_law_validate(const kr_limb_law* law, int motion, const char* who)
{
    const int rc = limb_validate(law, who);
    if (rc != KR_OK) return rc;
    if (motion != 0 && law->law != 0) return invalid_arg(who, "motion != 0 needs limb law 0 (only the orbiting observer has the frame of mu)");
    return KR_OK;
}

int post_spectrum_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_spectrum_model* m, const kr_limb_law* law, void* d,
                      int64_t n, void* d_out, hipStream_t st)
{
    return spectrum_launch<true, false>(m, *law, (kr_ray_f64*) d, n, spin, V, reverse, projradius, motion, lo, hi, d_out, st, NoStokes{});
}

int reduce_spectrum_dev(const kr_spectrum_model* m, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return spectrum_launch<false, false>(m, isotropic_limb(), (const kr_ray_f64*) d, n, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, d_out, st, NoStokes{});
}

// the surface forms (kr_post_spectrum_surface_dev_f64, kr_reduce_spectrum_surface_dev_f64): the Keplerian observer at rho
int post_spectrum_surface_dev(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_spectrum_model* m, const kr_limb_law* law, void* d,
                              int64_t n, void* d_out, hipStream_t st)
{
    return spectrum_launch<true, false, true>(m, *law, (kr_ray_f64*) d, n, spin, -1.0, reverse, 1, 0, lo, hi, d_out, st, NoStokes{}, surface_dev(s));
}

int reduce_spectrum_surface_dev(const kr_spectrum_model* m, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    DiscSurface<true> none;
    none.r_in = none.slope = none.scale = 0;             // (the reduce form reads no angle)
    return spectrum_launch<false, false, true>(m, isotropic_limb(), (const kr_ray_f64*) d, n, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, d_out, st, NoStokes{}, none);
}

// the Stokes forms (kr_post_spectrum_stokes_dev_f64, kr_reduce_spectrum_stokes_dev_f64): motion is 0, the validators refuse the rest
static StokesDev stokes_dev(double inc_deg, const kr_pol_law* pol)
{
    StokesDev S;
    S.sin_incl = sin_inclination(inc_deg);
    S.pol = *pol;
    return S;
}

int post_spectrum_stokes_dev(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_spectrum_model* m, const kr_limb_law* law,
                             const kr_pol_law* pol, void* d, int64_t n, void* d_out, hipStream_t st)
{
    return spectrum_launch<true, true>(m, *law, (kr_ray_f64*) d, n, spin, V, reverse, projradius, 0, lo, hi, d_out, st, stokes_dev(inc_deg, pol));
}

int reduce_spectrum_stokes_dev(double spin, double V, int reverse, int projradius, double inc_deg, const kr_spectrum_model* m, const kr_limb_law* law, const kr_pol_law* pol,
                               const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return spectrum_launch<false, true>(m, *law, (const kr_ray_f64*) d, n, spin, V, reverse, projradius, 0, 0.0, 0.0, d_out, st, stokes_dev(inc_deg, pol));
}

}  // namespace kr
