// kr_hotspot.hip -- an orbiting hot spot on the disc from image-plane traces (include/kr_trace.h, kr_hotspot): the light curve, the flux-weighted
// image position and the energy-time spectrogram of a Gaussian pattern of enhanced emission that moves over the disc.  A ray near the spot's annulus adds
// to EVERY observer time, n_ring x nt evaluations of a cosine and an exponential, so the kernel has the two phases of kr_spectrum.hip, per tile of kBlock
// records:
//   phase A  one RECORD per lane: the steps of disc_ray (kr_disc_pass.hpp: redshift, range_phi, filter, mu, limb law) and the ring test; a ray that
//            survives leaves one compact item in LDS, placed as tile_compact places it.  The item carries what does not depend on the time sample:
//            head {psi, om, half}   the folded angle (phi - phi0 + Om t) / 2 pi, Om / 2 pi and the spot's half-width in turns as seen from this radius,
//                                   widened by a margin: |frac(psi - om T)| > half means s <= 0 for certain (the sparsity test)
//            body {A, B, phi, t, Om, c, cx, cy, ie}   A = r r + r_s r_s, B = 2 r r_s, the weight c = limb g^-g_index, its moments, the energy bin
//   phase B  one TIME SAMPLE per lane and slot: lane k keeps T_k and the sums flux, sx, sy in registers and walks the tile's items -- every lane reads the
//            same LDS address, a broadcast.  A pair that passes the sparsity test evaluates the rule as the header writes it (the angle from phi, t, Om
//            and T_k, not from the folded head), so the test decides only what is skipped, never a value.  With nt > kBlock a lane owns SLOTS samples;
//            the test is compiled in from kSparseMinSlots slots (at one slot it costs more than it saves).
// No atomic sits in the light-curve loop: at the end of the launch a workgroup adds each non-zero sum it owns into the global words, once.
// The spectrogram: a lane owns its time samples, so within a workgroup row k of spec is written by one lane only.  SPEC 1 keeps the workgroup's
// [nt x ne] block in LDS (plain read-modify-write by the owning lane, rows padded to an odd stride against bank conflicts) and flushes it once;
// SPEC 2, above kHotSpecLdsWords, adds to global memory for the pairs with s > 0, which are sparse.  SPEC 0: ne == 0.
//   hotspot_kernel<FUSED, SLOTS, SPEC, STOKES>   FUSED: redshift + range_phi + the spot (rays[] ends as after post_line_kernel); otherwise the records
//                                        carry their redshift and are only read.
// STOKES: the Stokes light curves Q[k], U[k] beside flux, sx, sy (include/kr_trace.h, the Stokes rule under kr_hotspot).  Phase A evaluates polar_value
// (kr_post_device.hpp) for a record that passed the filter AND the ring -- about one in thirty; its E and mu are frame_value's to the bit, so nothing else
// changes value -- and the item gains cq = c delta c2 and cu = c delta s2; a bad-pol ring record is tallied and leaves no item.  Phase B keeps two more
// register sums per slot and reads two more broadcasts per lit pair.  The spectrogram stays intensity only.  Everything of it sits behind if constexpr:
// the instances without STOKES compile to what they were (profiles/hotspot_stokes_resources.txt).
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950, the flags of _build.py): the table above kHotSpecLdsWords.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>

#include "kr_disc_pass.hpp"

namespace kr {

namespace {

// Per-workgroup LDS budget of the spectrogram block in doubles: 4096 = 32 KiB next to the 23 KiB of the items, so a block of nt (ne | 1) <= 4096 words
// stays in LDS.  Registers bound the residency first (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs by slots 1 / 2 / 4 / 8 / 16):
//   reduce, SPEC 0 / 1 / 2:  168 / 209 / 227 / 256 + 2 AGPR / 256 + 75 AGPR;   184 / 227 / 247 / 256 + 24 / 256 + 103;   185 / 229 / 252 / 256 + 32 / 256 + 119
//   fused,  SPEC 0 / 1 / 2:  226, 231, 232 at one slot; 256 at two and four, held there (kTwoWaveSlots: 8 ... 37 VGPRs of phase B spilled to scratch across
//                            phase A); 256 + 62 ... 165 AGPRs at eight and sixteen
// i.e. two waves per SIMD = two workgroups per CU up to four slots (three for the one-slot reduce form without a spectrogram) and one above, and
// 2 x (32 + 23) KiB fit the CU's 160 KiB: the block never lowers the residency the registers allow.  The cosine with its large-argument reduction is what
// makes these kernels wider than kr_spectrum.hip's.
// profiles/hotspot_ab.txt has the A/B of the block against global adds and of the register bound.
// The STOKES instances: 27 KiB of items, so 2 x (32 + 27) KiB, still within the CU's 160 KiB; their registers and bound: profiles/hotspot_stokes_resources.txt
// and kStokesTwoWaveSlots below.
constexpr int kHotSpecLdsWords = 4096;
#ifdef KR_HOTSPOT_SPEC_LDS_WORDS                 // A/B builds only (scripts/hotspot_ab.py)
constexpr int kSpecBudget = KR_HOTSPOT_SPEC_LDS_WORDS;
#else
constexpr int kSpecBudget = kHotSpecLdsWords;
#endif
// The sparsity test pays once a lane owns several samples: measured at one slot (nt = 256 over one period, where a wave's 64 samples span a quarter turn and
// four waves in ten pass it anyway) it costs up to 16 % -- the acos of the head under phase A's divergence --, at two slots it wins 1.4 x, at four 2.2 x
// (profiles/hotspot_ab.txt (iii)).
#ifdef KR_HOTSPOT_SPARSE_MIN_SLOTS               // A/B builds only (1: always; 99: never, every (item, sample) pair takes the cosine)
constexpr int kSparseMinSlots = KR_HOTSPOT_SPARSE_MIN_SLOTS;
#else
constexpr int kSparseMinSlots = 2;
#endif
#ifdef KR_HOTSPOT_TWO_WAVE_SLOTS                 // A/B builds only
constexpr int kTwoWaveSlots = KR_HOTSPOT_TWO_WAVE_SLOTS;
#else
constexpr int kTwoWaveSlots = 4;                 // from two up to this many slots the kernels are held to two waves per SIMD (256 registers a lane): the
#endif                                           // fused forms then spill 8 ... 37 registers of phase B to scratch across phase A instead of halving the
                                                 // residency (3.6 against 5.5 ms at two slots, 4.1 against 6.5 at four); one slot fits as the compiler sizes it
#ifdef KR_HOTSPOT_TWO_WAVE_MIN_SLOTS             // A/B builds only (1: the bound at one slot too)
constexpr int kTwoWaveMinSlots = KR_HOTSPOT_TWO_WAVE_MIN_SLOTS;
#else
constexpr int kTwoWaveMinSlots = 2;             // (at one slot the bound is a tie or costs 3 ... 5 %: profiles/hotspot_ab.txt (v))
#endif
// The Stokes instances carry two more sums per slot and polar_value's live range across phase A: sized freely they take 252 ... 256 VGPRs and some AGPRs
// at ONE slot already.  Their bound is set by measurement like the one above (profiles/hotspot_stokes_ab.txt): two waves per SIMD up to
// kStokesTwoWaveSlots slots -- 3.9 against 6.0 ms at two slots, 4.3 against 6.7 at four -- and at one slot too wherever that wins: the fused forms (3.5
// against 5.4 ms) and the reduce forms with a spectrogram (3.5 against 4.9); the one-slot reduce form without one fits two waves as the compiler sizes it
// and runs 3 % slower under the bound, so it is left alone.
#ifdef KR_HOTSPOT_STOKES_TWO_WAVE_SLOTS          // A/B builds only (scripts/hotspot_stokes_ab.py)
constexpr int kStokesTwoWaveSlots = KR_HOTSPOT_STOKES_TWO_WAVE_SLOTS;
#else
constexpr int kStokesTwoWaveSlots = 4;
#endif
#ifdef KR_HOTSPOT_STOKES_TWO_WAVE_MIN_SLOTS      // A/B builds only (1: the bound at one slot in every form; 2: in none)
constexpr int kStokesOneSlotBound = KR_HOTSPOT_STOKES_TWO_WAVE_MIN_SLOTS == 1 ? 1 : 0;
#else
constexpr int kStokesOneSlotBound = -1;          // by form: fused, or with a spectrogram
#endif
#ifdef KR_HOTSPOT_STOKES_POLAR_ALL               // A/B builds only: the fused Stokes form takes polar_value for EVERY record, not for ring survivors only
constexpr bool kStokesPolarAll = true;
#else
constexpr bool kStokesPolarAll = false;
#endif
constexpr double kTwoPi = 6.283185307179586;

// what the kernels need besides the records: the spot by value and what is taken once, on the host
struct HotDev {
    kr_hotspot h;
    double ring;               // cut sigma, rounded once
    double ring2_wide;         // (cut sigma)^2 (1 + 1e-9): d2 at or above this gives s <= 0 with room for the rounding of d2 and of the two exponentials
    double rs2;                // r_spot r_spot
    double m_inv;              // -1 / (2 sigma sigma)
    double floor_s;            // exp(-cut cut / 2)
    double log_de;
    double t_abs_max;          // max |T_k|
    int nes;                   // the row stride of the spectrogram block in LDS: ne | 1
};

struct HotItem {
    double psi, om, half, A, B, phi, t, Om, c, cx, cy;
    int ie;
};

// what the Stokes instances take besides: the sine of the plane's inclination, taken once on the host, and the degree law.  The other instances take
// an empty struct in its place, so their arguments and their code stay what they were.
struct StokesDev {
    double sin_incl;
    kr_pol_law pol;
};
struct NoStokes {};

constexpr int two_wave_bound(int slots, bool stokes, bool fused, int spec)
{
    if (!stokes) return slots >= kTwoWaveMinSlots && slots <= kTwoWaveSlots ? 2 : 1;
    if (slots == 1) return (kStokesOneSlotBound < 0 ? fused || spec != 0 : kStokesOneSlotBound == 1) && kStokesTwoWaveSlots >= 1 ? 2 : 1;
    return slots <= kStokesTwoWaveSlots ? 2 : 1;
}

// one ray that passed the filter (and, under a law that needs it, has its angle) -> its item; false: the ray is outside the ring
template <bool SPARSE>
KR_DEV bool hotspot_item(const HotDev& D, double r, double phi, double t, double g, double limb, double x, double y, HotItem* it)
{
    const kr_hotspot& h = D.h;
    if (!(__builtin_fabs(r - h.r_spot) < D.ring)) return false;
    const double Om = h.shear ? 1 / (h.a_orbit + r * kr_sqrt(r)) : h.omega;
    const double c = limb * kr_pow(g, -1 * h.g_index);
    it->A = r * r + D.rs2;
    it->B = 2 * r * h.r_spot;
    it->phi = phi; it->t = t; it->Om = Om;
    it->c = c; it->cx = c * x; it->cy = c * y;
    it->ie = -1;
    if (h.ne > 0) {
        const double E = h.line_energy / g;
        const double fe = energy_bin_coord(h.log_e, h.e_min, h.de, D.log_de, E);
        if (fe >= 0 && fe < h.ne) it->ie = (int) fe;          // NaN fails too
    }
    it->psi = it->om = 0;
    it->half = 1.0;
    if (!SPARSE) return true;
    // the head, in turns.  s > 0 needs d2 < ring2_wide, i.e. cos(angle) > cmin; the margin covers the rounding of the folded angle
    it->psi = (phi - h.phi0 + Om * t) / kTwoPi;
    it->om = Om / kTwoPi;
    const double cmin = (it->A - D.ring2_wide) / it->B;
    const double margin = 1e-7 + 1e-12 * (__builtin_fabs(it->psi) + __builtin_fabs(it->om) * D.t_abs_max);
    it->half = cmin > -1 ? ::acos(__builtin_fmin(cmin, 1.0)) / kTwoPi + margin : 1.0;       // (1.0: every sample passes; a NaN cmin too)
    if (!(it->half == it->half)) it->half = 1.0;
    return true;
}

template <bool FUSED, int SLOTS, int SPEC, bool STOKES>
__global__ void __launch_bounds__(kBlock, two_wave_bound(SLOTS, STOKES, FUSED, SPEC))
hotspot_kernel(typename std::conditional<FUSED, kr_ray_f64, const kr_ray_f64>::type* __restrict__ rays, long long n, double spin, double V, int reverse,
               int projradius, int motion, double lo, double hi, HotDev D, kr_limb_law law, double* __restrict__ out,
               typename std::conditional<STOKES, StokesDev, NoStokes>::type S)
{
    extern __shared__ double lds_spec[];                 // SPEC 1: the workgroup's [nt x nes] block
    __shared__ double it_psi[kBlock], it_om[kBlock], it_half[kBlock];
    __shared__ double it_A[kBlock], it_B[kBlock], it_phi[kBlock], it_t[kBlock], it_Om[kBlock], it_c[kBlock], it_cx[kBlock], it_cy[kBlock];
    __shared__ int it_ie[kBlock];
    __shared__ int wave_count[kBlock / 64];
    __shared__ double it_cq[STOKES ? kBlock : 1], it_cu[STOKES ? kBlock : 1];       // (one unused word each without STOKES: the compiler drops them)
    constexpr bool SPARSE = SLOTS >= kSparseMinSlots;
    const kr_hotspot& h = D.h;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = h.nt, ne = h.ne;
    constexpr int kCurves = STOKES ? 5 : 3;              // flux, sx, sy (, Q, U)
    double* const g_spec = out + kCurves * (size_t) nt;

    // phase B's registers: the time samples this lane owns (slot q: sample q kBlock + tid) and their sums
    double T[SLOTS], flux[SLOTS], sx[SLOTS], sy[SLOTS];
    double sq[STOKES ? SLOTS : 1], su[STOKES ? SLOTS : 1];
#pragma unroll
    for (int q = 0; q < SLOTS; q++) {
        const int k = q * kBlock + tid;
        T[q] = h.t0 + k * h.dt;
        flux[q] = sx[q] = sy[q] = 0;
        if constexpr (STOKES) sq[q] = su[q] = 0;
    }
    // slots in which this wave owns a sample at all (wave-uniform)
    const int first = wave * 64;
    const int my_slots = nt > first ? min(SLOTS, (nt - first + kBlock - 1) / kBlock) : 0;
    if (SPEC == 1) {
        const int words = nt * D.nes;
        for (int w = tid; w < words; w += kBlock) lds_spec[w] = 0;
        __syncthreads();
    }

    unsigned long long on_disc = 0, used = 0, bad_angle = 0;      // (STOKES: bad_angle holds the bad-pol tally)
    for (long long base = blockIdx.x * (long long) kBlock; base < n; base += (long long) gridDim.x * kBlock) {
        // ---- phase A: one record per lane
        const long long i = base + tid;
        bool live = false;
        HotItem it;
        double cq = 0, cu = 0;
        // disc_ray and tile_compact (kr_disc_pass.hpp), written out: through the calls the fused two- and four-slot forms, which spill across phase A,
        // and the one-slot reduce forms run 1 ... 3 % slower (profiles/disc_pass_shared_ab.txt)
        if (i < n) {
            auto* ray = &rays[i];
            double r, theta, g, phi, limb = 1;
            const int steps = ray->steps;
            bool drop = false;
            if constexpr (STOKES) {
                // the Stokes rule: filter, then the ring, then polar_value for the survivors (motion is 0: the validator refuses the rest)
                kr_ray_f64 v;
                Polar pq;
                bool have_pq = false;
                if constexpr (FUSED) {
                    v = polar_record_of(ray);
                    if constexpr (kStokesPolarAll) {
                        pq = polar_value(v, spin, V, reverse, projradius, S.sin_incl);
                        have_pq = true;
                        g = pq.redshift;
                    } else {
                        const Frame f = frame_value(v, spin, V, reverse, projradius);
                        g = frame_redshift(f, v.emit, reverse);
                    }
                    r = v.r; theta = v.theta;
                    ray->redshift = g;
                    phi = wrap_phi(ray, steps, lo, hi);
                } else {
                    r = ray->r; theta = ray->theta; g = ray->redshift; phi = ray->phi;
                }
                if (disc_filter(h.r_isco, h.r_disc, steps, r, theta, g)) {
                    on_disc++;
                    if (__builtin_fabs(r - h.r_spot) < D.ring) {
                        if constexpr (!FUSED) v = polar_record_of(ray);
                        if (!have_pq) pq = polar_value(v, spin, V, reverse, projradius, S.sin_incl);
                        if (pq.bad) {
                            bad_angle++;
                        } else {
                            limb = limb_weight(law.law, law.coeff, pq.mu);
                            live = hotspot_item<SPARSE>(D, r, phi, ray->t, g, limb, v.alpha, v.beta, &it);
                            const double cd = it.c * pol_degree(S.pol.law, S.pol.coeff, pq.mu);
                            cq = cd * pq.c2;
                            cu = cd * pq.s2;
                        }
                    }
                }
                drop = true;                             // (the item, if any, is made)
            } else if constexpr (FUSED) {
                const kr_ray_f64 v = geodesic_of(ray);
                r = v.r; theta = v.theta;
                if (motion == 0) {
                    const Frame f = frame_value(v, spin, V, reverse, projradius);
                    g = frame_redshift(f, v.emit, reverse);
                    ray->redshift = g;
                    phi = wrap_phi(ray, steps, lo, hi);
                    if (disc_filter(h.r_isco, h.r_disc, steps, r, theta, g)) {
                        on_disc++;
                        const double mu = frame_mu(f);
                        if (frame_bad_angle(f, mu)) {
                            bad_angle++;
                            drop = law.law != 0;
                        }
                        limb = limb_weight(law.law, law.coeff, mu);
                    } else {
                        drop = true;
                    }
                } else {                                 // (law 0 only: the validator refuses the rest)
                    g = redshift_value(v, spin, V, reverse, projradius, motion);
                    ray->redshift = g;
                    phi = wrap_phi(ray, steps, lo, hi);
                    if (disc_filter(h.r_isco, h.r_disc, steps, r, theta, g)) on_disc++;
                    else drop = true;
                }
            } else {
                r = ray->r; theta = ray->theta; g = ray->redshift; phi = ray->phi;
                if (disc_filter(h.r_isco, h.r_disc, steps, r, theta, g)) on_disc++;
                else drop = true;
            }
            if (!drop) live = hotspot_item<SPARSE>(D, r, phi, ray->t, g, limb, ray->alpha, ray->beta, &it);
            if (live) used++;
        }
        const unsigned long long mask = __ballot(live);
        if (lane == 0) wave_count[wave] = __popcll(mask);
        __syncthreads();
        int at = __popcll(mask & ((1ull << lane) - 1)), items = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) {
            const int cnt = wave_count[w];
            if (w < wave) at += cnt;
            items += cnt;
        }
        if (live) {                                      // at < items <= kBlock
            it_psi[at] = it.psi; it_om[at] = it.om; it_half[at] = it.half;
            it_A[at] = it.A; it_B[at] = it.B; it_phi[at] = it.phi; it_t[at] = it.t; it_Om[at] = it.Om;
            it_c[at] = it.c; it_cx[at] = it.cx; it_cy[at] = it.cy; it_ie[at] = it.ie;
            if constexpr (STOKES) { it_cq[at] = cq; it_cu[at] = cu; }
        }
        __syncthreads();
        // ---- phase B: one time sample per lane and slot, over the tile's live items
        for (int j = 0; j < items; j++) {
            const double psi = it_psi[j], om = it_om[j], half = it_half[j];
#pragma unroll
            for (int q = 0; q < SLOTS; q++) {
                bool near = q < my_slots;
                if (SPARSE && near) {
                    const double u = psi - om * T[q];
                    near = __builtin_fabs(u - __builtin_rint(u)) <= half;
                }
                if (near) {
                    const double ang = it_phi[j] - (h.phi0 + it_Om[j] * (T[q] - it_t[j]));
                    const double d2 = it_A[j] - it_B[j] * ::cos(ang);
                    const double s = d2 < D.ring2_wide ? ::exp(d2 * D.m_inv) - D.floor_s : 0.0;
                    if (s > 0) {
                        const double cs = it_c[j] * s;
                        flux[q] += cs;
                        sx[q] += it_cx[j] * s;
                        sy[q] += it_cy[j] * s;
                        if constexpr (STOKES) {
                            sq[q] += it_cq[j] * s;
                            su[q] += it_cu[j] * s;
                        }
                        if (SPEC != 0) {
                            const int ie = it_ie[j], k = q * kBlock + tid;
                            if (ie >= 0 && k < nt) {
                                if (SPEC == 1) lds_spec[k * D.nes + ie] += cs;          // this lane owns row k
                                else atomicAdd(&g_spec[(size_t) k * ne + ie], cs);
                            }
                        }
                    }
                }
            }
        }
        // (no barrier here: tile_compact has the argument)
    }

    // ---- the flush: one global atomic per non-zero sum, the spectrogram block, and the tallies
#pragma unroll
    for (int q = 0; q < SLOTS; q++) {
        const int k = q * kBlock + tid;
        if (k < nt) {
            if (flux[q] != 0) atomicAdd(&out[k], flux[q]);
            if (sx[q] != 0) atomicAdd(&out[nt + k], sx[q]);
            if (sy[q] != 0) atomicAdd(&out[2 * nt + k], sy[q]);
            if constexpr (STOKES) {
                if (sq[q] != 0) atomicAdd(&out[3 * nt + k], sq[q]);
                if (su[q] != 0) atomicAdd(&out[4 * nt + k], su[q]);
            }
        }
    }
    if (SPEC == 1) {
        __syncthreads();
        const int cells = nt * ne;
        for (int w = tid; w < cells; w += kBlock) {
            const double v = lds_spec[(w / ne) * D.nes + w % ne];
            if (v != 0) atomicAdd(&g_spec[w], v);
        }
    }
    double* const tallies = out + (size_t) nt * (kCurves + ne);
    on_disc = wave_sum(on_disc); used = wave_sum(used); bad_angle = wave_sum(bad_angle);
    if (lane == 0) {
        if (on_disc) atomicAdd(&tallies[0], (double) on_disc);
        if (used) atomicAdd(&tallies[1], (double) used);
        if (bad_angle) atomicAdd(&tallies[2], (double) bad_angle);
    }
}

HotDev hotspot_dev(const kr_hotspot* h)
{
    HotDev D;
    std::memset(&D, 0, sizeof D);
    D.h = *h;
    D.ring = h->cut * h->sigma;
    D.ring2_wide = D.ring * D.ring * (1 + 1e-9);
    D.rs2 = h->r_spot * h->r_spot;
    D.m_inv = -1 / (2 * h->sigma * h->sigma);
    D.floor_s = std::exp(-1 * h->cut * h->cut / 2);
    D.log_de = h->ne > 0 && h->log_e ? std::log(h->de) : 0;
    D.t_abs_max = std::fmax(std::fabs(h->t0), std::fabs(h->t0 + (h->nt - 1) * h->dt));
    D.nes = h->ne | 1;
    return D;
}

template <bool FUSED, bool STOKES, typename Rays, typename Extra>
int hotspot_launch(const kr_hotspot* h, const kr_limb_law& law, Rays* d, int64_t n, double spin, double V, int reverse, int projradius, int motion, double lo, double hi,
                   void* d_out, hipStream_t st, Extra extra)
{
    if (n <= 0) return KR_OK;
    const HotDev D = hotspot_dev(h);
    const int slots = (h->nt + kBlock - 1) / kBlock, grid = grid_for(n, kBlock, kCapHist);
    const int64_t block_words = (int64_t) h->nt * D.nes;
    const int spec = h->ne == 0 ? 0 : block_words <= kSpecBudget ? 1 : 2;
    const size_t lds = spec == 1 ? (size_t) block_words * sizeof(double) : 0;
    for_slots(slots, [&](auto K) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, d, (long long) n, spin, V, reverse, projradius, motion, lo, hi, D, law, (double*) d_out, extra);
        };
        if (spec == 0) launch(hotspot_kernel<FUSED, K.value, 0, STOKES>);
        else if (spec == 1) launch(hotspot_kernel<FUSED, K.value, 1, STOKES>);
        else launch(hotspot_kernel<FUSED, K.value, 2, STOKES>);
    });
    KR_LAUNCH_CHECK();
    return KR_OK;
}

StokesDev stokes_dev(double inc_deg, const kr_pol_law* pol)
{
    StokesDev S;
    S.sin_incl = sin_inclination(inc_deg);
    S.pol = *pol;
    return S;
}

}  // namespace

int hotspot_validate(const kr_hotspot* h, const char* who)
{
    auto bad = [&](const char* why) { return invalid_arg(who, why); };
    if (!h) return bad("null spot");
    const double params[] = {h->r_spot, h->sigma, h->cut, h->phi0, h->omega, h->a_orbit, h->t0, h->dt, h->g_index, h->line_energy, h->e_min, h->de, h->r_isco, h->r_disc};
    for (double v : params)
        if (!std::isfinite(v)) return bad("non-finite spot parameter");
    if (h->nt < 1 || h->nt > kMaxSlots * kBlock) return bad("nt must be in 1 ... 4096");
    if (h->ne < 0 || h->ne > 4096) return bad("ne must be in 0 ... 4096");
    if ((int64_t) h->nt * h->ne > ((int64_t) 1 << 20)) return bad("nt * ne must not exceed 2^20");
    if (!(h->sigma > 0)) return bad("sigma must be positive");
    if (!(h->cut > 0)) return bad("cut must be positive");
    if (!(h->r_spot > 0)) return bad("r_spot must be positive");
    if (h->ne > 0) {
        if (const int rc = energy_axis_validate(bad, h->de, h->log_e, h->e_min)) return rc;
        if (!(h->line_energy > 0)) return bad("line_energy must be positive");
    }
    if (h->shear != 0 && h->shear != 1) return bad("shear must be 0 or 1");
    if (h->shear == 1 && !(h->a_orbit + h->r_isco * std::sqrt(h->r_isco) > 0)) return bad("shear: a_orbit + r_isco sqrt(r_isco) must be positive");
    return KR_OK;
}

int post_hotspot_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_hotspot* h, const kr_limb_law* law, void* d, int64_t n,
                     void* d_out, hipStream_t st)
{
    return hotspot_launch<true, false>(h, *law, (kr_ray_f64*) d, n, spin, V, reverse, projradius, motion, lo, hi, d_out, st, NoStokes{});
}

int reduce_hotspot_dev(const kr_hotspot* h, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return hotspot_launch<false, false>(h, isotropic_limb(), (const kr_ray_f64*) d, n, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, d_out, st, NoStokes{});
}

// the Stokes forms (kr_post_hotspot_stokes_dev_f64, kr_reduce_hotspot_stokes_dev_f64): motion is 0, the validators refuse the rest
int post_hotspot_stokes_dev(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_hotspot* h, const kr_limb_law* law,
                            const kr_pol_law* pol, void* d, int64_t n, void* d_out, hipStream_t st)
{
    return hotspot_launch<true, true>(h, *law, (kr_ray_f64*) d, n, spin, V, reverse, projradius, 0, lo, hi, d_out, st, stokes_dev(inc_deg, pol));
}

int reduce_hotspot_stokes_dev(double spin, double V, int reverse, int projradius, double inc_deg, const kr_hotspot* h, const kr_limb_law* law, const kr_pol_law* pol,
                              const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return hotspot_launch<false, true>(h, *law, (const kr_ray_f64*) d, n, spin, V, reverse, projradius, 0, 0.0, 0.0, d_out, st, stokes_dev(inc_deg, pol));
}

}  // namespace kr
