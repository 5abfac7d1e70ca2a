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

// PLUNGE: the disc flow of KR_V_PLUNGE (DiscFlow, kr_post_device.hpp), fused form only; the host picks the instance from V
template <int MODEL, bool FUSED, int SLOTS, bool PLUNGE>
__global__ void __launch_bounds__(kBlock)
spectrum_kernel(typename std::conditional<FUSED, kr_ray_f64, const kr_ray_f64>::type* __restrict__ rays, long long n, double spin, double V, int reverse,
                int projradius, int motion, double lo, double hi, SpecDev D, kr_limb_law law, double* __restrict__ out, DiscFlow<PLUNGE> fl)
{
    constexpr bool THERMAL = MODEL == 0;
    extern __shared__ double lds_s[];                    // MODEL 1: the table
    __shared__ double it_a[kBlock], it_b[kBlock], it_c[kBlock];
    __shared__ int it_z[kBlock];
    __shared__ int wave_count[kBlock / 64];
    const kr_spectrum_model& m = D.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ne = m.ne;

    // phase B's registers: the energies this lane owns (slot s: energy s kBlock + tid), their per-energy term and their sums
    double E[SLOTS], U[SLOTS], sum[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int e = s * kBlock + tid;
        E[s] = e < ne ? (m.log_e ? m.e_min * kr_pow(m.de, e + 0.5) : m.e_min + (e + 0.5) * m.de) : 0;      // (0: an energy beyond ne adds nothing, and is never flushed)
        U[s] = (!THERMAL && e < ne) ? (kr_log(E[s]) - D.log_semin) / D.log_sde : 0;
        sum[s] = 0;
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

    unsigned long long on_disc = 0, used = 0, bad_angle = 0;
    for (long long base = blockIdx.x * (long long) kBlock; base < n; base += (long long) gridDim.x * kBlock) {
        // ---- phase A: one record per lane
        const long long i = base + tid;
        bool live = false;
        double a = 0, b = 0, c = 0;
        int zone = 0;
        if (i < n) {
            DiscRay d;
            if (disc_ray<FUSED, PLUNGE>(&rays[i], m.r_isco, m.r_disc, spin, V, reverse, projradius, motion, lo, hi, law, &d, on_disc, bad_angle, fl))
                live = spectrum_item<THERMAL>(D, d.r, d.g, d.limb, &a, &b, &c, &zone);
            if (live) used++;
        }
        int at, items;
        tile_compact(live, wave_count, &at, &items);
        if (live) { it_a[at] = a; it_b[at] = b; it_c[at] = c; it_z[at] = zone; }
        __syncthreads();
        // ---- phase B: one energy per lane and slot, over the tile's live items
        for (int j = 0; j < items; j++) {
            const double g = it_a[j], q = it_b[j], w = it_c[j];
            const double* Sz = THERMAL ? nullptr : S + (size_t) it_z[j] * m.s_ne;
#pragma unroll
            for (int s = 0; s < SLOTS; s++) {
                if (s >= my_slots) break;
                const double Ep = g * E[s];
                if (THERMAL) {
                    sum[s] += w * (Ep * Ep * Ep) / expm1(Ep * q);
                } else if (Ep >= m.s_e_min && Ep <= D.s_e_last) {
                    const double p = fmin(fmax(q + U[s], 0.0), (double) (m.s_ne - 1));
                    const int k = min((int) p, m.s_ne - 2);
                    const double v0 = Sz[k], v1 = Sz[k + 1];
                    sum[s] += w * (v0 + (p - k) * (v1 - v0));
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
    }
    on_disc = wave_sum(on_disc); used = wave_sum(used); bad_angle = wave_sum(bad_angle);
    if (lane == 0) {
        if (on_disc) atomicAdd(&out[ne], (double) on_disc);
        if (used) atomicAdd(&out[ne + 1], (double) used);
        if (bad_angle) atomicAdd(&out[ne + 2], (double) bad_angle);
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

template <bool FUSED, typename Rays>
int spectrum_launch(const kr_spectrum_model* m, const kr_limb_law& law, Rays* d, int64_t n, double spin, double V, int reverse, int projradius, int motion, double lo,
                    double hi, void* d_out, hipStream_t st)
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
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, d, (long long) n, spin, V, reverse, projradius, motion, lo, hi, D, law, (double*) d_out, flow.arg);
            };
            if (m->model == 0) launch(spectrum_kernel<0, FUSED, K.value, P>, 0);
            else if (s_words <= kSpecLdsWords) launch(spectrum_kernel<1, FUSED, K.value, P>, (size_t) s_words * sizeof(double));
            else launch(spectrum_kernel<2, FUSED, K.value, P>, 0);
        });
    };
    if constexpr (FUSED) for_flow(spin, V, reverse, with_flow);
    else with_flow(FlowChoice<false>{});
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
    return spectrum_launch<true>(m, *law, (kr_ray_f64*) d, n, spin, V, reverse, projradius, motion, lo, hi, d_out, st);
}

int reduce_spectrum_dev(const kr_spectrum_model* m, const void* d, int64_t n, void* d_out, hipStream_t st)
{
    return spectrum_launch<false>(m, isotropic_limb(), (const kr_ray_f64*) d, n, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, d_out, st);
}

}  // namespace kr
