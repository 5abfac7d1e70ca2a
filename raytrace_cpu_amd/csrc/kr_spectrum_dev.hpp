// kr_spectrum_dev.hpp -- what the passes that smear a kr_spectrum_model over the disc rays share (kr_spectrum.hip, kr_response.hip): the model as the
// kernels see it, the radial-table index and the per-ray item of phase A.  The device helpers are forced-inline functions, as in kr_disc_pass.hpp; the
// host functions are defined in kr_spectrum.hip.
#pragma once

#include "kr_disc_pass.hpp"

namespace kr {

// what the kernels need besides the records: the model by value (its host pointers are never dereferenced on the device), the device copies of the
// tables and the logarithms that are taken once, on the host
struct SpecDev {
    kr_spectrum_model m;
    const double* t_kt;        // [table_nr] on the device (model 0)
    const double* t_emis;      // [table_nr] on the device, or null: powerlaw3 (model 1)
    const double* s;           // [nz][s_ne] on the device (model 1)
    double log_de, log_tdr, log_sde, log_semin, log_span, s_e_last, fcol_m4;
};

KR_DEV bool table_index(const SpecDev& D, double r, int* ir)
{
    return radial_table_index(D.m.table_logbin, D.m.table_r_min, D.m.table_dr, D.log_tdr, D.m.table_nr, r, ir);
}

// one ray that passed the filter (and, under a law that needs it, has its angle) -> its item {a, b, c, zone}; false: the ray is not used
template <bool THERMAL>
KR_DEV bool spectrum_item(const SpecDev& D, double r, double g, double limb, double* a, double* b, double* c, int* zone)
{
    const kr_spectrum_model& m = D.m;
    const double g3 = 1 / (g * g * g);
    *a = g;
    *zone = 0;
    if (THERMAL) {
        int ir;
        if (!table_index(D, r, &ir)) return false;
        const double kT = D.t_kt[ir];
        if (!(__builtin_isfinite(kT) && kT > 0)) return false;
        *b = 1 / (m.f_col * kT);
        *c = limb * g3 * D.fcol_m4;
        return true;
    }
    double emis;
    if (D.t_emis) {
        int ir;
        if (!table_index(D, r, &ir)) return false;
        emis = D.t_emis[ir];
        if (!__builtin_isfinite(emis)) return false;
    } else {
        emis = powerlaw3(r, m.q1, m.rb1, m.q2, m.rb2, m.q3);
    }
    const double fz = m.nz * kr_log(r / m.r_isco) / D.log_span;
    *zone = (int) fmin(fmax(fz, 0.0), (double) (m.nz - 1));         // (a NaN becomes zone 0)
    *b = kr_log(g) / D.log_sde;
    *c = emis * limb * g3;
    return true;
}

// ---- host side (kr_spectrum.hip) ------------------------------------------------------------------------------------------------------------
// one array per distinct contents in the device table store (TablePins, kr_common.hpp), under `kind`
int table_on_device(TablePins& pins, TableKind kind, const double* host, size_t count, const double** dev);
// the model's tables on the device and the logarithms; pinned in `pins`: keep it until the kernel that reads the tables has been enqueued
int spectrum_dev(const kr_spectrum_model* m, TablePins& pins, SpecDev* D);
// whether the table S of a model-1 spectrum goes into LDS (kSpecLdsWords) or stays in global memory
bool spectrum_table_in_lds(const kr_spectrum_model* m);

}  // namespace kr
