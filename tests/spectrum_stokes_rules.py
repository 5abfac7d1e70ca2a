"""TEST INFRASTRUCTURE: the Stokes spectra of the disc continuum (include/kr_trace.h, STOKES SPECTRA under kr_spectrum_model) restated in numpy over ray
records, on top of tests/spectrum_rules.py (filter, energies, radial index, zones, the table interpolation) and tests/polarisation_rules.py through
hotspot_stokes_rules.polar (frame, Walker-Penrose transport, c2, s2, bad-pol, the degree law).  Written from the header's text, not from the kernel;
nothing here runs in the product path.

Per record the rule takes mu, c2, s2 and bad-pol from polar(...) -- evaluated in float64, like the records themselves: they are the per-record inputs of
the sums -- and then evaluates the weights, X and the sums in `dtype`, in the header's order of operations: np.float64, the arithmetic of the device, or
np.longdouble, the same rule with a 64-bit mantissa.

Besides I, Q and U the rule returns P[i] = sum |cd| X_i, the polarised flux with no cancellation between rays.  Differences in Q and U are taken
relative to P[i], not to |Q[i]|: Q crosses zero, and a quotient by |Q| there means nothing (hotspot_stokes_rules.scale is the precedent)."""
import numpy as np

import angle_rules as ar
import hotspot_stokes_rules as hsr
import line_rules as lr
import polarisation_rules as pr
import spectrum_rules as sr

PLANES = ("flux", "q", "u")
polar = hsr.polar


def spectrum_stokes(m, rays, pol, limb=(0, 0.0), pol_law=(0, 0.0), dtype=np.float64):
    """The rule over records that carry their redshift.  pol: polar(...) of the same records.  limb, pol_law: (law, coeff).  Returns {"energy", "flux",
    "q", "u", "p" (ne, in dtype), "on_disc", "used", "bad_pol", "used_index", "bad_index", "delta_max" (the largest |delta| of a used record)}."""
    on = sr.disc_filter(m, rays)
    bad = on & pol["bad"]
    keep = on & ~pol["bad"]
    r, g, mu = rays["r"], rays["redshift"], pol["mu"]
    kt_table, emis_table, S = sr.table(m.table_kt, m.table_nr), sr.table(m.table_emis, m.table_nr), sr.table(m.s, m.nz * m.s_ne)
    emis = None
    with np.errstate(all="ignore"):
        if m.model == 0:
            inside, ir = sr.table_index(m, r, dtype)
            kT = np.where(inside, kt_table[ir], np.nan)
            keep &= inside & np.isfinite(kT) & (kT > 0)
        elif emis_table is not None:
            inside, ir = sr.table_index(m, r, dtype)
            emis = np.where(inside, emis_table[ir], np.nan)
            keep &= inside & np.isfinite(emis)
        else:
            emis = lr.powerlaw3(r, m.q1, m.rb1, m.q2, m.rb2, m.q3)
    idx = np.flatnonzero(keep)
    E = sr.energies(m, dtype)
    out = {k: np.zeros(m.ne, dtype=dtype) for k in PLANES + ("p",)}
    delta_max = 0.0
    f = dtype(m.f_col)
    fcol_m4 = 1 / (((f * f) * f) * f)
    for at in range(0, len(idx), sr.CHUNK):
        j = idx[at:at + sr.CHUNK]
        gj = g[j].astype(dtype)
        with np.errstate(all="ignore"):
            w = ar.limb_weight(limb[0], limb[1], mu[j]).astype(dtype)
            delta = pr.degree(pol_law[0], pol_law[1], mu[j]).astype(dtype)
            g3 = 1 / ((gj * gj) * gj)
            if m.model == 0:
                c = (w * g3) * fcol_m4
                q = (1 / (f * kT[j].astype(dtype)))[:, None]
                Ep = gj[:, None] * E[None, :]
                X = ((Ep * Ep) * Ep) / np.expm1(Ep * q)
            else:
                c = (np.asarray(emis[j]).astype(dtype) * w) * g3
                X = sr.table_value(m, S, sr.zone_of(m, r[j], dtype), gj, E, dtype)
            cd = c * delta
            cq, cu = cd * pol["c2"][j].astype(dtype), cd * pol["s2"][j].astype(dtype)
            delta_max = max(delta_max, float(np.abs(delta).max()))
            out["flux"] += (c[:, None] * X).sum(axis=0)
            out["q"] += (cq[:, None] * X).sum(axis=0)
            out["u"] += (cu[:, None] * X).sum(axis=0)
            out["p"] += (np.abs(cd)[:, None] * X).sum(axis=0)
    out.update(energy=E, on_disc=int(on.sum()), used=int(len(idx)), bad_pol=int(bad.sum()), used_index=idx, bad_index=np.flatnonzero(bad), delta_max=delta_max)
    return out


def scale(want, k):
    """What a difference in plane k is divided by, per energy: P for q and u, |I| for the flux."""
    return np.abs(np.asarray(want["p"] if k in ("q", "u") else want["flux"], dtype=np.longdouble))


def diff(got, want, k):
    """max_i |got[k][i] - want[k][i]| / scale(want, k)[i] (an energy where both are equal counts 0; inf where they differ and the scale is 0)."""
    a, b = np.asarray(got[k], dtype=np.longdouble), np.asarray(want[k], dtype=np.longdouble)
    if a.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        rel = np.where(a == b, 0, np.abs(a - b) / scale(want, k))
    rel = np.where(np.isnan(rel), np.inf, rel)
    return float(rel.max())


def noise(m, rays, pol, **kw):
    """({plane: noise}, float64 result, longdouble result): the rule's own float64 - longdouble difference on the same records."""
    lo, hi = spectrum_stokes(m, rays, pol, dtype=np.float64, **kw), spectrum_stokes(m, rays, pol, dtype=np.longdouble, **kw)
    assert (lo["on_disc"], lo["used"], lo["bad_pol"]) == (hi["on_disc"], hi["used"], hi["bad_pol"])
    return {k: diff(lo, hi, k) for k in PLANES}, lo, hi


def from_words(m, words):
    """The 3 ne + 4 doubles of the Stokes entry points as the dict of spectrum_stokes (no "p")."""
    words, ne = np.asarray(words, dtype=np.float64), m.ne
    assert len(words) == 3 * ne + 4
    out = {k: words[q * ne:(q + 1) * ne] for q, k in enumerate(PLANES)}
    out.update(on_disc=int(round(words[-4])), used=int(round(words[-3])), bad_pol=int(round(words[-2])))
    return out


def degree_angle(res):
    """(degree, angle in radians) per energy: sqrt(Q^2 + U^2) / I and atan2(U, Q) / 2."""
    I, Q, U = (np.asarray(res[k], dtype=np.float64) for k in PLANES)
    with np.errstate(all="ignore"):
        return np.hypot(Q, U) / I, 0.5 * np.arctan2(U, Q)
