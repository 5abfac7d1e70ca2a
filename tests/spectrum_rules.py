"""TEST INFRASTRUCTURE: the continuum-spectrum rule of include/kr_trace.h (kr_spectrum_model) restated in numpy over ray records, in the manner of
tests/line_rules.py and tests/angle_rules.py.  Written from the header's text, not from the kernel; nothing here runs in the product path.

Every function takes a `dtype`: np.float64 evaluates the rule in the arithmetic of the device, np.longdouble evaluates the same rule with a 64-bit
mantissa.  The largest relative difference between the two (noise()) is the rounding noise of the rule itself on the given records: the yardstick
the device is held to."""
import numpy as np

import line_rules as lr

CHUNK = 256          # records per block of the (records x energies) evaluation


def table(ptr, count):
    return np.ctypeslib.as_array(ptr, shape=(count,)).copy() if ptr else None


def energies(m, dtype=np.float64):
    """E_i: the centre of bin i -- the geometric centre with log_e."""
    i = np.arange(m.ne).astype(dtype) + dtype(0.5)
    return dtype(m.e_min) * dtype(m.de) ** i if m.log_e else dtype(m.e_min) + i * dtype(m.de)


def disc_filter(m, rays):
    """steps > 0, r cos(theta) < 1e-2, r_isco <= r < r_disc, g > 0: the line's filter."""
    return lr.disc_filter(m, rays)


def table_index(m, r, dtype=np.float64):
    """(inside, ir): the truncated radial-table index of kr_line_bins; ir is 0 where r falls outside the table."""
    r = np.asarray(r).astype(dtype)
    with np.errstate(all="ignore"):
        fi = np.log(r / dtype(m.table_r_min)) / np.log(dtype(m.table_dr)) if m.table_logbin else (r - dtype(m.table_r_min)) / dtype(m.table_dr)
        inside = (fi > -1) & (fi < m.table_nr)
    return inside, np.where(inside, np.trunc(np.where(inside, fi, 0)), 0).astype(np.int64)


def zone_of(m, r, dtype=np.float64):
    """z = (int) (nz log(r / r_isco) / log(r_disc / r_isco)), clamped to [0, nz - 1]."""
    r = np.asarray(r).astype(dtype)
    with np.errstate(all="ignore"):
        fz = m.nz * np.log(r / dtype(m.r_isco)) / np.log(dtype(m.r_disc) / dtype(m.r_isco))
    fz = np.where(np.isnan(fz), 0, fz)
    return np.trunc(np.clip(fz, 0, m.nz - 1)).astype(np.int64)


def last_node(m):
    """s_e_last = s_e_min pow(s_de, s_ne - 1), in double, taken once."""
    return np.float64(m.s_e_min) * np.float64(m.s_de) ** np.float64(m.s_ne - 1)


def planck(E, kT, f_col, dtype=np.float64):
    """I_rest of the thermal model: f_col^-4 E^3 / expm1(E / (f_col kT))."""
    E, kT, f_col = np.asarray(E).astype(dtype), np.asarray(kT).astype(dtype), dtype(f_col)
    with np.errstate(all="ignore"):
        return f_col ** -4 * E ** 3 / np.expm1(E / (f_col * kT))


def table_value(m, S, z, g, E, dtype=np.float64):
    """S_z(g E) for records (z, g) x energies E: linear in log E' between neighbouring nodes, exactly 0 outside [s_e_min, s_e_last]."""
    g, E = np.asarray(g).astype(dtype)[:, None], np.asarray(E).astype(dtype)[None, :]
    log_sde = np.log(dtype(m.s_de))
    with np.errstate(all="ignore"):
        Ep = g * E
        inside = (Ep >= dtype(m.s_e_min)) & (Ep <= dtype(last_node(m)))
        u_g = np.log(g) / log_sde
        u_i = (np.log(E) - np.log(dtype(m.s_e_min))) / log_sde
        p = u_g + u_i
    p = np.clip(np.where(np.isnan(p), 0, p), 0, m.s_ne - 1)
    k = np.minimum(np.trunc(p).astype(np.int64), m.s_ne - 2)
    Sz = np.asarray(S).astype(dtype).reshape(m.nz, m.s_ne)[np.asarray(z)]            # (records, s_ne)
    v0, v1 = np.take_along_axis(Sz, k, axis=1), np.take_along_axis(Sz, k + 1, axis=1)
    return np.where(inside, v0 + (p - k.astype(dtype)) * (v1 - v0), dtype(0))


def limb_weight(law, coeff, mu, dtype=np.float64):
    mu = np.asarray(mu).astype(dtype)
    with np.errstate(all="ignore"):
        if law == 1:
            return 1 + dtype(coeff) * mu
        if law == 2:
            return np.log(1 + 1 / mu)
    return np.ones_like(mu)


def spectrum(m, rays, law=0, coeff=0.0, mu=None, bad=None, dtype=np.float64):
    """The rule over records that carry their redshift.  mu, bad: the emission angle and the bad-angle flag per record (tests/angle_rules.py) for the
    fused pass; None for the isotropic reduce form (law 0, bad_angle = 0).  Returns {"energy", "flux" (ne, in dtype), "on_disc", "used", "bad_angle",
    "used_index"}."""
    n = len(rays)
    on = disc_filter(m, rays)
    bad = np.zeros(n, dtype=bool) if bad is None else np.asarray(bad) & on
    keep = on & ~bad if law != 0 else on.copy()
    r, g = rays["r"], rays["redshift"]
    w = limb_weight(law, coeff, mu, dtype) if mu is not None else np.ones(n, dtype=dtype)
    kt_table, emis_table, S = table(m.table_kt, m.table_nr), table(m.table_emis, m.table_nr), table(m.s, m.nz * m.s_ne)
    with np.errstate(all="ignore"):
        if m.model == 0:
            inside, ir = table_index(m, r, dtype)
            kT = np.where(inside, kt_table[ir], np.nan)
            keep &= inside & np.isfinite(kT) & (kT > 0)
        else:
            if emis_table is not None:
                inside, ir = table_index(m, r, dtype)
                emis = np.where(inside, emis_table[ir], np.nan)
                keep &= inside & np.isfinite(emis)
            else:
                emis = lr.powerlaw3(r, m.q1, m.rb1, m.q2, m.rb2, m.q3)
            w = w * np.asarray(emis).astype(dtype)
    idx = np.flatnonzero(keep)
    E = energies(m, dtype)
    flux = np.zeros(m.ne, dtype=dtype)
    for at in range(0, len(idx), CHUNK):
        j = idx[at:at + CHUNK]
        gj = g[j].astype(dtype)
        with np.errstate(all="ignore"):
            c = (w[j] * (1 / (gj * gj * gj)))[:, None]
            if m.model == 0:
                val = planck(gj[:, None] * E[None, :], kT[j][:, None], m.f_col, dtype)
            else:
                val = table_value(m, S, zone_of(m, r[j], dtype), gj, E, dtype)
            flux += (c * val).sum(axis=0)
    return {"energy": E, "flux": flux, "on_disc": int(on.sum()), "used": int(len(idx)), "bad_angle": int(bad.sum()), "used_index": idx}


def rel_diff(got, want):
    """The largest |got - want| / |want| over the energies (0 where both are 0; inf where only one is)."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    with np.errstate(all="ignore"):
        rel = np.where(got == want, 0, np.abs(got - want) / np.abs(want))
    return float(np.max(rel)) if rel.size else 0.0


def noise(m, rays, **kw):
    """(noise, float64 result, longdouble result): the largest relative difference between the float64 and the longdouble evaluation of the rule."""
    lo, hi = spectrum(m, rays, dtype=np.float64, **kw), spectrum(m, rays, dtype=np.longdouble, **kw)
    assert (lo["on_disc"], lo["used"], lo["bad_angle"]) == (hi["on_disc"], hi["used"], hi["bad_angle"])
    return rel_diff(lo["flux"], hi["flux"]), lo, hi


def synthetic_records(r, g, theta=np.pi / 2, steps=1):
    """Records that carry only what the reduce form reads: steps, r, theta, redshift."""
    from raytrace_cpu_amd import capi
    r = np.atleast_1d(np.asarray(r, dtype=np.float64))
    rays = np.zeros(len(r), dtype=capi.RAY_F64)
    rays["r"], rays["theta"], rays["redshift"], rays["steps"] = r, theta, g, steps
    return rays
