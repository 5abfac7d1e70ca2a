"""TEST INFRASTRUCTURE: the reverberation-response rule of include/kr_trace.h (kr_response_model) restated in numpy over ray records, on top of
tests/spectrum_rules.py.  Written from the header's text, not from the kernel; nothing here runs in the product path.

Every function takes a `dtype`: np.float64 evaluates the rule in the arithmetic of the device, np.longdouble evaluates the same rule with a 64-bit
mantissa.  The largest relative difference between the two over the non-zero cells (noise()) is the rounding noise of the rule itself on the given
records: the yardstick the device is held to."""
import numpy as np

import line_rules as lr
import spectrum_rules as sr


def time_coordinate(R, t, tt, dtype=np.float64):
    """ft = (t + tt - t0) / dt: the line pass's expression, in its order."""
    with np.errstate(all="ignore"):
        return (np.asarray(t).astype(dtype) + np.asarray(tt).astype(dtype) - dtype(R.t0)) / dtype(R.dt)


def used_records(R, rays, law=0, coeff=0.0, mu=None, bad=None, dtype=np.float64):
    """The records that pass every test except the time window.  Returns a dict: on (the filter), bad (bad-angle and on the disc), idx (the used
    records), and per used record w (emis limb), tt (the source->disc time, 0 without table_time), fi and fz (the radial-table and zone coordinates,
    NaN where none is taken: for the tests' preconditions)."""
    m = R.spec
    assert m.model == 1
    n = len(rays)
    on = sr.disc_filter(m, rays)
    bad = np.zeros(n, dtype=bool) if bad is None else np.asarray(bad) & on
    keep = on & ~bad if law != 0 else on.copy()
    r = rays["r"]
    w = sr.limb_weight(law, coeff, mu, dtype) if mu is not None else np.ones(n, dtype=dtype)
    emis_table, time_table = sr.table(m.table_emis, m.table_nr), sr.table(R.table_time, m.table_nr)
    tt = np.zeros(n, dtype=dtype)
    fi = np.full(n, np.nan)
    with np.errstate(all="ignore"):
        if emis_table is not None or time_table is not None:
            inside, ir = sr.table_index(m, r, dtype)
            keep &= inside
            rr = np.asarray(r).astype(dtype)
            fi = np.asarray(np.log(rr / dtype(m.table_r_min)) / np.log(dtype(m.table_dr)) if m.table_logbin else (rr - dtype(m.table_r_min)) / dtype(m.table_dr), dtype=np.float64)
        if emis_table is not None:
            emis = np.where(inside, emis_table[ir], np.nan)
            keep &= np.isfinite(emis)
        else:
            emis = lr.powerlaw3(r, m.q1, m.rb1, m.q2, m.rb2, m.q3)
        if time_table is not None:
            delay = np.where(inside, time_table[ir], np.nan)
            keep &= np.isfinite(delay)
            tt = np.where(keep, delay, 0).astype(dtype)
        w = w * np.asarray(emis).astype(dtype)
        fz = np.asarray(m.nz * np.log(np.asarray(r).astype(dtype) / dtype(m.r_isco)) / np.log(dtype(m.r_disc) / dtype(m.r_isco)), dtype=np.float64)
    idx = np.flatnonzero(keep)
    return {"on": on, "bad": bad, "idx": idx, "w": w[idx], "tt": tt[idx], "fi": fi[idx], "fz": fz[idx]}


def response(R, rays, law=0, coeff=0.0, mu=None, bad=None, dtype=np.float64):
    """The rule over records that carry their redshift.  mu, bad: as for spectrum_rules.spectrum.  Returns {"resp" (nt, ne, in dtype), "on_disc", "used",
    "bad_angle", "outside", "used_index", "row" (the time row of every used record, -1 outside), "ft" (float64)}."""
    m = R.spec
    u = used_records(R, rays, law, coeff, mu, bad, dtype)
    idx = u["idx"]
    ft = time_coordinate(R, rays["t"][idx], u["tt"], dtype)
    with np.errstate(all="ignore"):
        inside = (ft >= 0) & (ft < R.nt)                                        # (a NaN fails)
    row = np.where(inside, np.floor(np.where(inside, ft, 0)), -1).astype(np.int64)
    E = sr.energies(m, dtype)
    S = sr.table(m.s, m.nz * m.s_ne)
    resp = np.zeros((R.nt, m.ne), dtype=dtype)
    g, r = rays["redshift"], rays["r"]
    for at in range(0, len(idx), sr.CHUNK):
        sel = slice(at, at + sr.CHUNK)
        j = idx[sel]
        gj = g[j].astype(dtype)
        with np.errstate(all="ignore"):
            c = (u["w"][sel] * (1 / (gj * gj * gj)))[:, None]
            val = c * sr.table_value(m, S, sr.zone_of(m, r[j], dtype), gj, E, dtype)
        for k in np.flatnonzero(row[sel] >= 0):                                  # record by record, in order: the sum of a cell is taken one way
            resp[row[sel][k]] += val[k]
    return {"resp": resp, "on_disc": int(u["on"].sum()), "used": int(len(idx)), "bad_angle": int(u["bad"].sum()), "outside": int((row < 0).sum()),
            "used_index": idx, "row": row, "ft": np.asarray(ft, dtype=np.float64), "fi": u["fi"], "fz": u["fz"]}


def tallies(res):
    return res["on_disc"], res["used"], res["bad_angle"], res["outside"]


def cell_diff(got, want):
    """|got - want| / |want| per cell (0 where both are equal; inf where only one is 0)."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    with np.errstate(all="ignore"):
        return np.where(got == want, 0, np.abs(got - want) / np.abs(want)).astype(np.float64)


def noise(R, rays, **kw):
    """(noise, float64 result, longdouble result): the largest relative difference, over the cells, between the float64 and the longdouble evaluation
    of the rule; the tallies and the rows of the two must agree."""
    lo, hi = response(R, rays, dtype=np.float64, **kw), response(R, rays, dtype=np.longdouble, **kw)
    assert tallies(lo) == tallies(hi) and np.array_equal(lo["row"], hi["row"])
    d = cell_diff(lo["resp"], hi["resp"])
    return (float(d.max()) if d.size else 0.0), lo, hi


def synthetic_records(r, g, t, theta=np.pi / 2, steps=1):
    """Records that carry only what the reduce form reads: steps, r, theta, redshift, t."""
    rays = sr.synthetic_records(r, g, theta, steps)
    rays["t"] = t
    return rays
