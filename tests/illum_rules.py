"""TEST INFRASTRUCTURE: the (r, phi) illumination map of the disc (include/kr_trace.h, kr_illum_bins; csrc/kr_illum.hip) restated in numpy over ray
records, in the manner of tests/reducer_rules.py, whose filter, radial quotient, index rule and exact per-bin sums it takes as they are.  Nothing here
runs in the product path.

The azimuthal rule is stated on the floating quotient, like the radial one: with dphi = 2 pi / nphi rounded once,
    p = phi + phi_shift;   phi_w = p - 2 pi floor((p + pi) / (2 pi));   q_ph = (phi_w + pi) / dphi
a record is binned iff q_ph >= 0 (a NaN fails, and an infinite phi gives one), at ip = min(trunc(q_ph), nphi - 1): a p one ulp below -pi wraps to
just below pi, where q_ph rounds to nphi itself, and that is the last cell; a p one ulp below pi has p + pi round up to 2 pi, wraps to one ulp below -pi
and fails the test (tests/test_illum_rules.py has the table).  With nphi == 1 there is no phi test, ip = 0.  Every operation of it is one IEEE
operation on both sides, so the device's cell is the rule's cell; the radial quotient goes through a log with logbin, and edge_margin() is how a test
shows that no record it uses sits within 1e-9 of a cell edge on either axis."""
import math

import numpy as np

import reducer_rules as rr

PLANES = ("count", "flux", "emis", "sum_redshift", "sum_time")
SUMS = rr.EMIS_SUMS
TWO_PI = 2 * math.pi


def phi_quotient(m, phi):
    """q_ph of the records' phi (NaN for a NaN or infinite phi); with nphi == 1 there is no quotient: zeros."""
    phi = np.asarray(phi, dtype=np.float64)
    if m.nphi == 1:
        return np.zeros(len(phi))
    dphi = TWO_PI / m.nphi
    with np.errstate(invalid="ignore"):
        p = phi + np.float64(m.phi_shift)
        phi_w = p - TWO_PI * np.floor((p + math.pi) / TWO_PI)
        return (phi_w + math.pi) / dphi


def phi_index(m, phi):
    """(binned, ip) of the records' phi."""
    q = phi_quotient(m, phi)
    with np.errstate(invalid="ignore"):
        ok = q >= 0
    return ok, np.minimum(np.trunc(np.where(ok, q, 0.0)).astype(np.int64), m.nphi - 1)


def per_ray(m, rays):
    """Per record: on_disc (the filter of kr_emis_bins), binned, cell (0 where not binned), and the two quotients q, q_ph."""
    b = m.rad
    on_disc = rr.emissivity_filter(b, rays)
    q = rr.emissivity_quotient(b, rays["r"])
    ok_r, ir = rr.bin_index(q, b.nr)
    ok_p, ip = phi_index(m, rays["phi"])
    binned = on_disc & ok_r & ok_p
    return {"on_disc": on_disc, "binned": binned, "cell": np.where(binned, ir * m.nphi + ip, 0), "q": q, "q_ph": phi_quotient(m, rays["phi"])}


def reduce_illum(m, rays):
    """api.reduce_illum in numpy: count (int64), flux, emis, sum_redshift, sum_time shaped (nr, nphi) (raw sums, exact per cell), disc_count, binned;
    plus "abs" (the per-cell sums of absolute terms) and "rays" (per_ray)."""
    b = m.rad
    ncell = b.nr * m.nphi
    pr = per_ray(m, rays)
    sel = pr["binned"]
    cell, g, t = pr["cell"][sel], rays["redshift"][sel], rays["t"][sel]
    with np.errstate(all="ignore"):
        terms = {"flux": 1 / (b.num_primary_rays * g ** 1.0), "emis": 1 / g ** b.gamma, "sum_redshift": g, "sum_time": t}
    shape = (b.nr, m.nphi)
    out = {"count": np.bincount(cell, minlength=ncell).astype(np.int64).reshape(shape), "disc_count": int(pr["on_disc"].sum()), "binned": int(sel.sum()),
           "abs": {}, "rays": pr}
    for k in SUMS:
        total, total_abs = rr.bin_sums(cell, terms[k], ncell)
        out[k], out["abs"][k] = total.reshape(shape), total_abs.reshape(shape)
    return out


def edge_margin(want, logbin):
    """The smallest distance of a binned record's quotient to an integer: q_ph always (nphi > 1), q where it went through a log.  inf without such a
    record.  A linear radial quotient is IEEE-exact on both sides and may sit on an edge."""
    pr = want["rays"]
    gaps = [np.inf]
    sel = pr["binned"]
    if want["count"].shape[1] > 1:
        q = pr["q_ph"][sel]
        gaps.append(np.abs(q - np.rint(q)).min() if q.size else np.inf)
    if logbin:
        q = pr["q"][sel]
        q = q[q != 0]                                      # (r == r_min: log(1) = 0 exactly)
        gaps.append(np.abs(q - np.rint(q)).min() if q.size else np.inf)
    return float(min(gaps))


def summed_over_phi(res):
    """The map as a radial histogram: the planes summed over ip, in the layout reducer_rules.reduce_emissivity returns (with "abs" when the map has it)."""
    out = {k: np.asarray(res[k]).sum(axis=1) for k in PLANES}
    out["disc_count"] = res["disc_count"]
    if "abs" in res:
        out["abs"] = {k: res["abs"][k].sum(axis=1) for k in SUMS}
    return out


def check_illum(got, want, rtol, label=""):
    """The bar of the map tests, `want` from reduce_illum: counts and both tallies exact (no slack, no cell left out), every sum within rtol of the
    per-cell sum of absolute terms, non-finite cells alike.  Returns the worst relative sum error."""
    flat = lambda d: {k: (np.asarray(v).reshape(-1) if k in PLANES else v) for k, v in d.items() if k != "abs"}      # noqa: E731
    g, w = flat(got), flat(want)
    w["abs"] = {k: want["abs"][k].reshape(-1) for k in SUMS}
    assert got["binned"] == want["binned"], (label, got["binned"], want["binned"])
    return rr.check_reduction(g, w, "count", SUMS, rtol, label)


def table_from_map(res, areas):
    """api.illumination_table's two planes from a map: emis = emis_sum / (areas[ir] / nphi), time = sum_time / count, NaN where count == 0."""
    nr, nphi = res["emis"].shape
    with np.errstate(invalid="ignore", divide="ignore"):
        emis = res["emis"] / (np.asarray(areas, dtype=np.float64) / nphi)[:, None]
        time = np.where(res["count"] > 0, res["sum_time"] / res["count"], np.nan)
    return emis, time


# ---- the map as an (r, phi) table of the line and the response (include/kr_trace.h, kr_illum_table) ---------------------------------------------------
# T below is anything with r_min, dr, logbin, phi_shift, nphi and the planes: a capi.IllumTable (planes read through its pointers) or a Table.
class Table:
    """The table as the rules read it; emis, time: (nr, nphi) arrays, time may be None."""

    def __init__(self, emis, r_min, dr, logbin=1, time=None, phi_shift=0.0):
        self.emis, self.time = np.asarray(emis, dtype=np.float64), (None if time is None else np.asarray(time, dtype=np.float64))
        self.nr, self.nphi = self.emis.shape
        self.r_min, self.dr, self.logbin, self.phi_shift = float(r_min), float(dr), int(logbin), float(phi_shift)

    def struct(self):
        from raytrace_cpu_amd import capi
        return capi.illum_table(self.emis, self.r_min, self.dr, logbin=self.logbin, time=self.time, phi_shift=self.phi_shift)


def table_lookup(T, r, phi, dtype=np.float64):
    """Per record: (used, emis, tt, fi, q_ph).  used: the record has a ring (-1 < fi < nr), a cell (q_ph >= 0) and finite emis and tt there."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        rr_ = r.astype(dtype)
        fi = np.asarray(np.log(rr_ / dtype(T.r_min)) / np.log(dtype(T.dr)) if T.logbin else (rr_ - dtype(T.r_min)) / dtype(T.dr), dtype=np.float64)
        ok_r = (fi > -1) & (fi < T.nr)
    ir = np.trunc(np.where(ok_r, fi, 0.0)).astype(np.int64)
    ok_p, ip = phi_index(T, phi)
    q_ph = phi_quotient(T, phi)
    ok = ok_r & ok_p
    cell = (np.where(ok, ir, 0), np.where(ok, ip, 0))
    emis = np.where(ok, T.emis[cell], np.nan)
    tt = np.where(ok, T.time[cell], np.nan) if T.time is not None else np.where(ok, 0.0, np.nan)
    used = ok & np.isfinite(emis) & np.isfinite(tt)
    return used, emis, tt, fi, q_ph


def line_from_rays(b, T, rays):
    """kr_reduce_line_illum_dev_f64 in numpy (line_rules.line_from_rays with emis and tt from the table), on records after redshift(-1, reverse=1).
    Also returns "fi", "q_ph", "fe", "ft" of the used records, for the tests' preconditions."""
    import line_rules as lr
    m = lr.disc_filter(b, rays)
    r, g, t, phi = rays["r"][m], rays["redshift"][m], rays["t"][m], rays["phi"][m]
    used, emis, tt, fi, q_ph = table_lookup(T, r, phi)
    with np.errstate(all="ignore"):
        E = b.line_energy / g
        w = emis * np.power(g, -1 * b.g_index)
        tau = t + tt - b.t0
        fe = np.log(E / b.e_min) / np.log(b.de) if b.log_e else (E - b.e_min) / b.de
        ft = tau / b.dt if lr.has_time_axis(b) else np.zeros_like(tau)
    out = lr.bin_items(b, E, w, tau, used, m.sum())
    out.update(fi=fi[used], q_ph=q_ph[used], fe=fe[used], ft=ft[used], used=int(used.sum()))
    return out


def response(R, T, rays, dtype=np.float64):
    """kr_reduce_response_illum_dev_f64 in numpy: response_rules.response (isotropic) with emis and tt from the table; the same result dict."""
    import response_rules as rsp
    import spectrum_rules as sr
    m = R.spec
    assert m.model == 1 and not m.table_emis and not R.table_time
    on = sr.disc_filter(m, rays)
    used, emis, tt, fi, q_ph = table_lookup(T, rays["r"], rays["phi"], dtype)
    keep = on & used
    idx = np.flatnonzero(keep)
    r, g = rays["r"], rays["redshift"]
    with np.errstate(all="ignore"):
        fz = np.asarray(m.nz * np.log(np.asarray(r).astype(dtype) / dtype(m.r_isco)) / np.log(dtype(m.r_disc) / dtype(m.r_isco)), dtype=np.float64)
    w = emis[idx].astype(dtype)
    ft = rsp.time_coordinate(R, rays["t"][idx], tt[idx], dtype)
    with np.errstate(all="ignore"):
        inside = (ft >= 0) & (ft < R.nt)
    row = np.where(inside, np.floor(np.where(inside, ft, 0)), -1).astype(np.int64)
    E = sr.energies(m, dtype)
    S = sr.table(m.s, m.nz * m.s_ne)
    resp = np.zeros((R.nt, m.ne), dtype=dtype)
    for at in range(0, len(idx), sr.CHUNK):
        sel = slice(at, at + sr.CHUNK)
        j = idx[sel]
        gj = g[j].astype(dtype)
        with np.errstate(all="ignore"):
            c = (w[sel] * (1 / (gj * gj * gj)))[:, None]
            val = c * sr.table_value(m, S, sr.zone_of(m, r[j], dtype), gj, E, dtype)
        for k in np.flatnonzero(row[sel] >= 0):
            resp[row[sel][k]] += val[k]
    return {"resp": resp, "on_disc": int(on.sum()), "used": int(len(idx)), "bad_angle": 0, "outside": int((row < 0).sum()), "used_index": idx, "row": row,
            "ft": np.asarray(ft, dtype=np.float64), "fi": fi[idx], "fz": fz[idx], "q_ph": q_ph[idx]}


def response_noise(R, T, rays):
    """(noise, float64 result, longdouble result): response_rules.noise for the table flavour."""
    import response_rules as rsp
    lo, hi = response(R, T, rays, np.float64), response(R, T, rays, np.longdouble)
    assert rsp.tallies(lo) == rsp.tallies(hi) and np.array_equal(lo["row"], hi["row"])
    d = rsp.cell_diff(lo["resp"], hi["resp"])
    return (float(d.max()) if d.size else 0.0), lo, hi
