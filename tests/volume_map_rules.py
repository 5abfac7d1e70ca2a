"""The volume-map rule in numpy (TEST INFRASTRUCTURE): what kr_trace_volume_* must make of a ray's rows, stated independently of the kernel.

The yardstick is not the code under test: the rows are those of the path recorder (api.trace_paths with write_step = 1 and an open window, pinned to the
reference's own trajectory files and to the strict trace by tests/test_gpu_paths.py), binned here by the rule of include/kr_trace.h, with the energy
shift g from the CPU oracle (oracle_lib.oracle().kro_redshift_f64) on synthetic records: r, theta, phi from the row; k, h, Q, emit from the ray;
the signs as `signs_for` gives them.

Every axis quotient except the logarithmic one is a single IEEE operation on both sides (csrc is built with -ffp-contract=off), so cells -- hence
counts and tallies -- are exact; time and redshift are sums in another order."""
import math

import numpy as np

from raytrace_cpu_amd import capi

PLANES = ("count", "time", "redshift")
TALLIES = ("rows", "in_grid", "deposits", "bad_g")


def quotients(m, rows):
    """(q_r, q_th, q_ph) of rows[:, (t, r, theta, phi)]; q_ph is None for nphi == 1 (no phi test, no wrap)."""
    r, theta, phi = rows[:, 1], rows[:, 2], rows[:, 3]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q_r = np.log(r / m.r_min) / math.log(m.dr) if m.logbin else (r - m.r_min) / m.dr
        q_th = theta / m.dtheta
        if m.nphi == 1:
            return q_r, q_th, None
        phi_w = phi - (2 * np.pi) * np.floor((phi + np.pi) / (2 * np.pi))
        q_ph = (phi_w + np.pi) / m.dphi
    return q_r, q_th, q_ph


def cells_of(m, rows):
    """The cell of every row, -1 outside the grid: 0 <= q < n on every axis, decided on q itself (NaN and infinities are outside)."""
    q_r, q_th, q_ph = quotients(m, rows)
    with np.errstate(invalid="ignore"):
        inside = (q_r >= 0) & (q_r < m.nr) & (q_th >= 0) & (q_th < m.ntheta)
        if q_ph is not None:
            inside &= (q_ph >= 0) & (q_ph < m.nphi)
    cell = np.full(len(rows), -1, dtype=np.int64)
    ir, ith = q_r[inside].astype(np.int64), q_th[inside].astype(np.int64)
    iph = q_ph[inside].astype(np.int64) if q_ph is not None else 0
    cell[inside] = (ir * m.ntheta + ith) * m.nphi + iph
    return cell


def near_edge(m, rows, eps=1e-9):
    """How many in-range radial quotients sit within eps of a whole number (where a last-bit difference of the device's log moves a row next door)."""
    q_r = quotients(m, rows)[0]
    ok = np.isfinite(q_r) & (q_r > -1) & (q_r < m.nr + 1)
    return int((np.abs(q_r[ok] - np.rint(q_r[ok])) < eps).sum())


def ray_of_rows(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def due_rows(m, offsets, cell):
    """mode 0: a row is due iff it is in the grid and its cell differs from the ray's previous row's (-1 before the first row and after a row outside
    the grid); mode 1: every row in the grid."""
    if m.mode == 1:
        return cell >= 0
    prev = np.empty_like(cell)
    prev[1:] = cell[:-1]
    first = offsets[:-1][np.diff(offsets) > 0]
    prev[first] = -1
    return (cell >= 0) & (cell != prev)


def signs_for(m, init, offsets, rows):
    """(rdot_sign, thetadot_sign) per row.  motion = 0: the observer's four-velocity has no r or theta component and neither sign enters g: +1.
    motion = 1: rdot_sign = sign(r_row - r_previous), the previous position being the previous row or the ray's initial record -- exact for an
    Euler update, whose r moves by pr * step with the sign the step used.  A zero difference has no sign: refused."""
    n = len(rows)
    one = np.ones(n, dtype=np.int32)
    if m.motion == 0:
        return one, one
    prev_r = np.empty(n)
    prev_r[1:] = rows[:-1, 1]
    nonempty = np.diff(offsets) > 0
    prev_r[offsets[:-1][nonempty]] = init["r"][nonempty]
    d = rows[:, 1] - prev_r
    if (d == 0).any():
        raise AssertionError(f"{int((d == 0).sum())} rows did not move in r: sign(r_row - r_previous) is undefined")
    return np.where(d > 0, 1, -1).astype(np.int32), one


def oracle_g(m, spin, init, offsets, rows, which, signs):
    """g of the rows `which` (a boolean mask) from the CPU oracle on synthetic records."""
    import oracle_lib as ol
    idx = np.flatnonzero(which)
    ray = ray_of_rows(offsets)[idx]
    rec = np.zeros(len(idx), dtype=capi.RAY_F64)
    rec["r"], rec["theta"], rec["phi"] = rows[idx, 1], rows[idx, 2], rows[idx, 3]
    for f in ("k", "h", "Q", "emit"):
        rec[f] = init[f][ray]
    rec["rdot_sign"], rec["thetadot_sign"] = signs[0][idx], signs[1][idx]
    rec["steps"] = 1
    if len(rec):
        ol.oracle().kro_redshift_f64(spin, m.V, m.reverse, m.projradius, m.motion, ol.ptr(rec), len(rec))
    return rec["redshift"].copy()


def bin_rows(m, offsets, rows, g_of):
    """The map of rows under the rule.  g_of(due mask) -> g of the due rows.  Returns count / time / redshift shaped (nr, ntheta, nphi) and the tallies."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    ncell = m.nr * m.ntheta * m.nphi
    cell = cells_of(m, rows)
    due = due_rows(m, offsets, cell)
    g = np.asarray(g_of(due), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        good = (g > 0) & np.isfinite(g)
    at = cell[due][good]
    shape = (m.nr, m.ntheta, m.nphi)
    out = {"count": np.bincount(at, minlength=ncell).astype(np.float64).reshape(shape),
           "time": np.bincount(at, weights=rows[due, 0][good], minlength=ncell).reshape(shape),
           "redshift": np.bincount(at, weights=g[good], minlength=ncell).reshape(shape),
           "rows": int(len(rows)), "in_grid": int((cell >= 0).sum()), "deposits": int(good.sum()), "bad_g": int((~good).sum())}
    return out


def rule(m, spin, init, offsets, rows):
    """The map the device must produce for a write_step = 1 recording (offsets, rows) of the rays `init`."""
    offsets = np.asarray(offsets, dtype=np.int64)
    signs = signs_for(m, init, offsets, rows)
    return bin_rows(m, offsets, rows, lambda due: oracle_g(m, spin, init, offsets, rows, due, signs))


def add_maps(a, b):
    return {k: a[k] + b[k] for k in PLANES + TALLIES}


def compare(got, want, rtol):
    """Problems (empty = pass): count and the four tallies equal, time and redshift within rtol relative, cell by cell."""
    problems = []
    for k in TALLIES:
        if int(got[k]) != int(want[k]):
            problems.append((k, int(got[k]), int(want[k])))
    if got["count"].shape != want["count"].shape or not np.array_equal(got["count"], want["count"]):
        problems.append(("count", int((got["count"] != want["count"]).sum()) if got["count"].shape == want["count"].shape else got["count"].shape))
        return problems
    for k in ("time", "redshift"):
        g, w = got[k], want[k]
        rel = np.where(g == w, 0.0, np.abs(g - w) / np.maximum(np.abs(w), 1e-300))
        if (rel > rtol).any():
            problems.append((k, float(rel.max()), int(np.argmax(rel))))
    return problems
