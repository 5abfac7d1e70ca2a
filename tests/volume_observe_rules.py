"""The observing rule in numpy (TEST INFRASTRUCTURE): what kr_trace_observe_* must make of a ray's rows, stated independently of the kernel.

The yardstick is not the code under test: the rows are those of the path recorder (api.trace_paths with write_step = 1 and an open window, pinned to the
reference's own trajectory files and to the strict trace by tests/test_gpu_paths.py), the cells come from volume_map_rules.cells_of, the energy shift z
from the CPU oracle on synthetic records (volume_map_rules.oracle_g with volume_map_rules.signs_for), and everything else -- the step displacement, the
proper length, the per-ray optical depth, the weights and the bins -- is the rule of include/kr_trace.h written out here.

`measure` turns rows into per-row quantities (which rows contribute, with what weight, energy and time); `bin_rows` bins them.  They are separate so that
a test can choose its energy and time bins from what the rule finds before it bins."""
import math

import numpy as np

import volume_map_rules as vr

TALLIES = ("rows", "in_grid", "lit", "contributions", "bad_g", "degenerate")


def proper_length(spin, r, theta, dr, dth, dph):
    """l = sqrt((Sigma / Delta) dr^2 + Sigma dtheta^2 + (A sin^2 theta / Sigma) dphi^2) at (r, theta)"""
    a = spin
    sn, cs = np.sin(theta), np.cos(theta)
    sigma = r * r + (a * cs) * (a * cs)
    delta = r * r - 2 * r + a * a
    big_a = (r * r + a * a) * (r * r + a * a) - a * a * delta * sn * sn
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.sqrt((sigma / delta) * dr * dr + sigma * dth * dth + (big_a * sn * sn / sigma) * dph * dph)


def measure(m, spin, offsets, rows, start, z_of, emis, kappa=None, delay=None):
    """Steps 1-5 of the rule for every row.  offsets, rows: a write_step = 1 recording; start[ray] = (r, theta, phi) of the ray's initial record;
    z_of(mask) -> z of the rows in the boolean mask; emis / kappa / delay: one value per cell (kappa, delay may be None).
    Returns a dict: the six tallies, "image" (per ray), and for the CONTRIBUTING rows (in row order) "row" (their indices), "ray", "w", "E", "T", "cell", "len", "tau";
    "t_in_grid": t of every row in the grid."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    n_rays, n = len(offsets) - 1, len(rows)
    ray = vr.ray_of_rows(offsets)
    before = np.empty((n, 3))
    before[1:] = rows[:-1, 1:4]
    nonempty = np.diff(offsets) > 0
    before[offsets[:-1][nonempty]] = np.asarray(start, dtype=np.float64).reshape(-1, 3)[nonempty]
    d = rows[:, 1:4] - before
    cell = vr.cells_of(m, rows)
    inside = cell >= 0
    emis = np.asarray(emis, dtype=np.float64).ravel()
    j, kap, dly = np.zeros(n), np.zeros(n), np.zeros(n)
    j[inside] = emis[cell[inside]]
    if kappa is not None:
        kap[inside] = np.asarray(kappa, dtype=np.float64).ravel()[cell[inside]]
    if delay is not None:
        dly[inside] = np.asarray(delay, dtype=np.float64).ravel()[cell[inside]]
    with np.errstate(invalid="ignore"):
        lit = inside & ((j > 0) | (kap > 0))
    length = proper_length(spin, rows[:, 1], rows[:, 2], d[:, 0], d[:, 1], d[:, 2])
    with np.errstate(invalid="ignore"):
        ok_len = (length > 0) & np.isfinite(length) & (np.abs(d[:, 2]) < np.pi / 2)
    degenerate = lit & ~ok_len
    live = lit & ok_len
    emitting = live & (j > 0)
    z = np.full(n, np.nan)
    z[emitting] = np.asarray(z_of(emitting), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        good = emitting & (z > 0) & np.isfinite(z)
    # tau before the row: the ray's running sum of l kappa over its earlier live rows (sequential, per ray, from 0)
    inc = np.where(live, length * kap, 0.0)
    tau = np.zeros(n)
    for s, e in zip(offsets[:-1], offsets[1:]):
        if e > s + 1:
            tau[s + 1:e] = np.cumsum(inc[s:e - 1])
    E = 1 / z[good]
    w = j[good] * length[good] * E * E * E
    if kappa is not None:
        w = w * np.exp(-tau[good])
    return {"rows": int(n), "in_grid": int(inside.sum()), "lit": int(lit.sum()), "contributions": int(good.sum()), "bad_g": int((emitting & ~good).sum()),
            "degenerate": int(degenerate.sum()), "image": np.bincount(ray[good], weights=w, minlength=n_rays),
            "row": np.flatnonzero(good), "ray": ray[good], "w": w, "E": E, "T": rows[good, 0] + dly[good], "cell": cell[good], "len": length[good], "tau": tau[good],
            "t_in_grid": rows[inside, 0]}


def quotients(b, meas):
    """(q_e, q_t) of the contributing rows; q_t is None when nt == 0"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q_e = np.log(meas["E"] / b.en0) / math.log(b.den) if b.logbin_en else (meas["E"] - b.en0) / b.den
        q_t = (meas["T"] - b.t0) / b.dt if b.nt > 0 else None
    return q_e, q_t


def near_edge_e(rows, eps=1e-9, bins=None):
    """How many contributing rows have a q_e within eps of a whole number (where a last-bit difference between the device's and the oracle's energy
    shift, or of the device's log, moves a row next door).  rows: the q_e themselves, or a measure() result together with `bins`."""
    q_e = quotients(bins, rows)[0] if isinstance(rows, dict) else np.asarray(rows, dtype=np.float64)
    ok = np.isfinite(q_e)
    return int((np.abs(q_e[ok] - np.rint(q_e[ok])) < eps).sum())


def bin_rows(b, meas):
    """The output of the rule: spectrum, hits, response (nen, nt), image and the tallies.  Range tests on q itself."""
    q_e, q_t = quotients(b, meas)
    with np.errstate(invalid="ignore"):
        in_e = (q_e >= 0) & (q_e < b.nen)
    ie = q_e[in_e].astype(np.int64)
    out = {k: meas[k] for k in TALLIES}
    out["image"] = meas["image"]
    out["spectrum"] = np.bincount(ie, weights=meas["w"][in_e], minlength=b.nen)
    out["hits"] = np.bincount(ie, minlength=b.nen).astype(np.float64)
    resp = np.zeros(b.nen * b.nt)
    if b.nt > 0:
        with np.errstate(invalid="ignore"):
            in_t = in_e & (q_t >= 0) & (q_t < b.nt)
        resp = np.bincount(q_e[in_t].astype(np.int64) * b.nt + q_t[in_t].astype(np.int64), weights=meas["w"][in_t], minlength=b.nen * b.nt)
    out["response"] = resp.reshape(b.nen, b.nt)
    return out


def measure_recording(m, spin, init, offsets, rows, emis, kappa=None, delay=None):
    """measure() for a write_step = 1 recording (offsets, rows) of the rays `init`, z from the CPU oracle."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    signs = vr.signs_for(m, init, offsets, rows)
    start = np.stack([init["r"], init["theta"], init["phi"]], axis=1)
    return measure(m, spin, offsets, rows, start, lambda which: vr.oracle_g(m, spin, init, offsets, rows, which, signs), emis, kappa, delay)


def worst_rel(got, want):
    g, w = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    if g.shape != w.shape:
        return float("inf")
    rel = np.where(g == w, 0.0, np.abs(g - w) / np.maximum(np.abs(w), 1e-300))
    return float(rel.max()) if len(rel) else 0.0


def compare(got, want, rtol):
    """Problems (empty = pass): hits and the six tallies equal; spectrum, response and image (where got has one) within rtol relative."""
    problems = []
    for k in TALLIES:
        if int(got[k]) != int(want[k]):
            problems.append((k, int(got[k]), int(want[k])))
    if got["hits"].shape != want["hits"].shape or not np.array_equal(got["hits"], want["hits"]):
        problems.append(("hits", got["hits"].tolist(), want["hits"].tolist()))
    for k in ("spectrum", "response", "image"):
        if k == "image" and got.get("image") is None:
            continue
        rel = worst_rel(got[k], want[k])
        if not rel <= rtol:
            problems.append((k, rel))
    return problems
