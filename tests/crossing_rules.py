"""The equatorial-crossing rule in numpy (TEST INFRASTRUCTURE): what kr_trace_crossings_* must make of a ray, stated independently of the kernel.

The yardstick is not the code under test: a ray's states are its initial record, then the rows of the path recorder (api.trace_paths with
write_step = 1 and an open window, pinned to the reference's own trajectory files and to the strict trace by tests/test_gpu_paths.py), then -- when
the call ended the ray on r <= horizon or on dest->reached(), an iteration that leaves no row -- the (t, r, theta, phi) of its final record.  A
theta-flip iteration moves nothing and leaves no row, so consecutive states are exactly the states either side of every iteration that moved.

Between consecutive states 0 and 1 the rule of include/kr_trace.h applies: crossed iff (theta0 < pi/2 <= theta1) or (theta0 > pi/2 >= theta1);
    f = (pi/2 - theta0) / (theta1 - theta0),   r_c = r0 + f (r1 - r0),   phi_c = phi0 + f (phi1 - phi0),   t_c = t0 + f (t1 - t0)
in float64, one IEEE operation each in this association: r_c, phi_c and t_c are therefore held to the device's BITS.  g comes from the CPU oracle
(oracle_lib.oracle().kro_redshift_f64) on synthetic records at (r_c, pi/2) with the ray's k, h, Q and emit and the final record's signs -- for
motion = 0 the observer's four-velocity has neither an r nor a theta component and the signs do not enter g.

Nothing here runs in the product path."""
import math

import numpy as np

from raytrace_cpu_amd import capi

HALF_PI = math.pi / 2          # M_PI / 2: the same double as the device's kPi2
COLS = ("t", "r", "theta", "phi")


def crossed(before, after):
    """crossed_equator of the trace (raytracer.cpp: the equatorial_crossings counter), elementwise; NaN never crosses."""
    before, after = np.asarray(before, dtype=np.float64), np.asarray(after, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ((before < HALF_PI) & (after >= HALF_PI)) | ((before > HALF_PI) & (after <= HALF_PI))


def interpolate(s0, s1):
    """(r_c, phi_c, t_c) between states s0 and s1, arrays [..., (t, r, theta, phi)]: the four expressions of the rule, in its association."""
    s0, s1 = np.asarray(s0, dtype=np.float64), np.asarray(s1, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = (HALF_PI - s0[..., 2]) / (s1[..., 2] - s0[..., 2])
        r_c = s0[..., 1] + f * (s1[..., 1] - s0[..., 1])
        phi_c = s0[..., 3] + f * (s1[..., 3] - s0[..., 3])
        t_c = s0[..., 0] + f * (s1[..., 0] - s0[..., 0])
    return r_c, phi_c, t_c


def crossings_of_states(states):
    """Every crossing of ONE ray's state sequence [k, (t, r, theta, phi)]: (after, r_c, phi_c, t_c), `after` the index of the state that the crossing
    iteration produced."""
    states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    if len(states) < 2:
        z = np.zeros(0)
        return np.zeros(0, dtype=np.int64), z, z, z
    hit = np.flatnonzero(crossed(states[:-1, 2], states[1:, 2]))
    r_c, phi_c, t_c = interpolate(states[hit], states[hit + 1])
    return hit + 1, r_c, phi_c, t_c


def truncate(n_crossings, max_crossings, stop_when_full):
    """(seen, stored, ended) of a ray that would make n_crossings if left alone: with stop_when_full the ray ends with its M-th crossing."""
    ended = bool(stop_when_full) and n_crossings >= max_crossings
    seen = max_crossings if ended else n_crossings
    return seen, min(seen, max_crossings), ended


def uses_destination(params):
    return params.stop_kind != capi.STOP_THETA


def ray_states(params, init, offsets, rows, final, i):
    """The state sequence of ray i (above)."""
    first = np.array([[init[c][i] for c in COLS]], dtype=np.float64)
    seq = [first, rows[offsets[i]:offsets[i + 1]]]
    added = int(final["status"][i]) & ~int(init["status"][i])
    broke = added & (capi.STATUS_HORIZON | (capi.STATUS_DEST if uses_destination(params) else 0))
    if broke:
        seq.append(np.array([[final[c][i] for c in COLS]], dtype=np.float64))
    return np.concatenate(seq, axis=0)


def all_crossings(params, init, offsets, rows, traced, final):
    """Every crossing of every traced ray, left alone (no truncation): a dict of flat arrays ray, ordinal, after, r_c, phi_c, t_c, in_break (the
    crossing lies in the ray's break iteration: the one that ended on the horizon or the destination), plus n_states per ray."""
    out = {k: [] for k in ("ray", "ordinal", "after", "r_c", "phi_c", "t_c", "in_break")}
    n_states = np.zeros(len(init), dtype=np.int64)
    for i in np.flatnonzero(np.asarray(traced).astype(bool)):
        states = ray_states(params, init, offsets, rows, final, i)
        n_states[i] = len(states)
        after, r_c, phi_c, t_c = crossings_of_states(states)
        has_break = len(states) - 1 > offsets[i + 1] - offsets[i]
        out["ray"].append(np.full(len(after), i, dtype=np.int64))
        out["ordinal"].append(np.arange(len(after), dtype=np.int64))
        out["after"].append(after)
        out["r_c"].append(r_c); out["phi_c"].append(phi_c); out["t_c"].append(t_c)
        out["in_break"].append((after == len(states) - 1) & has_break)
    res = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in out.items()}
    for k in ("ray", "ordinal", "after"):
        res[k] = res[k].astype(np.int64)
    res["in_break"] = res["in_break"].astype(bool)
    res["n_states"] = n_states
    return res


def oracle_g(spin, spec, init, final, ray, r_c):
    """g of crossings at radii r_c of rays `ray` from the CPU oracle: synthetic records at (r_c, pi/2), the final record's signs."""
    import oracle_lib as ol
    rec = np.zeros(len(ray), dtype=capi.RAY_F64)
    rec["r"], rec["theta"] = r_c, HALF_PI
    for f in ("k", "h", "Q", "emit"):
        rec[f] = init[f][ray]
    for f in ("rdot_sign", "thetadot_sign"):
        rec[f] = final[f][ray]
    rec["steps"] = 1
    if len(rec):
        ol.oracle().kro_redshift_f64(spin, spec.V, spec.reverse, spec.projradius, spec.motion, ol.ptr(rec), len(rec))
    return rec["redshift"].copy()


def rule(params, spec, init, offsets, rows, traced, final, found=None):
    """What kr_trace_crossings_* returns for these rays: "rows" [n, M, 4] = {r_c, phi_c, t_c, g}, NaN where nothing is stored; "seen" [n]; "ended" [n]:
    the recorder ended the ray; "end_state" [n, 4]: (t, r, theta, phi) of the iteration that made an ended ray's M-th crossing (NaN otherwise).
    found: all_crossings(...) of the same arguments, to share it between specs."""
    c = found if found is not None else all_crossings(params, init, offsets, rows, traced, final)
    n, M = len(init), int(spec.max_crossings)
    out_rows = np.full((n, M, 4), np.nan)
    seen = np.zeros(n, dtype=np.int32)
    ended = np.zeros(n, dtype=bool)
    end_state = np.full((n, 4), np.nan)
    per_ray = np.bincount(c["ray"], minlength=n)
    for i in np.flatnonzero(per_ray):
        seen[i], _, ended[i] = truncate(int(per_ray[i]), M, spec.stop_when_full)
    keep = c["ordinal"] < M
    ray, m = c["ray"][keep], c["ordinal"][keep]
    g = oracle_g(params.spin, spec, init, final, ray, c["r_c"][keep])
    out_rows[ray, m, 0], out_rows[ray, m, 1], out_rows[ray, m, 2], out_rows[ray, m, 3] = c["r_c"][keep], c["phi_c"][keep], c["t_c"][keep], g
    last = keep & (c["ordinal"] == M - 1) & ended[c["ray"]]
    for i, after in zip(c["ray"][last], c["after"][last]):
        end_state[i] = ray_states(params, init, offsets, rows, final, i)[after]
    return {"rows": out_rows, "seen": seen, "ended": ended, "end_state": end_state}


def pick(bins, rows, seen, order):
    """Which stored crossing of every ray an image of `order` takes, -1 for none: order >= 0 -- that crossing if the ray stored it; order = -1, the
    opaque disc -- the first stored crossing with r_isco <= r_c < r_disc (NaN fails)."""
    n, M = rows.shape[0], rows.shape[1]
    stored = np.minimum(np.asarray(seen, dtype=np.int64), M)
    if order >= 0:
        return np.where(order < stored, order, -1)
    r_c = rows[:, :, 0]
    with np.errstate(invalid="ignore"):
        ok = (r_c >= bins.r_isco) & (r_c < bins.r_disc) & (np.arange(M)[None, :] < stored[:, None])
    return np.where(ok.any(axis=1), ok.argmax(axis=1), -1)


def image_rule(bins, rays, rows, seen, order, lo=-math.pi, hi=math.pi):
    """kr_reduce_crossing_image_dev_f64 in numpy: the chosen crossings as synthetic records (steps = 1, r = r_c, theta = pi/2, phi = range_phi(phi_c),
    t = t_c, redshift = g, the ray's alpha and beta) through the image rule of tests/reducer_rules.py."""
    import reducer_rules as rr
    which = pick(bins, rows, seen, order)
    idx = np.flatnonzero(which >= 0)
    rec = np.zeros(len(idx), dtype=capi.RAY_F64)
    chosen = rows[idx, which[idx]]
    rec["steps"] = 1
    rec["r"], rec["theta"], rec["t"], rec["redshift"] = chosen[:, 0], HALF_PI, chosen[:, 2], chosen[:, 3]
    rec["phi"] = rr.range_phi(chosen[:, 1], rec["steps"], lo, hi)
    rec["alpha"], rec["beta"] = rays["alpha"][idx], rays["beta"][idx]
    return rr.reduce_image(bins, rec)
