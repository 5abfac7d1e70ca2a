"""TEST INFRASTRUCTURE: the disc flow "Keplerian, plunging inside the ISCO" (include/kr_trace.h, KR_V_PLUNGE) restated in numpy on top of
tests/angle_rules.py (metric, momentum_from_consts, dot_product).  Nothing here runs in the product path.

V == V_PLUNGE with motion = 0: at r >= r_ms = kr_kerr_isco(a, +1) (a = reverse ? -spin : spin) the observer and frame of V = -1; at r < r_ms the gas
on the equatorial geodesic that left the circular orbit at r_ms with its energy E_ms and angular momentum L_ms.  e_t = u, e2 = (0, 0, 1 / sqrt(rhosq), 0),
e3 (r-like) and e1 (phi-like) by Gram-Schmidt against the metric, seeds d/dr then d/dphi, oriented e3^r > 0 and e1^phi > 0.  Every function takes a
dtype so that the same rule runs in np.longdouble: the difference between the two is the rounding noise of the rule on those records."""
import contextlib
import ctypes as C

import numpy as np

import angle_rules as ar

V_PLUNGE = -2.0


def r_ms(a):
    """The project's float-rounded ISCO (kr_kerr_isco; no GPU needed), the radius at which the flow changes."""
    from raytrace_cpu_amd import api
    return float(api.lib().kr_kerr_isco(float(a), 1))


def flow(a, dtype=np.float64):
    """(r_ms, E_ms, L_ms): energy and angular momentum of the circular orbit at r_ms, every square root in `dtype`."""
    rm = dtype(r_ms(a))
    a = dtype(a)
    u = 1 / rm
    E = (1 - 2 * u + a * u * np.sqrt(u)) / np.sqrt(1 - 3 * u + 2 * a * u * np.sqrt(u))
    L = (1 + a * a * u * u - 2 * a * u * np.sqrt(u)) / np.sqrt(u * (1 - 3 * u + 2 * a * u * np.sqrt(u)))
    return rm, E, L


def radicand(r, a, dtype=np.float64):
    """(u^r)^2 of the plunging geodesic before the clamp at 0."""
    _, k, h = flow(a, dtype)
    r, a = np.asarray(r, dtype=dtype), dtype(a)
    return k * k - 1 + 2 / r + (a * a * (k * k - 1) - h * h) / (r * r) + 2 * (h - a * k) * (h - a * k) / (r * r * r)


def velocity(r, a, dtype=np.float64):
    """[u^t, u^r, u^theta, u^phi] of the plunging geodesic at r (arrays), whatever r is: the caller applies r < r_ms."""
    _, k, h = flow(a, dtype)
    r, a = np.asarray(r, dtype=dtype), dtype(a)
    delta = r * r - 2 * r + a * a
    rad = radicand(r, a, dtype)
    with np.errstate(all="ignore"):
        ut = ((r * r + a * a + 2 * a * a / r) * k - 2 * a * h / r) / delta
        ur = -1 * np.sqrt(np.where(rad > 0, rad, dtype(0)))
        uphi = (2 * a * k / r + (1 - 2 / r) * h) / delta
    return [ut, ur, np.zeros_like(r), uphi]


def circular_velocity(r, a, dtype=np.float64):
    """The e_t of the V = -1 observer on the equatorial plane (Omega = 1 / (a + r sqrt(r)))."""
    r, a = np.asarray(r, dtype=dtype), dtype(a)
    g, c = ar.metric(r, np.full_like(r, np.pi / 2), a)
    V = 1 / (a + r * np.sqrt(r))
    et, _, _, _ = ar.tetrad(c, V)
    return et


def legs(g, u):
    """(e1, e3): the phi-like and r-like legs of the observer u by Gram-Schmidt, projections removed leg by leg before any leg is normalised."""
    zero, one = np.zeros_like(u[0]), np.ones_like(u[0])
    seed_r, seed_phi = [zero, one, zero, zero], [zero, zero, zero, one]
    with np.errstate(all="ignore"):
        uu = ar.dot_product(g, u, u)
        c3 = ar.dot_product(g, seed_r, u) / uu
        v3 = [seed_r[c] - c3 * u[c] for c in range(4)]
        n3 = ar.dot_product(g, v3, v3)
        c1, c13 = ar.dot_product(g, seed_phi, u) / uu, ar.dot_product(g, seed_phi, v3) / n3
        v1 = [(seed_phi[c] - c1 * u[c]) - c13 * v3[c] for c in range(4)]
        n1 = ar.dot_product(g, v1, v1)
        l3 = np.where(v3[1] < 0, -1, 1) * np.sqrt(np.abs(n3))
        l1 = np.where(v1[3] < 0, -1, 1) * np.sqrt(np.abs(n1))
        return [v1[c] / l1 for c in range(4)], [v3[c] / l3 for c in range(4)]


def tetrad_at(r, theta, a, dtype=np.float64):
    """(g, [et, e1, e2, e3]) of the plunging gas at (r, theta) -- all four legs, for the identities."""
    r, theta = np.asarray(r, dtype=dtype), np.asarray(theta, dtype=dtype)
    g, c = ar.metric(r, theta, dtype(a))
    u = velocity(r, a, dtype)
    e1, e3 = legs(g, u)
    zero = np.zeros_like(r)
    return g, [u, e1, [zero, zero, 1 / np.sqrt(c["rhosq"]), zero], e3]


def inside(rays, spin, reverse):
    """The records the plunging side of the rule applies to: r < r_ms of the metric's a (a NaN is outside)."""
    a = -spin if reverse else spin
    with np.errstate(invalid="ignore"):
        return rays["r"] < r_ms(a)


def frame(rays, spin, V=-1.0, reverse=0, projradius=0, dtype=np.float64):
    """angle_rules.frame for any V but V_PLUNGE; for V_PLUNGE its V = -1 outside r_ms and the plunging gas inside."""
    if V != V_PLUNGE:
        assert dtype is np.float64
        return ar.frame(rays, spin, V, reverse, projradius)
    if dtype is np.float64:
        out = ar.frame(rays, spin, -1.0, reverse, projradius)
    else:
        out = {k: np.full(len(rays), np.nan, dtype=dtype) for k in ("E", "P_r", "P_th", "P_phi")}
        out["live"] = rays["steps"] > 0
    ins = inside(rays, spin, reverse)
    if not ins.any():
        return out
    sub = rays[ins]
    a = dtype(-spin if reverse else spin)
    r, theta = sub["r"].astype(dtype), sub["theta"].astype(dtype)
    with np.errstate(all="ignore"):
        g, (et, e1, e2, e3) = tetrad_at(r, theta, a, dtype)
        p = ar.momentum_from_consts(sub["k"].astype(dtype), sub["h"].astype(dtype), sub["Q"].astype(dtype), sub["rdot_sign"], sub["thetadot_sign"], r, theta,
                                    dtype(spin))
        if reverse:
            p = [p[0], -1 * p[1], -1 * p[2], -1 * p[3]]
        vals = {"E": ar.dot_product(g, et, p), "P_phi": -1 * ar.dot_product(g, e1, p), "P_th": -1 * ar.dot_product(g, e2, p), "P_r": -1 * ar.dot_product(g, e3, p)}
    live = sub["steps"] > 0
    for k, v in vals.items():
        out[k] = out[k].copy()
        out[k][ins] = np.where(live, v, np.nan)
    return out


@contextlib.contextmanager
def _plunge_frame():
    """angle_rules' histogram rules call the module's frame(): while this is open they see the plunge frame (V_PLUNGE) and angle_rules.frame itself for
    every other V."""
    kept = ar.frame

    def either(rays, spin, V=-1.0, reverse=0, projradius=0):
        return frame(rays, spin, V, reverse, projradius) if V == V_PLUNGE else kept(rays, spin, V, reverse, projradius)

    ar.frame = either
    try:
        yield
    finally:
        ar.frame = kept


def line_limb_rule(*args, **kw):
    """angle_rules.line_limb_rule with the frame above (law 0: the plain line, whose only input from the frame is the redshift)."""
    with _plunge_frame():
        return ar.line_limb_rule(*args, **kw)


def emissivity_mu_rule(*args, **kw):
    """angle_rules.emissivity_mu_rule with the frame above."""
    with _plunge_frame():
        return ar.emissivity_mu_rule(*args, **kw)


def redshift_rule(rays, spin, V, reverse, projradius=0, dtype=np.float64):
    f = frame(rays, spin, V, reverse, projradius, dtype)
    with np.errstate(all="ignore"):
        return f["E"] / rays["emit"].astype(dtype) if reverse else rays["emit"].astype(dtype) / f["E"]


def noise(rays, spin, reverse, projradius=0):
    """{"g", "mu", "chi"}: |float64 rule - longdouble rule| on the records inside r_ms with steps > 0 and finite values -- the rounding noise of the
    rule's own expressions there (largest where Delta -> 0)."""
    ins = inside(rays, spin, reverse) & (rays["steps"] > 0)
    sub = rays[ins]
    lo, hi = frame(sub, spin, V_PLUNGE, reverse, projradius), frame(sub, spin, V_PLUNGE, reverse, projradius, dtype=np.longdouble)
    out = {}
    with np.errstate(all="ignore"):
        pairs = {"mu": (np.abs(lo["P_th"]) / lo["E"], np.abs(hi["P_th"]) / hi["E"]), "chi": (np.arctan2(lo["P_phi"], lo["P_r"]), np.arctan2(hi["P_phi"], hi["P_r"])),
                 "g": (redshift_rule(sub, spin, V_PLUNGE, reverse, projradius), redshift_rule(sub, spin, V_PLUNGE, reverse, projradius, np.longdouble))}
        for k, (x, y) in pairs.items():
            d = np.abs(x.astype(np.longdouble) - y)
            if k == "g":
                d = d / np.abs(y)
            fin = np.isfinite(d)
            out[k] = np.zeros(len(rays))
            vals = np.where(fin, d, 0).astype(np.float64)
            out[k][ins] = vals
    return out


def helper_flow(spin):
    """kr_plunge_flow through ctypes."""
    from raytrace_cpu_amd import api
    v = [C.c_double() for _ in range(3)]
    rc = api.lib().kr_plunge_flow(float(spin), *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)
