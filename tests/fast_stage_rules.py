"""One stage evaluation of the fast RK4 step as a numpy rule (TEST INFRASTRUCTURE; tests/test_gpu_fast_stage_terms.py).

The stage (raytrace_cpu_amd/csrc/kr_device.hpp::step_fixed, kr_fast.hpp::sincos_near / potentials_fast) takes the sine and the cosine of the stage angle
theta0 + d by angle addition from the base point's pair, squares them (s2, c2) and evaluates the separated potentials:

    P = (r^2 + a^2) k - a h      rho^2 = r^2 + a^2 c2      Delta = r^2 + a^2 - 2 r      PD = P / (rho^2 Delta)
    tdot   = (r^2 + a^2) PD - (a (a k) s2 - a h) / rho^2           N = Q + c2 ((a k)^2 - h^2 / s2)       thetadot = sign sqrt(max(|N|, 1e-300)) / rho^2
    phidot = a PD + (h / s2 - a k) / rho^2                         R = P^2 - Delta (Q + (h - a k)^2) - Delta (|N| - N)      rdot = sign sqrt(max(|R|, 1e-300)) / rho^2

Every function takes a `dtype`: np.float64 evaluates the rule in the device's number format, np.longdouble the same rule with a 64-bit mantissa; their
difference is the rule's rounding noise on those points (the convention of the response and spectrum rules).  Beside each value the rule returns the
MAGNITUDE of the terms that were summed into it: what the number format alone allows is a few spacings of THAT, not of a result that may be a
cancellation (floors())."""
import numpy as np

COLUMNS = ("r", "theta0", "d", "k", "h", "Q", "a", "signs")       # one probe group: include/kr_trace.h, kr_debug_arith_f64 op 29
EPS = 2.0 ** -52
# Roundings between the inputs and an output, in half-spacings (2^-53) of the summed terms: on the device at most ~12 -- rho^2, rho^2 Delta, its product
# with s2, the refined reciprocal (<= 1 ulp), two products for 1 / rho^2 or 1 / s2, the inner fused sum, its product, the outer fused sum, and for the two
# roots fast_sqrt (<= 1 ulp) and two products -- and ~4 on the float64 rule, which divides directly.  16 half-spacings = 8 EPS.
FLOOR_EPS = 8.0


def pair(p, dtype):
    """(sine, cosine of the stage angle by the angle addition of sincos_near, magnitudes of their terms); cos d - 1 as -2 sin^2(d / 2), free of cancellation."""
    th0, d = p["theta0"].astype(dtype), p["d"].astype(dtype)
    s0, c0, sd = np.sin(th0), np.cos(th0), np.sin(d)
    cm = -2 * np.sin(d / 2) ** 2
    return (c0 * sd + (s0 * cm + s0), (c0 * cm + c0) - s0 * sd,
            np.abs(c0 * sd) + np.abs(s0 * cm) + np.abs(s0), np.abs(s0 * sd) + np.abs(c0 * cm) + np.abs(c0))


def stage(p, s, c, dtype):
    """{name: value}, {name: magnitude} of tdot, rdot, thetadot, phidot (and N, R, c2) from the sine s and the cosine c of the stage angle; tdot_two / phidot_two: the
    association with (r^2 + a^2) P and a P formed first, two products with 1 / (rho^2 Delta)."""
    r, k, h, Q, a = (p[n].astype(dtype) for n in ("r", "k", "h", "Q", "a"))
    code = p["signs"].astype(np.int64)
    sg_r, sg_th = np.where(code & 1, -1.0, 1.0).astype(dtype), np.where(code & 2, -1.0, 1.0).astype(dtype)
    s, c = s.astype(dtype), c.astype(dtype)
    with np.errstate(all="ignore"):
        s2 = s * s
        c2 = c * c
        r2a2 = r * r + a * a
        rhosq = a * a * c2 + r * r
        delta = r2a2 - 2 * r
        ak, ah = a * k, a * h
        inv_rd, inv_rho, inv_s2 = 1 / (rhosq * delta), 1 / rhosq, 1 / s2
        P, P_mag = r2a2 * k - ah, np.abs(r2a2 * k) + np.abs(ah)
        PD = P * inv_rd
        t2, t2_mag = (a * ak * s2 - ah) * inv_rho, (np.abs(a * ak * s2) + np.abs(ah)) * np.abs(inv_rho)
        p2, p2_mag = (h * inv_s2 - ak) * inv_rho, (np.abs(h * inv_s2) + np.abs(ak)) * np.abs(inv_rho)
        n1 = ak * ak - h * h * inv_s2
        N, N_mag = c2 * n1 + Q, np.abs(Q) + np.abs(c2) * (ak * ak + h * h * inv_s2)
        hmak = h - ak
        R = P * P - delta * (Q + hmak * hmak) - delta * (np.abs(N) - N)
        R_mag = P_mag * P_mag + np.abs(delta) * (np.abs(Q) + (np.abs(h) + np.abs(ak)) ** 2) + 2 * np.abs(delta) * np.abs(N)
        tiny = dtype(1e-300)
        val = {"tdot": r2a2 * PD - t2, "phidot": a * PD + p2, "tdot_two": (r2a2 * P) * inv_rd - t2, "phidot_two": (a * P) * inv_rd + p2,
               "thetadot": np.sqrt(np.maximum(np.abs(N), tiny)) * inv_rho * sg_th, "rdot": np.sqrt(np.maximum(np.abs(R), tiny)) * inv_rho * sg_r,
               "N": N, "R": R, "c2": c2}
        mag = {"tdot": np.abs(r2a2 * P_mag * inv_rd) + t2_mag, "phidot": np.abs(a * P_mag * inv_rd) + p2_mag, "N": N_mag, "R": R_mag,
               "inv_rho": np.abs(inv_rho), "delta": np.abs(delta)}
    return val, mag


def floors(val, mag):
    """What the number format alone allows per point, from the longdouble evaluation: FLOOR_EPS spacings of the summed terms for tdot and phidot; for the
    roots, the root's own FLOOR_EPS spacings plus what FLOOR_EPS spacings of N's (R's) terms move the root by -- |sqrt x - sqrt y| <= the difference of
    the roots of |x| +- that amount; R inherits 2 Delta times N's share through its last term."""
    f = FLOOR_EPS * EPS
    fN = f * mag["N"]
    fR = f * mag["R"] + 2 * mag["delta"] * fN

    def root(x, fx):
        x = np.abs(x)
        return (np.sqrt(x + fx) - np.sqrt(np.maximum(x - fx, 0))) * mag["inv_rho"]
    return {"tdot": f * mag["tdot"], "phidot": f * mag["phidot"],
            "thetadot": root(val["N"], fN) + f * np.abs(val["thetadot"]), "rdot": root(val["R"], fR) + f * np.abs(val["rdot"])}


def horizon(a):
    return 1.0 + np.sqrt(1.0 - a * a)


def points():
    """The chosen points as a structured array over COLUMNS, and masks by kind (tests/test_gpu_fast_stage_terms.py says what each is for)."""
    rows, kind = [], []
    rays = [(0.0, 5.0), (2.0, 0.0), (1.5, 10.0), (-3.0, 20.0), (0.0, 0.0)]          # (h, Q) with k = 1: h = 0, Q = 0, both; N < 0 wherever h^2 / s2 > Q + a^2
    code = 0

    def add(what, r, th0, d, h, Q, a):
        nonlocal code
        rows.append((r, th0, d, 1.0, h, Q, a, float(code & 3)))
        kind.append(what)
        code += 1
    rng = np.random.default_rng(20261021)
    for a in (0.0, 0.5, 0.998):
        radii = (horizon(a) + 1e-6, 3.0, 6.0, 50.0, 1000.0)
        # either pole: theta0 from 1e-8 to 0.3 from it; d = 0, the near limit (theta0 / 2 below 0.14, else 0.07), half and a thousandth of it, both ways
        for off in (1e-8, 1e-6, 1e-4, 1e-2, 0.1, 0.3):
            for th0 in (off, np.pi - off):
                lim = min(0.07, 0.5 * min(abs(th0), abs(np.pi - th0)))
                for d in (0.0, lim, -lim, 0.5 * lim, -0.5 * lim, 1e-3 * lim, -1e-3 * lim):
                    for r in radii:
                        for h, Q in rays:
                            add("pole", r, th0, d, h, Q, a)
        # the equator: stage angles ON pi / 2 (as exactly as theta0 + d can be) and 1e-12 ... 1e-3 either side, from base points up to 0.06 away
        for th0 in np.concatenate([np.pi / 2 + rng.uniform(-0.06, 0.06, 38), [np.pi / 2, np.nextafter(np.pi / 2, 0)]]):
            for eps in (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3):
                for r in radii[::2]:
                    h, Q = rays[code % len(rays)]
                    add("equator", r, th0, (np.pi / 2 - th0) + eps, h, Q, a)
    for r, th0 in ((np.nan, 1.0), (np.inf, 1.0), (-np.inf, 1.0), (6.0, np.nan), (6.0, np.inf), (np.nan, np.nan), (np.inf, np.pi / 2), (6.0, -np.inf)):
        add("nonfinite", r, th0, 0.01, 1.5, 10.0, 0.5)
    p = np.array(rows, dtype=[(n, np.float64) for n in COLUMNS])
    kind = np.array(kind)
    return p, {k: kind == k for k in ("pole", "equator", "nonfinite")}

