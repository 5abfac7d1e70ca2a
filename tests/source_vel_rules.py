"""TEST INFRASTRUCTURE: the rules of the point source with any four-velocity and of the angular distribution of where its rays end
(include/kr_trace.h: kr_pointsource_vel_spec, kr_angdist_spec) restated in numpy.

  tetrad(pos, u, spin)        -> the emitter's frame: SolveTetrad (pointsource_vel.cpp:113-260), one numpy float64 operation per operation
  launched(spec)              -> per grid point the momentum (tdot, rdot, thetadot, phidot) the tetrad launches, with the live mask
  records(spec, emit=False)   -> the ray records kr_pointsource_vel_init(_emit)_dev_f64 builds (InitPointSourceVel, :34-110)
  angdist(sp, rays)           -> the buffer of kr_reduce_angdist_dev_f64 as the dict of api.angdist_from_words (disc_source_return_angdist.cpp:132-196)

Python evaluates `a * b * c / d` left to right like C, so the expressions below are written as the reference writes them.  sin / cos / tan of the
source's polar angle come from `math` (the C library, as in the library's host code).  acos, sin and cos of the per-ray angles are CORRECTLY ROUNDED
here -- mpmath at 200 bits, rounded once to nearest -- which is what the device routines of kr_crmath.hpp / kr_sincos.hpp deliver; numpy's own are
within an ulp but not always equal, and the records are compared bit for bit.
"""
import math

import mpmath
import numpy as np

import reducer_rules as rr
from raytrace_cpu_amd import capi

F = np.float64
PI = math.pi
EPS = 2.0 ** -52

_CACHE = {}


def _cr(name, x):
    """fn(x) elementwise, correctly rounded to double (NaN where the function has no real value)."""
    fn = getattr(mpmath, name)
    x = np.asarray(x, dtype=F)
    out = np.empty(x.shape, dtype=F)
    flat_in, flat_out = x.ravel(), out.ravel()
    for q, v in enumerate(flat_in.tolist()):
        key = (name, v)
        if key not in _CACHE:
            if not math.isfinite(v) or (name == "acos" and abs(v) > 1):
                _CACHE[key] = float("nan")
            else:
                with mpmath.workprec(200):
                    y = fn(mpmath.mpf(v))
                with mpmath.workprec(53):
                    _CACHE[key] = float(+y)                  # one rounding to nearest; the conversion of a 53-bit value is exact
        flat_out[q] = _CACHE[key]
    return out


def acos_cr(x):
    return _cr("acos", x)


def sin_cr(x):
    return _cr("sin", x)


def cos_cr(x):
    return _cr("cos", x)


def tetrad(pos, u, spin):
    """SolveTetrad: dict with "tetrad" [leg][t, r, theta, phi], "un" = u / sqrt(g(u, u)), "norm_u" = g(u, u), "g" (4 x 4) and sin / cos / tan of pos[2]."""
    r, theta, a = F(pos[1]), float(pos[2]), F(spin)
    st, ct, tt = F(math.sin(theta)), F(math.cos(theta)), F(math.tan(theta))
    rhosq = r * r + (a * ct) * (a * ct)
    delta = r * r - 2 * r + a * a
    sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st
    e2nu = rhosq * delta / sigmasq
    e2psi = sigmasq * st * st / rhosq
    omega = 2 * a * r / sigmasq
    g = np.zeros((4, 4))
    g[0][0] = e2nu - omega * omega * e2psi
    g[0][3] = omega * e2psi
    g[3][0] = g[0][3]
    g[1][1] = -rhosq / delta
    g[2][2] = -rhosq
    g[3][3] = -e2psi
    v = np.zeros((4, 4))
    v[0] = [F(x) for x in u]
    v[1][1] = v[2][2] = v[3][3] = 1
    e = np.zeros((4, 4))
    e[0] = v[0]
    for i in range(1, 4):
        e[i] = v[i]
        for j in range(i):
            dotprod, enorm = F(0), F(0)
            for p in range(4):
                for q in range(4):
                    dotprod = dotprod + g[p][q] * v[i][p] * e[j][q]
                    enorm = enorm + g[p][q] * e[j][p] * e[j][q]
            for p in range(4):
                e[i][p] = e[i][p] - (dotprod / enorm) * e[j][p]
    norm_u, un = None, None
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(4):
            enorm = F(0)
            for p in range(4):
                for q in range(4):
                    enorm = enorm + g[p][q] * e[i][p] * e[i][q]
            if i == 0:
                norm_u = enorm
                un = np.array([F(x) / np.sqrt(enorm) for x in u])
            for p in range(4):
                e[i][p] = e[i][p] / np.sqrt(np.abs(enorm))
    legs = np.zeros((4, 4))
    for i, leg in enumerate((0, 3, 1, 2)):
        legs[leg] = e[i]
    if legs[1][2] < 0:
        legs[1] = legs[1] * -1
    if legs[2][3] < 0:
        legs[2] = legs[2] * -1
    if legs[3][1] < 0:
        legs[3] = legs[3] * -1
    return {"tetrad": legs, "un": un, "norm_u": norm_u, "g": g, "sin": st, "cos": ct, "tan": tt, "rhosq": rhosq}


def dot(g, x, y):
    """(sum, sum of absolute terms) of g_ab x^a y^b over all sixteen (a, b), row-major; x, y: sequences of four scalars or arrays."""
    total, total_abs = 0.0, 0.0
    for p in range(4):
        for q in range(4):
            term = g[p][q] * x[p] * y[q]
            total, total_abs = total + term, total_abs + np.abs(term)
    return total, total_abs


def grid(spec):
    """(rays, n_cosalpha, n_beta): the int-truncated product of doubles and the truncated factors (pointsource_vel.cpp:12, :15-16)."""
    fc = ((F(spec.cosalphamax) - F(spec.cosalpha0)) / F(spec.dcosalpha)) + 1
    fb = ((F(spec.betamax) - F(spec.beta0)) / F(spec.dbeta)) + 1
    return int(fc * fb), int(fc), int(fb)


def launched(spec, frame=None):
    """Per slot of the source: cosalpha, beta, the live mask and (tdot, rdot, thetadot, phidot) as the tetrad launches the photon (0 where dead)."""
    n, nc, nb = grid(spec)
    frame = frame or tetrad(spec.pos, spec.u, spec.spin)
    ix = np.arange(n)
    in_grid = ix < nc * nb
    i, j = ix // max(nb, 1), ix % max(nb, 1)
    cosalpha = F(spec.cosalpha0) + i * F(spec.dcosalpha)
    beta = F(spec.beta0) + j * F(spec.dbeta)
    live = in_grid & ~((cosalpha >= spec.cosalphamax) | (beta >= spec.betamax))
    alpha = acos_cr(np.where(live, cosalpha, 0.0))
    sa, ca = sin_cr(alpha), cos_cr(alpha)
    b = np.where(live, beta, 0.0)
    sb, cb = sin_cr(b), cos_cr(b)
    E, T = F(spec.E), frame["tetrad"]
    rp = [E, E * sa * cb, E * sa * sb, E * ca]
    p = [rp[0] * T[0][c] + rp[1] * T[1][c] + rp[2] * T[2][c] + rp[3] * T[3][c] for c in range(4)]
    return {"cosalpha": cosalpha, "beta": beta, "live": live, "p": p, "frame": frame, "rp": rp}


def constants(spec, p, frame):
    """k, h, Q of pointsource_vel.cpp:94-100 from the launched momentum p = (tdot, rdot, thetadot, phidot)."""
    r, a = F(spec.pos[1]), F(spec.spin)
    st, ct, tt, rhosq = frame["sin"], frame["cos"], frame["tan"], frame["rhosq"]
    tdot, _, thetadot, phidot = p
    k = (1 - 2 * r / rhosq) * tdot + (2 * a * r * st * st / rhosq) * phidot
    h = phidot * ((r * r + a * a) * (r * r + a * a * ct * ct - 2 * r) * st * st + 2 * a * a * r * st * st * st * st)
    h = h - 2 * a * r * k * st * st
    h = h / (r * r + a * a * ct * ct - 2 * r)
    Q = rhosq * rhosq * thetadot * thetadot - (a * k * ct + h / tt) * (a * k * ct - h / tt)
    return k, h, Q


def records(spec, emit=False):
    """The records of kr_pointsource_vel_init_dev_f64 (emit = 0) or kr_pointsource_vel_init_emit_dev_f64."""
    L = launched(spec)
    live, p, frame = L["live"], L["p"], L["frame"]
    rays = np.zeros(len(live), dtype=capi.RAY_F64)
    rays["steps"] = np.where(live, 0, -1)
    k, h, Q = constants(spec, p, frame)
    for name, val in (("t", spec.pos[0]), ("r", spec.pos[1]), ("theta", spec.pos[2]), ("phi", spec.pos[3]), ("alpha", L["cosalpha"]), ("beta", L["beta"]), ("k", k),
                      ("h", h), ("Q", Q), ("rdot_sign", np.where(p[1] > 0, 1, -1)), ("thetadot_sign", np.where(p[2] > 0, 1, -1))):
        rays[name] = np.where(live, val, 0)
    if emit:
        rays["emit"] = np.where(live, dot(frame["g"], frame["un"], p)[0], 0)
    return rays


def nangle_of(sp):
    return int(2 * PI / sp.dangle)


def angdist(sp, rays, wrap=None):
    """kr_reduce_angdist_dev_f64 in numpy (wrap = (lo, hi): range_phi first, as the fused pass classifies).  Sums are exact per bin (reducer_rules.bin_sums);
    out["abs"] holds the per-bin sums of the absolute terms (equal to the sums: every weight is >= 0)."""
    b, n = sp.cls, nangle_of(sp)
    rec = rays[rays["steps"] > 0]
    out = {"bad_g": int((~(rec["redshift"] > 0)).sum())}
    c = rec["alpha"]
    out["skipped"] = int((c == 0).sum())
    rec = rec[c != 0]
    c, beta = rec["alpha"], rec["beta"]
    phi = rr.range_phi(rec["phi"], rec["steps"], *wrap) if wrap else rec["phi"]
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = acos_cr(c)
        sa, sb, cb = sin_cr(alpha), sin_cr(beta), cos_cr(beta)
        if sp.labels:
            sb, cb = -1 * cb, sb                                  # PointSourceVel's (alpha, beta) is PointSource's (alpha, beta - pi/2)
        s = sa * sb
        sasb = np.abs(s)
        norm = acos_cr(sasb)
        az = acos_cr(-c / np.sqrt(1 - s * s))
        az = np.where(sa * cb < 0, az * -1, az)
        idx = {}
        ok = np.ones(len(rec), dtype=bool)
        for name, x in (("alpha", alpha), ("beta", beta), ("norm", norm), ("az", az)):
            good, idx[name] = rr.bin_index((x + PI) / sp.dangle, n)
            ok &= good
        out["out_of_range"] = int((~ok).sum())
        w = sasb if b.plane_iso else np.ones(len(rec))
        if b.limb:
            w = w * (1 + 2.06 * sasb)
        r = rec["r"]
        disc = (rec["theta"] >= PI / 2) & (r >= b.r_isco) & (r < b.r_disc)
        away = (np.abs(r - b.source_r) > 0.1 * b.source_r) | (np.abs(phi - b.source_phi) > 0.1)
        escape = ~disc & (r > b.r_esc)
        lost = ~disc & ~escape & (r < b.r_isco)
    member = {"escape": ok & escape, "return": ok & disc & away, "lost": ok & lost}
    out["other"] = int((ok & ~member["escape"] & ~member["return"] & ~member["lost"]).sum())

    def total(x):
        return rr.bin_sums(np.zeros(len(x), dtype=np.int64), x, 1)[0][0] if len(x) else 0.0
    out["ray_count"] = total(w[ok]) if b.weight_norm else float(ok.sum())
    out["abs"] = {}
    for cls, m in member.items():
        out[cls + "_sum"] = total(w[m])
        out[cls + "_count"] = int(m.sum())
        for name in ("alpha", "beta", "norm", "az"):
            key = f"{cls}_{name}"
            out[key], out["abs"][key] = rr.bin_sums(idx[name][m], w[m], n)
            out[key + "_n"] = np.bincount(idx[name][m], minlength=n)
    out["total_norm"] = np.bincount(idx["norm"][ok], minlength=n).astype(F)
    out["total_az"] = np.bincount(idx["az"][ok], minlength=n).astype(F)
    return out


HIST_KEYS = tuple(f"{c}_{a}" for c in ("escape", "return", "lost") for a in ("alpha", "beta", "norm", "az"))


def check_angdist(got, want, rtol, label=""):
    """The bar of the angular-distribution tests: tallies and unweighted totals exact, a histogram bin non-zero exactly where the rule has rays in it,
    every weighted sum within rtol of the per-bin sum of absolute terms.  Returns the worst relative sum error."""
    for k in ("other", "skipped", "out_of_range", "bad_g"):
        assert got[k] == want[k], (label, k, got[k], want[k])
    for k in ("total_norm", "total_az"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{label} {k}")
    worst, problems = rr.sum_errors(got, want, HIST_KEYS)
    assert problems == [] and worst <= rtol, (label, worst, problems)
    for k in HIST_KEYS:
        w, g = np.asarray(want[k]), np.asarray(got[k])
        assert np.array_equal(g != 0, w != 0) or not np.isfinite(w).all(), (label, k)
    for k in ("ray_count", "escape_sum", "return_sum", "lost_sum"):
        g, w = float(got[k]), float(want[k])
        if math.isnan(w):
            assert math.isnan(g), (label, k)
            continue
        rel = 0.0 if g == w else abs(g - w) / abs(w)
        assert rel <= rtol, (label, k, g, w)
        worst = max(worst, rel)
    return worst


# ---- the four emitters of the tests, a = 0.998, and the small grid ---------------------------------------------------------------------------
SPIN = 0.998
EMITTERS = ("lamp-post", "outflow", "blob", "plunge")


def emitter(name):
    """(pos, u): the lamp-post at rest in the orbital sense (omega = 0), the same flowing out at dr/dt = 0.3, an orbiting and outflowing blob, and a
    plunging one inside the ISCO.  u comes un-normalised on purpose where the coordinate velocities are simple numbers."""
    from raytrace_cpu_amd import api
    if name == "lamp-post":
        return (0.0, 5.0, 1e-3, 1.5707), (1.0, 0.0, 0.0, 0.0)
    if name == "outflow":
        return (0.0, 5.0, 1e-3, 1.5707), (1.0, 0.3, 0.0, 0.0)
    if name == "blob":
        pos = (0.0, 6.0, 1.2, 0.3)
        return pos, api.four_velocity(pos, SPIN, omega=0.06, dr_dt=0.15, dtheta_dt=-0.01)
    pos = (0.0, 1.15, PI / 2 - 0.05, 1.0)
    return pos, (2.0, -2.0 * 0.004, 0.0, 2.0 * 0.45)


def spec_of(name, dcosalpha=0.06, dbeta=0.18, E=1.0, **kw):
    from raytrace_cpu_amd import api
    pos, u = emitter(name)
    return api.pointsource_vel_spec(pos, u, SPIN, dcosalpha, dbeta, E=E, **kw)


# ---- the two measured tolerances (python tests/source_vel_rules.py prints them; profiles/source_vel_ab.txt keeps them) -------------------------
def null_residuals(spec):
    """How far the records are from null vectors, over the live rays: rdot^2 and thetadot^2 rebuilt from (k, h, Q) by angle_rules.momentum_from_consts
    against the tetrad-launched ones, and g(p, p) of the launched momentum, each relative to N = the sum of the absolute terms of g(p, p) (the two
    squares weighted by |g_rr|, |g_thth|).  Near a turning point rdot^2 is the small difference of terms of size N, hence the scale."""
    import angle_rules as ar
    L = launched(spec)
    live, frame = L["live"], L["frame"]
    p = [x[live] for x in L["p"]]
    k, h, Q = constants(spec, p, frame)
    g = frame["g"]
    gpp, N = dot(g, p, p)
    mom = ar.momentum_from_consts(k, h, Q, np.where(p[1] > 0, 1, -1), np.where(p[2] > 0, 1, -1), F(spec.pos[1]), F(spec.pos[2]), F(spec.spin))
    return {"rdot_sq": float((np.abs(g[1][1]) * np.abs(mom[1] * mom[1] - p[1] * p[1]) / N).max()),
            "thetadot_sq": float((np.abs(g[2][2]) * np.abs(mom[2] * mom[2] - p[2] * p[2]) / N).max()),
            "tdot": float((np.abs(g[0][0]) * np.abs(mom[0] * mom[0] - p[0] * p[0]) / N).max()),
            "null": float((np.abs(gpp) / N).max())}


def orbital_spec(pos, V, spin, dcosalpha, dbeta, beta0, betamax):
    """The PointSourceVel spec of an emitter on a circular orbit, u = u^t (1, 0, 0, V) with u^t left at 1, on a beta grid from beta0."""
    from raytrace_cpu_amd import api
    return api.pointsource_vel_spec(pos, (1.0, 0.0, 0.0, V), spin, dcosalpha, dbeta, cosalpha0=-0.995, cosalphamax=0.995, beta0=beta0, betamax=betamax)


def orbital_difference(pos, V, spin, dcosalpha=0.06, dbeta=0.18):
    """PointSourceVel against the host PointSource constructor (the oracle's, pinned to the compiled reference) for u = u^t (1, 0, 0, V).
    calculate_constants (raytracer.cpp:625-676) puts p'1 = sin(alpha) cos(beta) on its leg along +phi and p'2 = sin(alpha) sin(beta) on e2 = -1 / sqrt(rhosq)
    d_theta; SolveTetrad's leg 1 is +theta and leg 2 +phi.  Equating the components, sin(beta_ps) = -cos(beta_vel) and cos(beta_ps) = sin(beta_vel):
    PointSourceVel(alpha, beta) is PointSource(alpha, beta - pi/2), so the PointSource grid starts a quarter turn earlier.  Returns the worst
    |difference| of k, h (relative to the largest |k|, |h| of the source) and Q (relative to the largest |Q|), and whether the signs agree where the
    launched component is not a rounding residue."""
    import oracle_lib as ol
    b0 = -3.0
    vel = orbital_spec(pos, V, spin, dcosalpha, dbeta, b0, b0 + 6.2)
    ps = ol.pointsource_spec(list(pos), V, spin, dcosalpha, dbeta, cosalpha0=-0.995, cosalphamax=0.995, beta0=b0 - PI / 2, betamax=b0 + 6.2 - PI / 2)
    want, got = ol.oracle_pointsource(ps), records(vel)
    assert len(want) == len(got) and np.array_equal(want["steps"] != -1, got["steps"] != -1)
    live = got["steps"] != -1
    want, got = want[live], got[live]
    out = {"rays": int(live.sum())}
    for f in ("k", "h", "Q"):
        out[f] = float(np.abs(got[f] - want[f]).max() / np.abs(want[f]).max())
    moving = np.abs(np.sin(np.arccos(got["alpha"])) * np.cos(got["beta"])) > 1e-9
    out["signs"] = bool(np.array_equal(got["rdot_sign"], want["rdot_sign"]) and np.array_equal(got["thetadot_sign"][moving], want["thetadot_sign"][moving]))
    return out


def radial_difference(rays=None):
    """The radial emitter ("outflow": u = (1, 0.3, 0, 0)) against the HEALPix source's motion = 1 constants (healpix_rules.constants, the rule of
    calc_consts_from_vector) for matching directions: that tetrad has its leg 1 along phi, leg 2 along +theta and leg 3 along r, SolveTetrad's has
    leg 1 along +theta and leg 2 along +phi, so the HEALPix vector of the ray (alpha, beta) is (sin(alpha) sin(beta), sin(alpha) cos(beta), cos(alpha)).
    rays: the records to judge (default: this module's).  Returns the worst |difference| of k, h, Q relative to the source's largest and whether
    the signs agree."""
    import healpix_rules as hr
    spec = spec_of("outflow")
    L = launched(spec)
    live = L["live"]
    rec = (records(spec) if rays is None else rays)[live]
    vec = np.stack([L["rp"][2], L["rp"][1], L["rp"][3]], axis=1)[live]
    k, h, Q, rs, ts, _ = hr.constants(vec, spec.pos, spec.u[1] / spec.u[0], spec.spin, spec.E, motion=1)
    out = {f: float(np.abs(x - rec[f]).max() / np.abs(x).max()) for f, x in (("k", k), ("h", h), ("Q", Q))}
    out["signs"] = bool(np.array_equal(rs, rec["rdot_sign"]) and np.array_equal(ts, rec["thetadot_sign"]))
    return out


ORBITS = (((0.0, 5.0, 1e-3, 1.5707), 0.0, 0.998), ((0.0, 6.0, 1.2, 0.3), 0.06, 0.998), ((0.0, 3.0, PI / 2 - 1e-6, 1.5707), 1 / (0.998 + 3.0 ** 1.5), 0.998))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    for name in EMITTERS:
        print("null residuals", name, null_residuals(spec_of(name)))
    for pos, V, spin in ORBITS:
        print("orbital difference", pos, V, orbital_difference(pos, V, spin))
    print("radial difference", radial_difference())
