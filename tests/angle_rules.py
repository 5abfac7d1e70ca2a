"""TEST INFRASTRUCTURE: the photon's angles in the rest frame of the orbiting disc gas (include/kr_trace.h, kr_angles_dev_f64), restated in numpy
over ray records in the manner of tests/line_rules.py and tests/reducer_rules.py, on which the two histogram rules build.  Nothing here runs in the
product path.

The observer is the one of redshift(V, reverse, projradius, motion = 0): metric with a = reverse ? -spin : spin, momentum from the constants of motion
with `spin` (host/include/kerr.h momentum_from_consts), spatial part negated with reverse, V == -1 Keplerian at the record's r.  The frame is the
reference's Tetrad (kerr.h:127-170) and every component its DotProduct: all 16 terms, row-major, zeros included."""
import numpy as np

import line_rules as lr
import reducer_rules as rr


def metric(r, theta, a):
    """g[i][j] of kerr_metric (kerr.h:94-124) and the coefficients the tetrad needs."""
    st, ct = np.sin(theta), np.cos(theta)
    rhosq = r * r + (a * ct) * (a * ct)
    delta = r * r - 2 * r + a * a
    sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st
    e2nu = rhosq * delta / sigmasq
    e2psi = sigmasq * st * st / rhosq
    omega = 2 * a * r / sigmasq
    zero = np.zeros_like(r)
    g03 = omega * e2psi
    g = [[e2nu - omega * omega * e2psi, zero, zero, g03], [zero, -rhosq / delta, zero, zero], [zero, zero, -rhosq, zero], [g03, zero, zero, -e2psi]]
    return g, dict(rhosq=rhosq, delta=delta, e2nu=e2nu, e2psi=e2psi, omega=omega)


def momentum_from_consts(k, h, Q, rdot_sign, thetadot_sign, r, theta, a):
    """(tdot, rdot, thetadot, phidot): kerr.h:300-335."""
    s, c = np.sin(theta), np.cos(theta)
    s2 = s * s
    rhosq = r * r + (a * c) * (a * c)
    delta = r * r - 2 * r + a * a
    rhosq_delta = rhosq * delta
    pt = ((rhosq * (r * r + a * a) + 2 * a * a * r * s2) * k - 2 * a * r * h) / rhosq_delta
    pphi = (2 * a * r * s2 * k + (rhosq - 2 * r) * h) / (s2 * rhosq_delta)
    thetadotsq = (Q + (k * a * c + h * c / s) * (k * a * c - h * c / s)) / (rhosq * rhosq)
    ptheta = np.sqrt(np.abs(thetadotsq)) * thetadot_sign
    rdotsq = (k * pt - h * pphi - rhosq * ptheta * ptheta) * delta / rhosq
    pr = np.sqrt(np.abs(rdotsq)) * rdot_sign
    return [pt, pr, ptheta, pphi]


def dot_product(g, u, v):
    total = np.zeros_like(v[0])
    for i in range(4):
        for j in range(4):
            total = total + g[i][j] * u[i] * v[j]
    return total


def tetrad(c, V):
    """(et, e1, e2, e3) of kerr.h:127-170 from the coefficients of metric()."""
    e2nu, e2psi, omega = c["e2nu"], c["e2psi"], c["omega"]
    zero = np.zeros_like(e2nu)
    et = [(1 / np.sqrt(e2nu)) / np.sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu), zero, zero,
          (1 / np.sqrt(e2nu)) * V / np.sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu)]
    e1 = [(V - omega) * np.sqrt(e2psi / e2nu) / np.sqrt(e2nu - (V - omega) * (V - omega) * e2psi), zero, zero,
          (1 / np.sqrt(e2nu * e2psi)) * (e2nu + V * omega * e2psi - omega * omega * e2psi) / np.sqrt(e2nu - (V - omega) * (V - omega) * e2psi)]
    e2 = [zero, zero, 1 / np.sqrt(c["rhosq"]), zero]
    e3 = [zero, np.sqrt(c["delta"] / c["rhosq"]), zero, zero]
    return et, e1, e2, e3


def frame(rays, spin, V=-1.0, reverse=0, projradius=0):
    """{"E", "P_r", "P_th", "P_phi", "live"} per record; NaN where steps <= 0."""
    live = rays["steps"] > 0
    r, theta = rays["r"].astype(np.float64), rays["theta"].astype(np.float64)
    a = -spin if reverse else spin
    with np.errstate(all="ignore"):
        g, c = metric(r, theta, a)
        if V == -1:
            rs = r * np.sin(theta)
            Vv = 1 / (a + rs * np.sqrt(rs)) if projradius else 1 / (a + r * np.sqrt(r))
        else:
            Vv = np.full_like(r, V)
        et, e1, e2, e3 = tetrad(c, Vv)
        p = momentum_from_consts(rays["k"], rays["h"], rays["Q"], rays["rdot_sign"], rays["thetadot_sign"], r, theta, spin)
        if reverse:
            p = [p[0], -1 * p[1], -1 * p[2], -1 * p[3]]
        out = {"E": dot_product(g, et, p), "P_phi": -1 * dot_product(g, e1, p), "P_th": -1 * dot_product(g, e2, p), "P_r": -1 * dot_product(g, e3, p)}
    for k in out:
        out[k] = np.where(live, out[k], np.nan)
    out["live"] = live
    return out


def mu_chi(f):
    with np.errstate(all="ignore"):
        return np.abs(f["P_th"]) / f["E"], np.arctan2(f["P_phi"], f["P_r"])


def bad_angle(f):
    """mu not finite, mu > 1 or E <= 0 (records with steps <= 0 are not judged: False)."""
    mu, _ = mu_chi(f)
    with np.errstate(invalid="ignore"):
        return f["live"] & (~np.isfinite(mu) | (mu > 1) | ~(f["E"] > 0))


def mu_closed_form(rays, f, spin):
    """sqrt(|Theta|) / (rho E), Theta = Q + cos^2(theta) (a^2 k^2 - h^2 / sin^2(theta)): independent of the tetrad's spatial legs."""
    with np.errstate(all="ignore"):
        s, c = np.sin(rays["theta"]), np.cos(rays["theta"])
        Theta = rays["Q"] + c * c * (spin * spin * rays["k"] * rays["k"] - rays["h"] * rays["h"] / (s * s))
        return np.sqrt(np.abs(Theta)) / (np.sqrt(rays["r"] * rays["r"] + spin * spin * c * c) * f["E"])


def redshift_of(rays, f, reverse):
    with np.errstate(all="ignore"):
        return f["E"] / rays["emit"] if reverse else rays["emit"] / f["E"]


def limb_weight(law, coeff, mu):
    mu = np.asarray(mu, dtype=np.float64)
    with np.errstate(all="ignore"):
        if law == 1:
            return 1 + coeff * mu
        if law == 2:
            return np.log(1 + 1 / mu)
    return np.ones_like(mu)


def line_limb_rule(b, law, coeff, rays, spin, V=-1.0, reverse=1, projradius=0, g=None):
    """kr_post_line_limb_dev_f64 in numpy over records before the redshift pass: the dict of line_rules.bin_items plus "bad_angle" and "binned_index"
    (the records that were binned).  g: the redshift to filter and weigh with (default: the rule's own)."""
    f = frame(rays, spin, V, reverse, projradius)
    rec = rays.copy()
    rec["redshift"] = redshift_of(rays, f, reverse) if g is None else g
    m = lr.disc_filter(b, rec)
    mu, _ = mu_chi(f)
    bad = bad_angle(f) & m
    keep = m if law == 0 else m & ~bad
    E, w, tau, ok = lr.items(b, rec["r"][keep], rec["redshift"][keep], rec["t"][keep])
    out = lr.bin_items(b, E, w * limb_weight(law, coeff, mu[keep]), tau, ok, m.sum())
    out["bad_angle"] = int(bad.sum())
    out["bad_index"] = np.flatnonzero(bad)
    return out


def emissivity_mu_rule(b, nmu, rays, spin, V=-1.0, reverse=0, projradius=0, g=None):
    """kr_post_emissivity_mu_dev_f64 in numpy over records before the redshift pass: (hist, mu) with hist = reducer_rules.reduce_emissivity and
    mu = {"count2", "flux2" (nr x nmu), "sum_mu", "disc_count", "binned", "bad_angle", "bad_per_bin", "abs": {"flux2", "sum_mu"}}."""
    f = frame(rays, spin, V, reverse, projradius)
    rec = rays.copy()
    rec["redshift"] = redshift_of(rays, f, reverse) if g is None else g
    hist = rr.reduce_emissivity(b, rec)
    m = rr.emissivity_filter(b, rec)
    ok, ir = rr.bin_index(rr.emissivity_quotient(b, rec["r"]), b.nr)
    binned = m & ok
    bad = bad_angle(f) & binned
    keep = binned & ~bad
    mu, _ = mu_chi(f)
    mu, ir_k, gk = mu[keep], ir[keep], rec["redshift"][keep]
    im = np.minimum((mu * nmu).astype(np.int64), nmu - 1)
    cell = ir_k * nmu + im
    out = {"count2": np.bincount(cell, minlength=b.nr * nmu).reshape(b.nr, nmu).astype(np.int64), "disc_count": int(m.sum()), "binned": int(binned.sum()),
           "bad_angle": int(bad.sum()), "bad_per_bin": np.bincount(ir[bad], minlength=b.nr).astype(np.int64), "abs": {}}
    flux2, flux2_abs = rr.bin_sums(cell, 1 / (b.num_primary_rays * gk ** 1.0), b.nr * nmu)
    out["flux2"], out["abs"]["flux2"] = flux2.reshape(b.nr, nmu), flux2_abs.reshape(b.nr, nmu)
    out["sum_mu"], out["abs"]["sum_mu"] = rr.bin_sums(ir_k, mu, b.nr)
    return hist, out


def mu_from_words(nr, nmu, words):
    """The (2 nmu + 1) nr + 3 doubles of kr_post_emissivity_mu_dev_f64 as the dict of emissivity_mu_rule."""
    words = np.asarray(words, dtype=np.float64)
    plane = nr * nmu
    return {"count2": words[:plane].reshape(nr, nmu).astype(np.int64), "flux2": words[plane:2 * plane].reshape(nr, nmu), "sum_mu": words[2 * plane:2 * plane + nr],
            "disc_count": int(words[-3]), "binned": int(words[-2]), "bad_angle": int(words[-1])}


def disc_filter(rays, r_isco, r_disc):
    """steps > 0, r cos(theta) < 1e-2, r_isco <= r < r_disc: the rays on the disc, whatever their redshift."""
    with np.errstate(invalid="ignore"):
        return (rays["steps"] > 0) & (rays["r"] * np.cos(rays["theta"]) < 1e-2) & (rays["r"] >= r_isco) & (rays["r"] < r_disc)
