"""TEST INFRASTRUCTURE: the polarisation of disc emission seen on an image plane (include/kr_trace.h, kr_polarisation_dev_f64), restated in numpy
over ray records on top of tests/angle_rules.py (metric, tetrad, momentum), tests/reducer_rules.py (the image filter, the pixel rule, exact sums) and
tests/line_rules.py (the line's items).  Nothing here runs in the product path.

The frame is the one of angle_rules.frame.  The emitted polarisation vector f lies in the disc plane, perpendicular to the projection of the photon
direction; the Walker-Penrose constant kappa = (A - iB)(r - i a cos theta) carries it to the observer, where it is inverted with the ray's own
image-plane coordinates (x, y) = (alpha, beta)."""
import numpy as np

import angle_rules as ar
import line_rules as lr
import reducer_rules as rr

CHANDRASEKHAR = 0.1171          # the coefficient with which law 1 fits the pure-scattering atmosphere


def walker_penrose(p, f, r, theta, a):
    """(kappa1, kappa2) of a momentum p and a polarisation vector f (contravariant components, lists of four arrays) at (r, theta)."""
    s, c = np.sin(theta), np.cos(theta)
    A = (p[0] * f[1] - p[1] * f[0]) + a * s * s * (p[1] * f[3] - p[3] * f[1])
    B = ((r * r + a * a) * (p[3] * f[2] - p[2] * f[3]) - a * (p[0] * f[2] - p[2] * f[0])) * s
    return r * A - a * c * B, -1 * (r * B + a * c * A)


def observer_vector(kappa1, kappa2, x, y, a, sin_i):
    """(f_al, f_be): the polarisation vector at the observer on the axes of the impact parameters (al, be) = (-x, -y)."""
    al, be = -1 * x, -1 * y
    nu = -1 * (al + a * sin_i)
    d = nu * nu + be * be
    return (be * kappa2 - nu * kappa1) / d, (be * kappa1 + nu * kappa2) / d


def disc_state(rays, spin, V=-1.0, reverse=1, projradius=0):
    """What the rule needs at the records: the metric g and its a, the tetrad legs, the momentum p (spatial part negated with reverse) and the frame
    components of angle_rules.frame (not masked by steps)."""
    r, theta = rays["r"].astype(np.float64), rays["theta"].astype(np.float64)
    a = -spin if reverse else spin
    g, c = ar.metric(r, theta, a)
    if V == -1:
        rs = r * np.sin(theta)
        Vv = 1 / (a + rs * np.sqrt(rs)) if projradius else 1 / (a + r * np.sqrt(r))
    else:
        Vv = np.full_like(r, V)
    et, e1, e2, e3 = ar.tetrad(c, Vv)
    p = ar.momentum_from_consts(rays["k"], rays["h"], rays["Q"], rays["rdot_sign"], rays["thetadot_sign"], r, theta, spin)
    if reverse:
        p = [p[0], -1 * p[1], -1 * p[2], -1 * p[3]]
    E, P_phi, P_th, P_r = ar.dot_product(g, et, p), -1 * ar.dot_product(g, e1, p), -1 * ar.dot_product(g, e2, p), -1 * ar.dot_product(g, e3, p)
    return dict(r=r, theta=theta, a=a, g=g, et=et, e1=e1, e2=e2, e3=e3, p=p, E=E, P_phi=P_phi, P_th=P_th, P_r=P_r)


def emitted_vector(s):
    """f = (P_phi e3 - P_r e1) / nrm in coordinates, and nrm."""
    nrm = np.sqrt(s["P_r"] * s["P_r"] + s["P_phi"] * s["P_phi"])
    zero = np.zeros_like(nrm)
    return [-1 * s["P_r"] * s["e1"][0] / nrm, s["P_phi"] * s["e3"][1] / nrm, zero, -1 * s["P_r"] * s["e1"][3] / nrm], nrm


def polarisation(rays, spin, inc_deg, V=-1.0, reverse=1, projradius=0):
    """kr_polarisation_dev_f64 in numpy: {"kappa1", "kappa2", "c2", "s2"} (NaN where steps <= 0), "mu", "E", "nrm", "live" and "bad" (the bad-pol
    records among the live ones)."""
    live = rays["steps"] > 0
    sin_i = np.sin(inc_deg * np.pi / 180)
    with np.errstate(all="ignore"):
        s = disc_state(rays, spin, V, reverse, projradius)
        f, nrm = emitted_vector(s)
        k1, k2 = walker_penrose(s["p"], f, s["r"], s["theta"], s["a"])
        f_al, f_be = observer_vector(k1, k2, rays["alpha"], rays["beta"], s["a"], sin_i)
        n2 = f_al * f_al + f_be * f_be
        c2, s2 = (f_al * f_al - f_be * f_be) / n2, 2 * f_al * f_be / n2
        mu = np.abs(s["P_th"]) / s["E"]
        bad_angle = ~np.isfinite(mu) | (mu > 1) | ~(s["E"] > 0)
        bad = live & (bad_angle | (nrm == 0) | ~np.isfinite(k1) | ~np.isfinite(k2) | ~np.isfinite(c2) | ~np.isfinite(s2))
    out = {k: np.where(live, v, np.nan) for k, v in (("kappa1", k1), ("kappa2", k2), ("c2", c2), ("s2", s2), ("mu", mu), ("E", s["E"]), ("nrm", nrm))}
    out.update(live=live, bad=bad, f_al=f_al, f_be=f_be)
    return out


def degree(law, coeff, mu):
    """kr_pol_law: 0 -> coeff; 1 -> coeff (1 - mu) / (1 + 3.582 mu)."""
    mu = np.asarray(mu, dtype=np.float64)
    if law == 1:
        return coeff * (1 - mu) / (1 + 3.582 * mu)
    return np.full_like(mu, coeff)


def _with_redshift(rays, pol, reverse, g):
    rec = rays.copy()
    with np.errstate(all="ignore"):
        rec["redshift"] = (pol["E"] / rays["emit"] if reverse else rays["emit"] / pol["E"]) if g is None else g
    return rec


def stokes_image_rule(b, limb, pol_law, rays, spin, inc_deg, V=-1.0, reverse=1, projradius=0, g=None):
    """kr_post_image_stokes_dev_f64 in numpy over records before the redshift pass.  limb, pol_law: (law, coeff).  g: the redshift to filter and
    weigh with (default: the rule's own).  Returns nrays (int64), I, Q, U (npix each, exact sums), disc_count, bad_pol and "abs"."""
    npix = b.img_nx * b.img_ny
    pol = polarisation(rays, spin, inc_deg, V, reverse, projradius)
    rec = _with_redshift(rays, pol, reverse, g)
    ok, _, _, px = rr.image_pixel(b, rec["alpha"], rec["beta"])
    hit = rr.image_filter(b, rec) & ok
    keep = hit & ~pol["bad"]
    px, mu, gk, r = px[keep], pol["mu"][keep], rec["redshift"][keep], rec["r"][keep]
    with np.errstate(all="ignore"):
        w = rr.powerlaw3(r, b.q1, b.rb1, b.q2, b.rb2, b.q3) * ar.limb_weight(limb[0], limb[1], mu) / gk ** 3.0
        d = degree(pol_law[0], pol_law[1], mu)
        terms = {"I": w, "Q": w * d * pol["c2"][keep], "U": w * d * pol["s2"][keep]}
    out = {"nrays": np.bincount(px, minlength=npix).astype(np.int64), "disc_count": int(hit.sum()), "bad_pol": int((hit & pol["bad"]).sum()), "abs": {}}
    for k in ("I", "Q", "U"):
        out[k], out["abs"][k] = rr.bin_sums(px, terms[k], npix)
    return out


def stokes_image_from_words(nx, ny, words):
    """The 4 npix + 2 doubles of kr_post_image_stokes_dev_f64 as the dict of stokes_image_rule."""
    words, npix = np.asarray(words, dtype=np.float64), nx * ny
    return {"nrays": np.rint(words[:npix]).astype(np.int64), "I": words[npix:2 * npix], "Q": words[2 * npix:3 * npix], "U": words[3 * npix:4 * npix],
            "disc_count": int(round(words[4 * npix])), "bad_pol": int(round(words[4 * npix + 1]))}


def line_cells(b, E, tau, ok):
    """(binned, cell) of the line's items: the index rules of line_rules.bin_items."""
    with np.errstate(all="ignore"):
        fe = np.log(E / b.e_min) / np.log(b.de) if b.log_e else (E - b.e_min) / b.de
        keep = ok & (fe >= 0) & (fe < b.ne)
        j = np.zeros(E.shape, dtype=np.int64)
        if lr.has_time_axis(b):
            ft = tau / b.dt
            keep &= (ft >= 0) & (ft < b.nt)
            j = np.where(keep, ft, 0).astype(np.int64)
        i = np.where(keep, fe, 0).astype(np.int64)
    return keep, j * b.ne + i


def stokes_line_rule(b, limb, pol_law, rays, spin, inc_deg, V=-1.0, reverse=1, projradius=0, g=None):
    """kr_post_line_stokes_dev_f64 in numpy over records before the redshift pass: count (int64), I, Q, U of shape (nt, ne), on_disc, binned,
    bad_pol and "abs".  Bad-pol rays are never binned."""
    nb = b.nt * b.ne
    pol = polarisation(rays, spin, inc_deg, V, reverse, projradius)
    rec = _with_redshift(rays, pol, reverse, g)
    m = lr.disc_filter(b, rec)
    keep = m & ~pol["bad"]
    E, w, tau, ok = lr.items(b, rec["r"][keep], rec["redshift"][keep], rec["t"][keep])
    mu = pol["mu"][keep]
    binned, cell = line_cells(b, E, tau, ok)
    with np.errstate(all="ignore"):
        w = (w * ar.limb_weight(limb[0], limb[1], mu))[binned]
        d = degree(pol_law[0], pol_law[1], mu[binned])
        terms = {"I": w, "Q": w * d * pol["c2"][keep][binned], "U": w * d * pol["s2"][keep][binned]}
    cell = cell[binned]
    out = {"count": np.bincount(cell, minlength=nb).astype(np.int64).reshape(b.nt, b.ne), "on_disc": int(m.sum()), "binned": int(binned.sum()),
           "bad_pol": int((m & pol["bad"]).sum()), "abs": {}}
    for k in ("I", "Q", "U"):
        total, total_abs = rr.bin_sums(cell, terms[k], nb)
        out[k], out["abs"][k] = total.reshape(b.nt, b.ne), total_abs.reshape(b.nt, b.ne)
    return out


def stokes_line_from_words(b, words):
    """The 4 nt ne + 3 doubles of kr_post_line_stokes_dev_f64 as the dict of stokes_line_rule."""
    words, nb, shape = np.asarray(words, dtype=np.float64), b.nt * b.ne, (b.nt, b.ne)
    out = {k: words[q * nb:(q + 1) * nb].reshape(shape) for q, k in enumerate(("count", "I", "Q", "U"))}
    out["count"] = np.rint(out["count"]).astype(np.int64)
    out.update(on_disc=int(round(words[4 * nb])), binned=int(round(words[4 * nb + 1])), bad_pol=int(round(words[4 * nb + 2])))
    return out


def check_stokes(got, want, count_key, tallies, rtol, label=""):
    """Counts and tallies exact, I / Q / U within rtol of the per-cell sum of absolute terms (reducer_rules.sum_errors).  Returns the worst error."""
    np.testing.assert_array_equal(np.asarray(got[count_key]), want[count_key], err_msg=str(label))
    for k in tallies:
        assert got[k] == want[k], (label, k, got[k], want[k])
    flat = lambda d: {k: np.asarray(v).ravel() for k, v in d.items() if k in ("I", "Q", "U")}          # noqa: E731
    worst, problems = rr.sum_errors(flat(got), {**flat(want), "abs": flat(want["abs"])}, ("I", "Q", "U"))
    assert problems == [] and worst <= rtol, (label, worst, problems)
    return worst
