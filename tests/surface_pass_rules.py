"""TEST INFRASTRUCTURE: the per-record rule of the passes over rays that LANDED ON THE SURFACE of a disc (include/kr_trace.h, kr_disc_surface:
kr_angles_surface_dev_f64, kr_post_line_surface_dev_f64, kr_post_spectrum_surface_dev_f64, kr_post_response_surface_dev_f64 and their reduce forms)
restated in numpy.  This file is the arbiter of the rule.  Nothing here runs in the product path.

The observer is the one of kr_post_image_surface_dev_f64: V = -1, projradius = 1, motion = 0 -- the Keplerian gas at the cylindrical radius
rho = r sin(theta) -- in the metric of a = reverse ? -spin : spin; the frame is tests/angle_rules.py's.  The angle is taken to the normal of
|z| = H(rho), H = slope rho + scale (1 - sqrt(r_in / rho)), one IEEE operation per line in the association of the header.  Every function takes a dtype,
so that the same rule runs in np.longdouble: the difference between the two is the rounding noise of the rule on those records (the convention of
tests/plunge_rules.py).

The line, the spectrum and the response are the FLAT rules (tests/line_rules.py, spectrum_rules.py, response_rules.py) fed rho, g and the limb weight of
this rule: flat_equivalent() turns surface records into records that the flat filter sees exactly as the surface filter sees the originals."""
import numpy as np

import angle_rules as ar
import line_rules as lr
import reducer_rules as rr
from raytrace_cpu_amd import capi


def surface_of(surface):
    """(r_in, r_out, slope, scale) of a 4-tuple or a capi.DiscSurface."""
    if isinstance(surface, capi.DiscSurface):
        return surface.r_in, surface.r_out, surface.slope, surface.scale
    r_in, r_out, slope, scale = surface
    return float(r_in), float(r_out), float(slope), float(scale)


def frame(rays, spin, reverse, dtype=np.float64):
    """angle_rules.frame(rays, spin, V = -1, reverse, projradius = 1) in `dtype`, plus what the normal needs of the same evaluation: sn, cs, delta, rhosq
    (and the metric g, the gas four-velocity et and the momentum p, for the identities)."""
    live = rays["steps"] > 0
    r, theta = rays["r"].astype(dtype), rays["theta"].astype(dtype)
    a = dtype(-spin if reverse else spin)
    with np.errstate(all="ignore"):
        g, c = ar.metric(r, theta, a)
        sn, cs = np.sin(theta), np.cos(theta)
        rs = r * sn
        V = 1 / (a + rs * np.sqrt(rs))
        et, e1, e2, e3 = ar.tetrad(c, V)
        p = ar.momentum_from_consts(rays["k"].astype(dtype), rays["h"].astype(dtype), rays["Q"].astype(dtype), rays["rdot_sign"], rays["thetadot_sign"], r, theta, dtype(spin))
        if reverse:
            p = [p[0], -1 * p[1], -1 * p[2], -1 * p[3]]
        out = {"E": ar.dot_product(g, et, p), "P_phi": -1 * ar.dot_product(g, e1, p), "P_th": -1 * ar.dot_product(g, e2, p), "P_r": -1 * ar.dot_product(g, e3, p)}
    for k in out:
        out[k] = np.where(live, out[k], np.nan)
    out.update(live=live, sn=sn, cs=cs, delta=c["delta"], rhosq=c["rhosq"], metric=g, et=et, e2=e2, e3=e3, p=p)
    return out


def angles(rays, spin, reverse, surface, dtype=np.float64, f=None):
    """The rule: {"mu", "chi", "nn", "P_n", "P_s", "n_r", "n_th", "rho", "z", "sg", "Hp"} per record (NaN in mu and chi where steps <= 0), one IEEE
    operation per line."""
    r_in, _, slope, scale = (dtype(x) for x in surface_of(surface))
    f = frame(rays, spin, reverse, dtype) if f is None else f
    r = rays["r"].astype(dtype)
    sn, cs = f["sn"], f["cs"]
    with np.errstate(all="ignore"):
        rho = r * sn
        z = r * cs
        sg = np.where(z < 0, dtype(-1), dtype(1))
        Hp = slope + (scale * dtype(0.5) * np.sqrt(r_in / rho)) / rho
        f_r = sg * cs - Hp * sn
        f_th = -1 * (sg * (r * sn)) - Hp * (r * cs)
        n_r = np.sqrt(f["delta"] / f["rhosq"]) * f_r
        n_th = f_th / np.sqrt(f["rhosq"])
        nn = np.sqrt(n_r * n_r + n_th * n_th)
        P_n = (n_r * f["P_r"] + n_th * f["P_th"]) / nn
        mu = np.abs(P_n) / f["E"]
        P_s = sg * (n_r * f["P_th"] - n_th * f["P_r"]) / nn
        chi = np.arctan2(f["P_phi"], P_s)
    live = f["live"]
    return {"mu": np.where(live, mu, np.nan), "chi": np.where(live, chi, np.nan), "nn": nn, "P_n": P_n, "P_s": P_s, "n_r": n_r, "n_th": n_th, "rho": rho, "z": z,
            "sg": sg, "Hp": Hp}


def bad_angle(f, an):
    """frame_bad_angle(f, mu), or nn not finite, or nn zero (records with steps <= 0 are not judged: False)."""
    mu, nn = an["mu"], an["nn"]
    with np.errstate(invalid="ignore"):
        return f["live"] & (~np.isfinite(mu) | (mu > 1) | ~(f["E"] > 0) | ~np.isfinite(nn) | (nn == 0))


def redshift_of(rays, f, reverse):
    with np.errstate(all="ignore"):
        return f["E"] / rays["emit"].astype(f["E"].dtype) if reverse else rays["emit"].astype(f["E"].dtype) / f["E"]


def records_after(rays, spin, reverse, lo=-np.pi, hi=np.pi):
    """The records as a fused surface pass (or kr_post_image_surface_dev_f64) leaves them: redshift and wrapped phi."""
    rec = np.array(rays, copy=True)
    rec["redshift"] = redshift_of(rays, frame(rays, spin, reverse), reverse)
    rec["phi"] = rr.range_phi(rays["phi"], rays["steps"], lo, hi)
    return rec


def rho_of(rays):
    with np.errstate(invalid="ignore"):
        return rays["r"] * np.sin(rays["theta"])


def dest(rays):
    return (rays["steps"] > 0) & ((rays["status"] & capi.STATUS_DEST) != 0)


def on_surface(rays, r_isco, r_disc):
    """image_surface_kernel's filter on records that carry their redshift: steps > 0, DEST, g > 0, r_isco <= rho < r_disc."""
    rho = rho_of(rays)
    with np.errstate(invalid="ignore"):
        return dest(rays) & (rays["redshift"] > 0) & (rho >= r_isco) & (rho < r_disc)


def flat_equivalent(rec):
    """Records (carrying their redshift) as the FLAT rules must see them to apply the surface rule: r = rho, theta = pi / 2 (so r cos(theta) < 1e-2
    holds for every rho below 1e14) and a redshift of 0 -- which fails g > 0 -- where the record did not land on a destination."""
    out = np.array(rec, copy=True)
    out["r"] = rho_of(rec)
    out["theta"] = np.pi / 2
    out["redshift"] = np.where(dest(rec), rec["redshift"], 0.0)
    return out


def line_rule(b, law, coeff, rec, mu=None, bad=None):
    """kr_post_line_surface_dev_f64 (mu, bad given) / kr_reduce_line_surface_dev_f64 (None: isotropic, bad_angle 0) in numpy over records that carry their
    redshift: the dict of line_rules.bin_items plus "bad_angle"."""
    flat = flat_equivalent(rec)
    m = lr.disc_filter(b, flat)
    bad = np.zeros(len(rec), dtype=bool) if bad is None else np.asarray(bad) & m
    keep = m if law == 0 else m & ~bad
    E, w, tau, ok = lr.items(b, flat["r"][keep], flat["redshift"][keep], flat["t"][keep])
    if mu is not None:
        w = w * ar.limb_weight(law, coeff, mu[keep])
    out = lr.bin_items(b, E, w, tau, ok, m.sum())
    out["bad_angle"] = int(bad.sum())
    return out


def noise(rays, spin, reverse, surface):
    """{"g", "mu", "chi"}: |float64 rule - longdouble rule| per record (g: relative), 0 where either is not finite."""
    lo_f, hi_f = frame(rays, spin, reverse), frame(rays, spin, reverse, np.longdouble)
    lo, hi = angles(rays, spin, reverse, surface, f=lo_f), angles(rays, spin, reverse, surface, np.longdouble, f=hi_f)
    out = {}
    with np.errstate(all="ignore"):
        pairs = {"mu": (lo["mu"], hi["mu"]), "chi": (lo["chi"], hi["chi"]), "g": (redshift_of(rays, lo_f, reverse), redshift_of(rays, hi_f, reverse))}
        for k, (x, y) in pairs.items():
            d = np.abs(x.astype(np.longdouble) - y)
            if k == "g":
                d = d / np.abs(y)
            out[k] = np.where(np.isfinite(d), d, 0).astype(np.float64)
    return out
