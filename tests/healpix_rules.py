"""TEST INFRASTRUCTURE: the rules of the HEALPix point source (include/kr_trace.h: kr_healpix_source, kr_healpix_map) restated in numpy.

  pixel_vectors(order, pix)            -> [n, 15]: four corners then the centre (healpix.h: ring2xyf, xyf2loc, get_pixel_vectors, quirks kept)
  constants(vec, pos, V, a, E, ...)    -> k, h, Q, rdot_sign, thetadot_sign (healpix_pointsource.cpp:11-109 at unit energy, one numpy operation per
                                          operation, then scaled by E, E, E E)
  records(spec, vecs)                  -> the ray records the source builds from given vectors (emit = 0)
  classify(m, rays)                    -> class per record (the fate pass' rule on records as they are)

Python evaluates `a * b * c / d` left to right like C, so the expressions below are written as the reference writes them.  sin / cos / tan of
the source's polar angle come from `math` (the C library); the pixel azimuth's sin / cos are numpy's.
"""
import math

import numpy as np

from raytrace_cpu_amd import capi

F = np.float64
PI2 = 1.57079632679489661923

JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], dtype=np.int64)
JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7], dtype=np.int64)


def npix_of(order):
    return 12 * 4 ** order


def _isqrt(x):
    return np.sqrt(x.astype(F) + 0.5).astype(np.int64)


def ring2xyf(order, pix):
    """RING pixel -> (ix, iy, face); every value fits the reference's 32-bit int for order <= 13, so int64 computes the same."""
    pix = np.asarray(pix, dtype=np.int64)
    nside = 1 << order
    nl2 = 2 * nside
    npface = nside << order
    ncap = (npface - nside) << 1
    npix = 12 * npface
    north, south = pix < ncap, pix >= npix - ncap
    belt = ~north & ~south
    iring, iphi, kshift, nr, face = (np.zeros(pix.shape, dtype=np.int64) for _ in range(5))

    p = pix[north]
    ir = (1 + _isqrt(1 + 2 * p)) >> 1
    ip_ = (p + 1) - 2 * ir * (ir - 1)
    iring[north], iphi[north], nr[north] = ir, ip_, ir
    face[north] = (ip_ - 1) // np.maximum(ir, 1)

    ip = pix[belt] - ncap
    tmp = ip >> (order + 2)
    ir = tmp + nside
    ip_ = ip - tmp * 4 * nside + 1
    iring[belt], iphi[belt], nr[belt] = ir, ip_, nside
    kshift[belt] = (ir + nside) & 1
    ire = ir - nside + 1
    irm = nl2 + 2 - ire
    ifm = (ip_ - ire // 2 + nside - 1) >> order
    ifp = (ip_ - irm // 2 + nside - 1) >> order
    face[belt] = np.where(ifp == ifm, ifp | 4, np.where(ifp < ifm, ifp, ifm + 8))

    ip = npix - pix[south]
    ir = (1 + _isqrt(2 * ip - 1)) >> 1
    ip_ = 4 * ir + 1 - (ip - 2 * ir * (ir - 1))
    iphi[south], nr[south] = ip_, ir
    iring[south] = 2 * nl2 - ir
    face[south] = 8 + (ip_ - 1) // np.maximum(ir, 1)

    irt = iring - JRLL[face] * nside
    ipt = 2 * iphi - JPLL[face] * nr - kshift - 1
    ipt = np.where(ipt >= nl2, ipt - 8 * nside, ipt)
    return (ipt - irt) >> 1, (-ipt - irt) >> 1, face


def xyf2loc(x, y, face):
    jr = JRLL[face].astype(F) - x - y
    low, high = jr < 1, jr > 3
    nr = np.where(low, jr, np.where(high, 4 - jr, F(1)))
    z = np.where(low, 1 - nr * nr / 3., np.where(high, nr * nr / 3. - 1, (2 - jr) * 2. / 3.))
    tmp = JPLL[face].astype(F) * nr + x - y
    tmp = np.where(tmp < 0, tmp + 8, tmp)
    tmp = np.where(tmp >= 8, tmp - 8, tmp)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(nr < 1e-15, F(0), (0.25 * math.pi * tmp) / nr)
    sin_theta = np.sqrt((1.0 - z) * (1.0 + z))
    return np.stack([sin_theta * np.cos(phi + 0.05), sin_theta * np.sin(phi + 0.05), z], axis=-1)


def centre_of(corners, unit_center=False):
    """corners [n, 4, 3] -> [n, 3]: 0.25 * (((c0 + c1) + c2) + c3), not normalised unless unit_center."""
    c = 0.25 * (corners[:, 0] + corners[:, 1] + corners[:, 2] + corners[:, 3])
    if unit_center:
        ln = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
        c = c / ln[:, None]
    return c


def pixel_vectors(order, pix, unit_center=False):
    ix, iy, face = ring2xyf(order, pix)
    nside = 1 << order
    dc = F(0.5) / nside
    xc, yc = (ix + 0.5) / nside, (iy + 0.5) / nside
    corners = np.stack([xyf2loc(xc + dc, yc + dc, face), xyf2loc(xc - dc, yc + dc, face), xyf2loc(xc - dc, yc - dc, face), xyf2loc(xc + dc, yc - dc, face)],
                       axis=1)
    return np.concatenate([corners.reshape(-1, 12), centre_of(corners, unit_center)], axis=1)


def constants(vec, pos, V, a, E=1.0, motion=0, basis=0):
    """calc_consts_from_vector on vectors [n, 3] at UNIT energy, as the reference's class calls it, then k and h times E and Q times E E (exact at
    E = 1): returns k, h, Q, rdot_sign, thetadot_sign and the unit rdot."""
    vec = np.asarray(vec, dtype=F)
    r, V, a, scale, E = F(pos[1]), F(V), F(a), F(E), F(1)
    st, ct, tt = F(math.sin(pos[2])), F(math.cos(pos[2])), F(math.tan(pos[2]))
    sqrt = np.sqrt
    rhosq = r * r + (a * ct) * (a * ct)
    delta = r * r - 2 * r + a * a
    sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st
    e2nu = rhosq * delta / sigmasq
    e2psi = sigmasq * st * st / rhosq
    omega = 2 * a * r / sigmasq
    g00 = e2nu - omega * omega * e2psi
    g03 = omega * e2psi
    g11 = -rhosq / delta
    g33 = -e2psi
    rp0, rp1, rp2, rp3 = E, E * vec[:, 0], E * vec[:, 1], E * vec[:, 2]
    if motion == 0:
        et0 = (1 / sqrt(e2nu)) / sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu)
        et3 = (1 / sqrt(e2nu)) * V / sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu)
        e10 = (V - omega) * sqrt(e2psi / e2nu) / sqrt(e2nu - (V - omega) * (V - omega) * e2psi)
        e13 = (1 / sqrt(e2nu * e2psi)) * (e2nu + V * omega * e2psi - omega * omega * e2psi) / sqrt(e2nu - (V - omega) * (V - omega) * e2psi)
        tdot = rp0 * et0 + rp1 * e10
        phidot = rp0 * et3 + rp1 * e13
        if basis == 0:
            e22 = -1 / sqrt(rhosq)
            e31 = sqrt(delta / rhosq)
            rdot = rp3 * e31
            thetadot = rp2 * e22
        else:
            e32 = -1 / sqrt(rhosq)
            e21 = -1 * sqrt(delta / rhosq)
            rdot = rp2 * e21
            thetadot = rp3 * e32
    else:
        et0 = 1 / sqrt(g00 + g11 * V * V)
        et1 = V * et0
        e12 = 1 / sqrt(rhosq)
        e23 = sqrt(g00 / (g03 * g03 - g00 * g33))
        e20 = -(g03 / g00) * e23
        e30 = sqrt(-g11 / g00) * V / sqrt(g00 + g11 * V * V)
        e31 = sqrt(-g00 / g11) / sqrt(g00 + g11 * V * V)
        tdot = rp0 * et0 + rp1 * e20 + rp3 * e30
        phidot = rp1 * e23
        rdot = rp0 * et1 + rp3 * e31
        thetadot = rp2 * e12
    k = (1 - 2 * r / rhosq) * tdot + (2 * a * r * st * st / rhosq) * phidot
    h = phidot * ((r * r + a * a) * (r * r + a * a * ct * ct - 2 * r) * st * st + 2 * a * a * r * st * st * st * st)
    h = h - 2 * a * r * k * st * st
    h = h / (r * r + a * a * ct * ct - 2 * r)
    Q = rhosq * rhosq * thetadot * thetadot - (a * k * ct + h / tt) * (a * k * ct - h / tt)
    return scale * k, scale * h, (scale * scale) * Q, np.where(rdot > 0, 1, -1).astype(np.int32), np.where(thetadot > 0, 1, -1).astype(np.int32), rdot


def constants_vs_oracle_pointsource():
    """Worst relative difference of k, h, Q between constants() (motion 0, basis 0) and the oracle's PointSource on the live rays of the 354-ray grid
    of raytrace_rk4_test, with v = (sin a cos b, sin a sin b, cos a); also whether the signs agree wherever rdot != 0.  The only inexact inputs are
    numpy's sin / cos / acos against the C library's.  `python tests/healpix_rules.py` writes the figure and 16 x it into
    profiles/healpix_parity.json, which tests/test_healpix_rules.py holds later runs to."""
    import oracle_lib as ol
    V = ol.oracle().kro_disc_velocity(5.0, 0.998, 1)
    spec = ol.pointsource_spec([0, 5, 1e-3, 0], V, 0.998, 0.2, 0.2)
    rays = ol.oracle_pointsource(spec)
    live = rays[rays["steps"] != -1]
    alpha, beta = np.arccos(live["alpha"]), live["beta"]                   # rays[].alpha holds cos(alpha)
    v = np.stack([np.sin(alpha) * np.cos(beta), np.sin(alpha) * np.sin(beta), np.cos(alpha)], axis=1)
    k, h, Q, rs, ts, rdot = constants(v, spec.pos, spec.V, spec.spin, spec.E, motion=0, basis=0)
    worst = max(float((np.abs(x - live[n]) / np.abs(live[n])).max()) for n, x in (("k", k), ("h", h), ("Q", Q)))
    moving = rdot != 0
    signs = bool(np.array_equal(rs[moving], live["rdot_sign"][moving]) and np.array_equal(ts, live["thetadot_sign"]))
    return {"rays": int(len(rays)), "live": int(len(live)), "worst_rel": worst, "signs_agree": signs}


def records(spec, vecs, beta=None):
    """The records kr_healpix_init_dev_f64 builds from the vectors [n, 3] (emit = 0).  beta: the device's atan2 values when the caller pins the
    rest bit for bit (numpy's arctan2 is within an ulp of the correctly rounded one, not always equal to it)."""
    vecs = np.asarray(vecs, dtype=F)
    rays = np.zeros(len(vecs), dtype=capi.RAY_F64)
    rays["t"], rays["r"], rays["theta"], rays["phi"] = spec.pos[0], spec.pos[1], spec.pos[2], spec.pos[3]
    rays["alpha"] = vecs[:, 2]
    rays["beta"] = np.arctan2(vecs[:, 1], vecs[:, 0]) if beta is None else beta
    k, h, Q, rs, ts, _ = constants(vecs, spec.pos, spec.V, spec.spin, spec.E, spec.motion, spec.basis)
    rays["k"], rays["h"], rays["Q"], rays["rdot_sign"], rays["thetadot_sign"] = k, h, Q, rs, ts
    if spec.disc_source:
        rays["steps"] = np.where(ts > 0, -1, 0)              # set_disc_source()
    return rays


def source_vectors(spec, vec15):
    """The vectors of a source's rays, in ray order, from the [npix, 15] geometry: all five per pixel or the centres."""
    v = np.asarray(vec15, dtype=F).reshape(-1, 5, 3)
    return v.reshape(-1, 3) if spec.rays_per_pixel == 5 else v[:, 4, :].copy()


def classify(m, rays):
    """Class per record (0 dead, 1 disc, 2 escape, 3 lost, 4 self-zone) from the records as they are (phi wrapped, redshift set)."""
    r, theta, phi = rays["r"], rays["theta"], rays["phi"]
    with np.errstate(invalid="ignore"):
        live = rays["steps"] > 0
        on_disc = (theta >= PI2 - m.theta_tol) & (r >= m.r_isco) & (r < m.r_disc)
        own = on_disc & bool(m.self_zone) & (np.abs(r - m.source_r) <= 0.1 * m.source_r) & (np.abs(phi - m.source_phi) <= 0.1)
        cls = np.where(on_disc, np.where(own, 4, 1), np.where(r > m.r_esc, 2, 3))
    return np.where(live, cls, 0).astype(np.int64)


def powerlaw3(r, q1, rb1, q2, rb2, q3):
    r = np.asarray(r, dtype=F)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(r < rb1, r ** (-1 * q1), np.where(r < rb2, rb1 ** (q2 - q1) * r ** (-1 * q2), rb1 ** (q2 - q1) * rb2 ** (q3 - q2) * r ** (-1 * q3)))


def tallies(cls):
    return np.array([(cls > 0).sum(), (cls == 1).sum(), (cls == 2).sum(), (cls == 3).sum(), (cls == 4).sum(), 0], dtype=F)


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "healpix_parity.json")
    doc = json.load(open(path))
    m = constants_vs_oracle_pointsource()
    doc["constants_rule_vs_oracle_pointsource"].update(worst_rel=m["worst_rel"], allowed=16 * m["worst_rel"], live_rays=m["live"])
    json.dump(doc, open(path, "w"), indent=2)
    print(path, m)
