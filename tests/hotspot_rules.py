"""TEST INFRASTRUCTURE: the hot-spot rule of include/kr_trace.h (kr_hotspot) restated in numpy over ray records, in the manner of tests/spectrum_rules.py.
Written from the header's text, not from the kernel; nothing here runs in the product path.

Every function takes a `dtype`: np.float64 evaluates the rule in the arithmetic of the device, np.longdouble evaluates the same rule with a 64-bit
mantissa.  The difference between the two, normalised by the largest value of the plane (noise()), is the rounding noise of the rule itself on the given
records: the yardstick the device is held to.  The difference is max-normalised, not element-wise: a sample near a zero of s is a small difference of
nearly equal numbers, and no relative bound holds there."""
import numpy as np

import angle_rules as ar
import line_rules as lr

CHUNK = 64           # records per block of the (records x samples) evaluation
PLANES = ("flux", "sx", "sy", "spectrogram")


def times(h, dtype=np.float64):
    """T_k = t0 + k dt."""
    return dtype(h.t0) + np.arange(h.nt).astype(dtype) * dtype(h.dt)


def disc_filter(h, rays):
    """steps > 0, r cos(theta) < 1e-2, r_isco <= r < r_disc, g > 0: the line's filter."""
    return lr.disc_filter(h, rays)


def ring(h, rays):
    """fabs(r - r_spot) < cut sigma, the product rounded once (in double: r is the record's double)."""
    with np.errstate(invalid="ignore"):
        return np.abs(rays["r"] - np.float64(h.r_spot)) < np.float64(h.cut) * np.float64(h.sigma)


def pattern_speed(h, r, dtype=np.float64):
    r = np.asarray(r).astype(dtype)
    if h.shear:
        return 1 / (dtype(h.a_orbit) + r * np.sqrt(r))
    return np.full(r.shape, dtype(h.omega))


def energy_index(h, g, dtype=np.float64):
    """ie per record, -1 where the ray adds to no cell (a NaN index or one outside [0, ne))."""
    g = np.asarray(g).astype(dtype)
    if h.ne <= 0:
        return np.full(g.shape, -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        E = dtype(h.line_energy) / g
        fe = np.log(E / dtype(h.e_min)) / np.log(dtype(h.de)) if h.log_e else (E - dtype(h.e_min)) / dtype(h.de)
        ok = (fe >= 0) & (fe < h.ne)
    return np.where(ok, np.floor(np.where(ok, fe, 0)), -1).astype(np.int64)


def shape(h, r, phi, t, Om, T, dtype=np.float64):
    """s for records x samples: exp(-d2 / (2 sigma sigma)) - exp(-cut cut / 2), as the header writes it."""
    r, phi, t, Om = (np.asarray(v).astype(dtype)[:, None] for v in (r, phi, t, Om))
    rs, sigma, cut = dtype(h.r_spot), dtype(h.sigma), dtype(h.cut)
    with np.errstate(all="ignore"):
        d2 = (r * r + rs * rs) - (2 * r * rs) * np.cos(phi - (dtype(h.phi0) + Om * (T[None, :] - t)))
        return np.exp(-d2 / (2 * sigma * sigma)) - np.exp(-cut * cut / 2)


def hotspot(h, rays, law=0, coeff=0.0, mu=None, bad=None, dtype=np.float64):
    """The rule over records that carry their redshift and their wrapped phi.  mu, bad: the emission angle and the bad-angle flag per record
    (tests/angle_rules.py) for the fused pass; None for the isotropic reduce form.  Returns {"time", "flux", "sx", "sy" (nt), "spectrogram" (nt x ne), all in
    dtype; "on_disc", "used", "bad_angle", "used_index", "pairs" (the (ray, sample) pairs with s > 0, a figure, not a result)}."""
    n = len(rays)
    on = disc_filter(h, rays)
    bad = np.zeros(n, dtype=bool) if bad is None else np.asarray(bad) & on
    keep = (on & ~bad if law != 0 else on.copy()) & ring(h, rays)
    idx = np.flatnonzero(keep)
    w = ar.limb_weight(law, coeff, mu).astype(dtype) if mu is not None else np.ones(n, dtype=dtype)
    T = times(h, dtype)
    out = {"flux": np.zeros(h.nt, dtype=dtype), "sx": np.zeros(h.nt, dtype=dtype), "sy": np.zeros(h.nt, dtype=dtype), "spectrogram": np.zeros((h.nt, h.ne), dtype=dtype)}
    pairs = 0
    for at in range(0, len(idx), CHUNK):
        j = idx[at:at + CHUNK]
        g = rays["redshift"][j].astype(dtype)
        with np.errstate(all="ignore"):
            c = (w[j] * g ** (-1 * dtype(h.g_index)))[:, None]
            s = shape(h, rays["r"][j], rays["phi"][j], rays["t"][j], pattern_speed(h, rays["r"][j], dtype), T, dtype)
            lit = s > 0
            cs = np.where(lit, c * s, dtype(0))
            pairs += int(lit.sum())
            out["flux"] += cs.sum(axis=0)
            out["sx"] += (np.where(lit, (c * rays["alpha"][j].astype(dtype)[:, None]) * s, dtype(0))).sum(axis=0)
            out["sy"] += (np.where(lit, (c * rays["beta"][j].astype(dtype)[:, None]) * s, dtype(0))).sum(axis=0)
        ie = energy_index(h, rays["redshift"][j], dtype)
        for row, e in zip(cs, ie):
            if e >= 0:
                out["spectrogram"][:, e] += row
    out.update(time=T, on_disc=int(on.sum()), used=int(len(idx)), bad_angle=int(bad.sum()), used_index=idx, pairs=pairs)
    return out


def max_diff(got, want):
    """max |got - want| / max |want| (0 when both are all zero; inf when only `want` is)."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    if got.size == 0:
        return 0.0
    top, d = np.abs(want).max(), np.abs(got - want).max()
    if not np.isfinite(d):
        return float("inf")
    return float(d / top) if top > 0 else (0.0 if d == 0 else float("inf"))


def noise(h, rays, **kw):
    """({plane: noise}, float64 result, longdouble result): the max-normalised difference between the float64 and the longdouble evaluation of the rule."""
    lo, hi = hotspot(h, rays, dtype=np.float64, **kw), hotspot(h, rays, dtype=np.longdouble, **kw)
    assert (lo["on_disc"], lo["used"], lo["bad_angle"]) == (hi["on_disc"], hi["used"], hi["bad_angle"])
    return {k: max_diff(lo[k], hi[k]) for k in PLANES}, lo, hi


def with_redshift(rays, spin, V=-1.0, reverse=1, projradius=0, lo=-np.pi, hi=np.pi):
    """Traced image-plane records as the redshift and range_phi passes leave them, by the rules of tests/angle_rules.py: (records, mu, bad)."""
    f = ar.frame(rays, spin, V, reverse, projradius)
    out = rays.copy()
    out["redshift"] = ar.redshift_of(rays, f, reverse)
    phi = out["phi"].copy()
    live = (out["steps"] > 0) & np.isfinite(phi)
    span = hi - lo
    for _ in range(64):
        over, under = live & (phi >= hi), live & (phi < lo)
        if not (over.any() or under.any()):
            break
        phi = np.where(over, phi - span, np.where(under, phi + span, phi))
    out["phi"] = phi
    return out, ar.mu_chi(f)[0], ar.bad_angle(f)


def synthetic_records(r, phi, g=1.0, t=0.0, x=0.0, y=0.0, theta=np.pi / 2, steps=1):
    """Records that carry only what the reduce form reads: steps, r, theta, phi, t, redshift, alpha, beta."""
    from raytrace_cpu_amd import capi
    r = np.atleast_1d(np.asarray(r, dtype=np.float64))
    rays = np.zeros(len(r), dtype=capi.RAY_F64)
    rays["r"], rays["theta"], rays["phi"], rays["t"], rays["redshift"], rays["alpha"], rays["beta"], rays["steps"] = r, theta, phi, t, g, x, y, steps
    return rays
