"""TEST INFRASTRUCTURE: the Stokes light curves of the orbiting hot spot (include/kr_trace.h, the Stokes rule under kr_hotspot) restated in numpy over
ray records, on top of tests/hotspot_rules.py (filter, ring, pattern speed, energy bin, the shifted Gaussian) and tests/polarisation_rules.py (frame,
Walker-Penrose transport, c2, s2, bad-pol, the degree law).  Written from the header's text, not from the kernel; nothing here runs in the product path.

Per record the rule takes mu, c2, s2 and bad-pol from polarisation_rules.polarisation -- evaluated in float64, like the records themselves: they are
the per-record inputs of the sums -- and then evaluates the weights, the shape and the sums in `dtype`: np.float64, the arithmetic of the device, or
np.longdouble, the same rule with a 64-bit mantissa.  noise() is their max-normalised difference, as in hotspot_rules.

Besides Q and U the rule returns P[k] = sum c |delta| s, the polarised flux with no cancellation between rays.  Differences in Q and U are normalised
by max_k P[k], not by max |Q|: where the rays' Q cancel, max |Q| is small for no reason that bears on accuracy, and the quotient would inflate; where
one sample dominates, it would hide the rest."""
import numpy as np

import angle_rules as ar
import hotspot_rules as hr
import polarisation_rules as pr

CURVES = ("flux", "sx", "sy", "q", "u")
PLANES = CURVES + ("spectrogram",)


def polar(rays, spin, inc_deg, V=-1.0, reverse=1, projradius=0):
    """polarisation_rules.polarisation: mu, c2, s2, bad (and the rest) per record, in float64."""
    return pr.polarisation(rays, spin, inc_deg, V, reverse, projradius)


def hotspot_stokes(h, rays, pol, limb=(0, 0.0), pol_law=(0, 0.0), dtype=np.float64):
    """The rule over records that carry their redshift and their wrapped phi.  pol: polar(...) of the same records.  limb, pol_law: (law, coeff).
    Returns {"time", "flux", "sx", "sy", "q", "u", "p" (nt), "spectrogram" (nt x ne), all in dtype; "on_disc", "used", "bad_pol", "used_index",
    "bad_index", "pairs", "delta_max" (the largest |delta| of a used record)}."""
    on = hr.disc_filter(h, rays)
    in_ring = on & hr.ring(h, rays)
    bad = in_ring & pol["bad"]
    idx = np.flatnonzero(in_ring & ~pol["bad"])
    T = hr.times(h, dtype)
    out = {k: np.zeros(h.nt, dtype=dtype) for k in CURVES + ("p",)}
    out["spectrogram"] = np.zeros((h.nt, h.ne), dtype=dtype)
    pairs, delta_max = 0, 0.0
    for at in range(0, len(idx), hr.CHUNK):
        j = idx[at:at + hr.CHUNK]
        g = rays["redshift"][j].astype(dtype)
        mu = pol["mu"][j]
        with np.errstate(all="ignore"):
            w = ar.limb_weight(limb[0], limb[1], mu).astype(dtype)
            delta = pr.degree(pol_law[0], pol_law[1], mu).astype(dtype)
            c = (w * g ** (-1 * dtype(h.g_index)))[:, None]
            cd = c * delta[:, None]
            s = hr.shape(h, rays["r"][j], rays["phi"][j], rays["t"][j], hr.pattern_speed(h, rays["r"][j], dtype), T, dtype)
            lit = s > 0
            zero = dtype(0)
            cs = np.where(lit, c * s, zero)
            pairs += int(lit.sum())
            delta_max = max(delta_max, float(np.abs(delta).max()))
            out["flux"] += cs.sum(axis=0)
            out["sx"] += np.where(lit, (c * rays["alpha"][j].astype(dtype)[:, None]) * s, zero).sum(axis=0)
            out["sy"] += np.where(lit, (c * rays["beta"][j].astype(dtype)[:, None]) * s, zero).sum(axis=0)
            out["q"] += np.where(lit, (cd * pol["c2"][j].astype(dtype)[:, None]) * s, zero).sum(axis=0)
            out["u"] += np.where(lit, (cd * pol["s2"][j].astype(dtype)[:, None]) * s, zero).sum(axis=0)
            out["p"] += np.where(lit, np.abs(cd) * s, zero).sum(axis=0)
        ie = hr.energy_index(h, rays["redshift"][j], dtype)
        for row, e in zip(cs, ie):
            if e >= 0:
                out["spectrogram"][:, e] += row
    out.update(time=T, on_disc=int(on.sum()), used=int(len(idx)), bad_pol=int(bad.sum()), used_index=idx, bad_index=np.flatnonzero(bad), pairs=pairs,
               delta_max=delta_max)
    return out


def scale(want, k):
    """What a difference in plane k is divided by: max_k P for q and u, the plane's own largest magnitude otherwise."""
    ref = want["p"] if k in ("q", "u") else want[k]
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(ref).max()) if ref.size else 0.0


def diff(got, want, k):
    """max |got[k] - want[k]| / scale(want, k) (0 when both are all zero; inf when only the scale is)."""
    a, b = np.asarray(got[k], dtype=np.longdouble), np.asarray(want[k], dtype=np.longdouble)
    if a.size == 0:
        return 0.0
    d, top = np.abs(a - b).max(), scale(want, k)
    if not np.isfinite(d):
        return float("inf")
    return float(d / top) if top > 0 else (0.0 if d == 0 else float("inf"))


def noise(h, rays, pol, **kw):
    """({plane: noise}, float64 result, longdouble result), as hotspot_rules.noise."""
    lo, hi = hotspot_stokes(h, rays, pol, dtype=np.float64, **kw), hotspot_stokes(h, rays, pol, dtype=np.longdouble, **kw)
    assert (lo["on_disc"], lo["used"], lo["bad_pol"]) == (hi["on_disc"], hi["used"], hi["bad_pol"])
    return {k: diff(lo, hi, k) for k in PLANES}, lo, hi


def from_words(h, words):
    """The nt (5 + ne) + 4 doubles of the Stokes entry points as the dict of hotspot_stokes (no "p")."""
    words, nt, ne = np.asarray(words, dtype=np.float64), h.nt, h.ne
    assert len(words) == nt * (5 + ne) + 4
    out = {k: words[q * nt:(q + 1) * nt] for q, k in enumerate(CURVES)}
    out["spectrogram"] = words[5 * nt:5 * nt + nt * ne].reshape(nt, ne)
    out.update(on_disc=int(round(words[-4])), used=int(round(words[-3])), bad_pol=int(round(words[-2])))
    return out


def winding_number(q, u):
    """How often the closed curve (q[k], u[k]), k = 0 .. nt - 1 and back to k = 0, turns about the origin: the sum of the angle steps, each taken in
    (-pi, pi], over 2 pi, rounded.  Counter-clockwise is positive.  The caller makes sure that no sample sits at the origin."""
    ang = np.arctan2(np.asarray(u, dtype=np.float64), np.asarray(q, dtype=np.float64))
    step = np.diff(np.concatenate([ang, ang[:1]]))
    step = (step + np.pi) % (2 * np.pi) - np.pi
    return int(round(float(step.sum()) / (2 * np.pi)))
