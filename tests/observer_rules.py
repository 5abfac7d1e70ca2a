"""TEST INFRASTRUCTURE: the rule of the source-to-observer link (include/kr_trace.h, kr_observer_spec) restated in numpy over ray records, in the
manner of tests/source_vel_rules.py.  Nothing here runs in the product path.

  per_ray(sp, rays, wrap=None)   -> per record: the class, and of the escaping rays theta_obs, phi_obs, mu, shift, t_ref, w, the two bin quotients
  observer(sp, rays, wrap=None)  -> the buffer of kr_reduce_observer_dev_f64 as the dict of api.observer_from_words, plus the per-bin sums of
                                    absolute terms ("abs"), the per-bin weight outside the time window ("outside_time_w") and per_ray's arrays ("rays")
  edge_margin(res)               -> how close the nearest record comes to an inclination-bin or time-row edge, relative to the quotient
  static_shift(r_s, theta_s, a)  -> the closed form of shift for an emitter at rest

Python evaluates `a + b * c / d` like C, so the expressions are written as the header writes them.  The momentum is angle_rules.momentum_from_consts
(kerr.h:300-335) with numpy's sin / cos; cos(theta_obs) is correctly rounded (mpmath, source_vel_rules.cos_cr), as csrc/kr_sincos.hpp delivers it; log
and pow are numpy's.  The device's log and pow are not correctly rounded and numpy's sin / cos in the momentum are not the device's, so a record within
rounding of a bin edge may fall on either side: the GPU tests assert edge_margin first."""
import math

import numpy as np

import angle_rules as ar
import reducer_rules as rr
import source_vel_rules as sv

TALLIES = ("ray_count", "return", "escape", "lost", "other", "binned", "outside_mu", "outside_time", "inbound", "bad_g")
PLANES = ("count", "sum_w", "sum_ws", "sum_wt")
SUMS = ("sum_w", "sum_ws", "sum_wt", "hist")


def static_shift(r_s, theta_s, a):
    """E_inf / E_emit of an emitter at rest at (r_s, theta_s): sqrt(g_tt) = sqrt(1 - 2 r_s / (r_s^2 + a^2 cos^2 theta_s))."""
    return math.sqrt(1 - 2 * r_s / (r_s * r_s + a * a * math.cos(theta_s) ** 2))


def per_ray(sp, rays, wrap=None):
    """The rule per record (arrays over all of `rays`; NaN / -1 / False where a step of the rule does not apply).  wrap = (lo, hi): range_phi first, as
    the fused pass classifies."""
    b = sp.cls
    n = len(rays)
    live = rays["steps"] > 0
    r, theta, t = rays["r"], rays["theta"], rays["t"]
    phi = rr.range_phi(rays["phi"], rays["steps"], *wrap) if wrap else rays["phi"]
    with np.errstate(all="ignore"):
        disc = (theta >= math.pi / 2) & (r >= b.r_isco) & (r < b.r_disc)
        away = (np.abs(r - b.source_r) > 0.1 * b.source_r) | (np.abs(phi - b.source_phi) > 0.1)
        escape = live & ~disc & (r > b.r_esc)
        lost = live & ~disc & ~escape & (r < b.r_isco)
        ret = live & disc & away
        other = live & ~escape & ~lost & ~ret
        pt, pr, ptheta, pphi = ar.momentum_from_consts(rays["k"], rays["h"], rays["Q"], rays["rdot_sign"], rays["thetadot_sign"], r, theta, sp.spin)
        finite = np.isfinite(pt) & np.isfinite(pr) & np.isfinite(ptheta) & np.isfinite(pphi)
        inbound = escape & ~((pr > 0) & finite)
        shift = rays["k"] / rays["emit"]                          # E_inf = + k
        bad_g = escape & ~inbound & ~(shift > 0)
        good = escape & ~inbound & ~bad_g
        theta_obs = np.where(good, theta + r * ptheta / pr, np.nan)
        phi_obs = np.where(good, phi + r * pphi / pr, np.nan)
        mu = np.full(n, np.nan)
        mu[good] = sv.cos_cr(theta_obs[good])
        q = (mu - sp.mu0) / sp.dmu
        ok_mu, imu = rr.bin_index(q, sp.nmu)
        binned = good & ok_mu
        t_ref = t + (sp.dist - r) + 2 * np.log(sp.dist / r) if sp.dist > 0 else t.astype(np.float64)
        t_ref = np.where(binned, t_ref, np.nan)
        w = np.where(binned, shift ** np.float64(sp.gamma), np.nan)
        ft = (t_ref - sp.t0) / sp.dt if sp.nt > 0 else np.full(n, np.nan)
        in_time = binned & (ft >= 0) & (ft < sp.nt)
        j = np.where(in_time, np.floor(np.where(in_time, ft, 0.0)), -1).astype(np.int64)
    cls = np.where(escape, 0, np.where(ret, 1, np.where(lost, 2, -1)))
    return {"live": live, "cls": np.where(live, cls, -1), "escape": escape, "return": ret, "lost": lost, "other": other, "inbound": inbound, "bad_g": bad_g,
            "good": good, "theta_obs": theta_obs, "phi_obs": phi_obs, "mu": mu, "shift": np.where(escape, shift, np.nan), "q": np.where(good, q, np.nan),
            "binned": binned, "imu": np.where(binned, imu, -1), "t_ref": t_ref, "w": w, "ft": np.where(binned, ft, np.nan), "in_time": in_time, "j": j}


def observer(sp, rays, wrap=None):
    """kr_reduce_observer_dev_f64 in numpy.  Sums are exact per bin (reducer_rules.bin_sums); out["abs"] holds the per-bin sums of absolute terms."""
    p = per_ray(sp, rays, wrap)
    nmu, nt = sp.nmu, sp.nt
    m = p["binned"]
    imu, w, shift, t_ref = p["imu"][m], p["w"][m], p["shift"][m], p["t_ref"][m]
    out = {"abs": {}, "rays": p}
    out["count"] = np.bincount(imu, minlength=nmu).astype(np.int64)
    with np.errstate(all="ignore"):
        for key, terms in (("sum_w", w), ("sum_ws", w * shift), ("sum_wt", w * t_ref)):
            out[key], out["abs"][key] = rr.bin_sums(imu, terms, nmu)
    it = p["in_time"]
    cell = p["imu"][it] * nt + p["j"][it]
    hist, hist_abs = rr.bin_sums(cell, p["w"][it], nmu * nt) if nt > 0 else (np.zeros(0), np.zeros(0))
    out["hist"], out["abs"]["hist"] = hist.reshape(nmu, nt), hist_abs.reshape(nmu, nt)
    out["hist_n"] = np.bincount(cell, minlength=nmu * nt).reshape(nmu, nt) if nt > 0 else np.zeros((nmu, 0), dtype=np.int64)
    late = m & ~it if nt > 0 else np.zeros(len(rays), dtype=bool)
    out["outside_time_w"] = rr.bin_sums(p["imu"][late], p["w"][late], nmu)[0]
    good = p["good"]
    out.update({"ray_count": int(p["live"].sum()), "return": int(p["return"].sum()), "escape": int(p["escape"].sum()), "lost": int(p["lost"].sum()),
                "other": int(p["other"].sum()), "binned": int(m.sum()), "outside_mu": int((good & ~m).sum()), "outside_time": int(late.sum()),
                "inbound": int(p["inbound"].sum()), "bad_g": int(p["bad_g"].sum())})
    return out


def edge_margin(res):
    """The smallest distance of a quotient from a whole number, relative to max(1, |quotient|): over the inclination quotients of every ray that reaches
    the bin test and the time quotients of every binned ray.  inf when there is none.  A fixture is safe for an exact count comparison against
    arithmetic that differs in the last bits when this is well above those bits (the GPU tests ask for 1e-9)."""
    p = res["rays"]
    worst = math.inf
    for x in (p["q"][p["good"]], p["ft"][p["binned"]]):
        x = x[np.isfinite(x)]
        if x.size:
            worst = min(worst, float((np.abs(x - np.rint(x)) / np.maximum(1.0, np.abs(x))).min()))
    return worst


def synthetic_records(t, theta=math.pi / 3, r=2000.0, k=1.0, emit=1.25, rdot_sign=1, steps=5):
    """Escaping records whose direction at infinity is their own position angle, for a spec with spin = 0: h = Q = 0 make ptheta = pphi = 0 exactly, so
    theta_obs = theta and mu = cos(theta), correctly rounded; t_ref = t with dist = 0; shift = k / emit.  Every argument broadcasts against t."""
    from raytrace_cpu_amd import capi
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    rays = np.zeros(len(t), dtype=capi.RAY_F64)
    rays["t"], rays["r"], rays["theta"], rays["phi"] = t, r, theta, 0.3
    rays["k"], rays["emit"], rays["rdot_sign"], rays["thetadot_sign"], rays["steps"] = k, emit, rdot_sign, 1, steps
    return rays


def mu_edge_cases(nmu=4, dmu=0.25):
    """[(mu0, binned, imu)]: the inclination quotient of synthetic_records() on and beside every edge of the index rule -- q exactly -1 (out), its
    neighbour above (bin 0), exactly 0 and its two neighbours (bin 0: the band -1 < q <= 0 belongs to bin 0), exactly nmu (out) and its neighbour
    below (bin nmu - 1).  mu = cos(pi / 3) lies in [0.5, 1) and dmu is a power of two, so mu - mu0 and the division are exact for these mu0."""
    mu = float(sv.cos_cr(np.array([math.pi / 3]))[0])
    assert 0.5 <= mu < 0.75

    def beside(x, ulps):
        for _ in range(abs(ulps)):
            x = float(np.nextafter(x, math.copysign(math.inf, ulps)))
        return x
    lo, zero, hi = mu + dmu, mu, mu - nmu * dmu
    assert (mu - lo) / dmu == -1.0 and (mu - zero) / dmu == 0.0 and (mu - hi) / dmu == float(nmu)
    # (four ulps of hi: the difference from mu then lies on the grid of doubles either side of nmu dmu = 1, no rounding tie)
    cases = [(lo, False, -1), (beside(lo, -1), True, 0), (beside(lo, 1), False, -1), (zero, True, 0), (beside(zero, 1), True, 0), (beside(zero, -1), True, 0),
             (hi, False, -1), (beside(hi, 4), True, nmu - 1), (beside(hi, -4), False, -1)]
    for mu0, binned, imu in cases:                               # the intent above against the quotient in plain Python floats
        q = (mu - mu0) / dmu
        assert (-1 < q < nmu) == binned and (not binned or int(q) == imu) and abs(q - round(q)) < 1e-14, (mu0, q)
    return cases


def check_observer(got, want, rtol, label=""):
    """The bar of the GPU tests: every tally and every count exact, a weighted bin non-zero exactly where the rule has rays in it, every weighted sum
    within rtol of the per-bin sum of absolute terms, non-finite bins alike.  No bin is left out.  Returns the worst relative sum error."""
    for k in TALLIES:
        assert got[k] == want[k], (label, k, got[k], want[k])
    np.testing.assert_array_equal(got["count"], want["count"], err_msg=f"{label} count")
    worst, problems = rr.sum_errors(got, want, SUMS)
    assert problems == [] and worst <= rtol, (label, worst, problems)
    assert np.array_equal(np.asarray(got["hist"]) != 0, want["hist_n"] != 0) or not np.isfinite(want["hist"]).all(), (label, "hist occupancy")
    assert np.array_equal(np.asarray(got["sum_w"]) != 0, want["count"] != 0) or not np.isfinite(want["sum_w"]).all(), (label, "sum_w occupancy")
    return worst
