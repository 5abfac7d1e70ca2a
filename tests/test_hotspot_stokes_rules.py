"""CPU: the identities that pin the Stokes light-curve rule of include/kr_trace.h (the Stokes rule under kr_hotspot) as tests/hotspot_stokes_rules.py
states it, on the fixtures ip15 / ip16 (final__rk4, with g from tests/angle_rules.py and mu, c2, s2, bad-pol from tests/polarisation_rules.py) and on
oracle-traced 65 x 65 planes.  The device is held to this rule in tests/test_gpu_hotspot_stokes.py; here the rule is held to what must be true of it,
and the integer that the device's physics check reproduces -- the winding number of (Q, U) over one orbit -- is computed and explained."""
import math

import numpy as np
import pytest

import golden_cases as gc
import hotspot_rules as hr
import hotspot_stokes_rules as hs
import oracle_lib as ol
from raytrace_cpu_amd import capi

SPIN, DIST, R_DISC, INC_DEG = 0.998, 10000.0, 30.0, 80.0        # the fixtures' plane: a = 0.998 seen at 80 degrees
PI = math.pi
LAOR, CHANDRA = (1, 2.06), (1, 0.1171)

_REC = {}


def records(name):
    """(records with redshift and wrapped phi, polar(...) of them)."""
    if name not in _REC:
        rays = np.ascontiguousarray(np.load(gc.golden_path(name))["final__rk4"])
        rec, _, _ = hr.with_redshift(rays, -SPIN)
        _REC[name] = rec, hs.polar(rec, -SPIN, INC_DEG)
    return _REC[name]


def wide(rec, **kw):
    """The wide spot of tests/test_hotspot_rules.py: r_spot = 15, sigma = 4, cut = 3, two periods from the ring's median travel time."""
    args = dict(r_spot=15.0, sigma=4.0, cut=3.0, spin=SPIN, nt=32, g_index=4.0, r_isco=gc.r_isco(), r_disc=R_DISC)
    args.update(kw)
    h = capi.hot_spot(**args)
    if "t0" not in kw:
        h.t0 = float(np.median(rec["t"][hr.disc_filter(h, rec) & hr.ring(h, rec)]))
    if "dt" not in kw:
        h.dt = 2 * (2 * PI / abs(h.omega)) / h.nt if h.omega else 1.0
    return h


def spoilt(rec, h):
    """A copy with three ring records made bad-pol: Q x 1e4 twice (mu > 1: bad-angle) and alpha = beta = NaN once (no observer)."""
    idx = np.flatnonzero(hr.disc_filter(h, rec) & hr.ring(h, rec))[[1, 7, 20]]
    out = rec.copy()
    out["Q"][idx[:2]] *= 1e4
    out["alpha"][idx[2]] = out["beta"][idx[2]] = np.nan
    return out, idx


@pytest.mark.parametrize("name", ["ip15", "ip16"])
@pytest.mark.parametrize("pol_law", [(0, 0.3), (0, -0.3), CHANDRA])
def test_the_polarised_flux_bounds_q_and_u(name, pol_law):
    """Q^2 + U^2 <= P^2 per sample: |sum w (c2, s2)| <= sum |w| for unit vectors (c2, s2)."""
    rec, pol = records(name)
    h = wide(rec)
    res = hs.hotspot_stokes(h, rec, pol, limb=LAOR, pol_law=pol_law)
    assert res["used"] > 30 and res["p"].max() > 0 and res["bad_pol"] == 0
    assert (np.hypot(res["q"], res["u"]) <= res["p"] * (1 + 1e-12)).all()
    assert (np.hypot(res["q"], res["u"])[res["p"] > 0] > 0).any()
    assert res["delta_max"] <= abs(pol_law[1])


@pytest.mark.parametrize("name", ["ip15", "ip16"])
@pytest.mark.parametrize("limb", [(0, 0.0), LAOR, (2, 0.0)])
def test_no_degree_gives_the_hotspot_rule_without_the_bad_pol_records(name, limb):
    """Law 0 with coeff = 0: Q = U = 0 exactly, and flux, sx, sy and the spectrogram are the kr_hotspot rule's on the records that are not bad-pol."""
    rec0, _ = records(name)
    h = wide(rec0, line_energy=6.4, e_min=0.5, de=4.0, ne=16)
    rec, idx = spoilt(rec0, h)
    rec, _, _ = hr.with_redshift(rec, -SPIN)                  # the spoilt constants of motion move g
    pol = hs.polar(rec, -SPIN, INC_DEG)
    res = hs.hotspot_stokes(h, rec, pol, limb=limb, pol_law=(0, 0.0))
    assert res["bad_pol"] == 3 and sorted(res["bad_index"]) == sorted(idx)
    assert not res["q"].any() and not res["u"].any() and not res["p"].any()
    keep = np.ones(len(rec), dtype=bool)
    keep[idx] = False
    plain = hr.hotspot(h, rec[keep], law=limb[0], coeff=limb[1], mu=pol["mu"][keep], bad=np.zeros(int(keep.sum()), dtype=bool))
    assert res["used"] == plain["used"] > 25 and res["on_disc"] == plain["on_disc"] + 3
    for k in ("flux", "sx", "sy", "spectrogram"):
        assert np.array_equal(res[k], plain[k]), k
    assert np.isfinite(res["flux"]).all() and res["flux"].max() > 0


@pytest.mark.parametrize("pol_law", [(0, 0.3), CHANDRA])
def test_the_sign_of_the_coefficient_is_the_sign_of_q_and_u(pol_law):
    rec, pol = records("ip16")
    h = wide(rec)
    a = hs.hotspot_stokes(h, rec, pol, limb=LAOR, pol_law=pol_law)
    b = hs.hotspot_stokes(h, rec, pol, limb=LAOR, pol_law=(pol_law[0], -1 * pol_law[1]))
    assert np.abs(a["q"]).max() > 0 and np.abs(a["u"]).max() > 0
    assert np.array_equal(b["q"], -1 * a["q"]) and np.array_equal(b["u"], -1 * a["u"])
    for k in ("flux", "sx", "sy", "p"):
        assert np.array_equal(a[k], b[k])


def test_a_static_spot_has_one_q_and_one_u():
    """omega = 0: the angle of the rule does not depend on T, so every sample carries the same sums."""
    rec, pol = records("ip15")
    h = wide(rec, omega=0.0, dt=3.0)
    res = hs.hotspot_stokes(h, rec, pol, limb=LAOR, pol_law=CHANDRA)
    assert res["used"] > 30 and np.abs(res["q"]).max() > 0
    for k in ("flux", "q", "u", "p"):
        assert (res[k] == res[k][0]).all(), k


@pytest.mark.parametrize("name", ["ip15", "ip16"])
def test_the_rows_of_the_spectrogram_sum_to_the_flux(name):
    rec, pol = records(name)
    h = wide(rec, line_energy=6.4, e_min=0.5, de=4.0, ne=16)            # a grid that holds every ray
    res = hs.hotspot_stokes(h, rec, pol, limb=LAOR, pol_law=CHANDRA)
    assert res["spectrogram"].max() > 0 and (hr.energy_index(h, rec["redshift"][res["used_index"]]) >= 0).all()
    assert hr.max_diff(res["spectrogram"].sum(axis=1), res["flux"]) <= 1e-13


@pytest.mark.parametrize("name", ["ip15", "ip16"])
def test_float64_against_longdouble_noise(name):
    rec, pol = records(name)
    h = wide(rec, line_energy=6.4, e_min=0.5, de=4.0, ne=16)
    noise, lo, hi = hs.noise(h, rec, pol, limb=LAOR, pol_law=CHANDRA)
    print(f"{name}: used {lo['used']}, pairs {lo['pairs']}, max P {lo['p'].max():.3e}; float64 - longdouble: " + ", ".join(f"{k} {v:.2e}" for k, v in noise.items()))
    assert lo["used"] > 30 and all(v < 1e-12 for v in noise.values())
    if np.finfo(np.longdouble).nmant > 52:
        assert max(noise.values()) > 0


def test_from_words_reads_the_layout_of_the_header():
    h = capi.hot_spot(10.0, 1.0, nt=3, ne=2, r_isco=1.3, r_disc=30.0)
    words = np.arange(3 * 7 + 4, dtype=np.float64)
    got = hs.from_words(h, words)
    assert got["q"].tolist() == [9, 10, 11] and got["u"].tolist() == [12, 13, 14] and got["spectrogram"].tolist() == [[15, 16], [17, 18], [19, 20]]
    assert (got["on_disc"], got["used"], got["bad_pol"]) == (21, 22, 23)


def test_winding_number_of_known_curves():
    t = 2 * PI * np.arange(40) / 40
    assert hs.winding_number(np.cos(t), np.sin(t)) == 1
    assert hs.winding_number(np.cos(2 * t), -1 * np.sin(2 * t)) == -2
    assert hs.winding_number(3 + np.cos(t), np.sin(t)) == 0


# ---- the physics check of tests/test_gpu_hotspot_stokes.py, first here with the rule on oracle-traced records ---------------------------------------
def plane(incl, nx=64):
    d = 2 * R_DISC / nx
    return ol.imageplane_spec(DIST, incl, -R_DISC, R_DISC, d, -R_DISC, R_DISC, d, SPIN)


def traced_plane(incl):
    """The 65 x 65 ray plane of tests/test_gpu_hotspot.py traced by the CPU oracle (strict RK4), with redshift and wrapped phi by the numpy rules."""
    p = capi.default_params(-SPIN)
    p.precision, p.integrator, p.theta_max, p.r_max = 100.0, capi.RK4, PI / 2, 1.1 * DIST
    p.stop_kind, p.flags = capi.STOP_THETA, 0
    rays = ol.oracle_imageplane(plane(incl))
    ol.oracle().kro_redshift_start_f64(-SPIN, 0.0, 1, 0, ol.ptr(rays), len(rays))
    out, _ = ol.oracle_trace(p, rays)
    rec, _, _ = hr.with_redshift(out, -SPIN)
    return rec, hs.polar(rec, -SPIN, incl)


def orbit_spot(nt=64, omega_sign=1):
    """r_spot = 10, sigma = 1.5 over one Keplerian period from t0 = DIST: the prograde spot of the GPU test."""
    h = capi.hot_spot(10.0, 1.5, cut=3.0, phi0=0.4, spin=SPIN, t0=DIST, nt=nt, g_index=4.0, r_isco=gc.r_isco(), r_disc=R_DISC)
    h.dt = (2 * PI * (SPIN + h.r_spot ** 1.5)) / nt
    h.omega *= omega_sign
    return h


WINDING_AT_30_DEGREES = 0


@pytest.mark.parametrize("incl,want,clear", [(10.0, 2, 0.3), (30.0, WINDING_AT_30_DEGREES, 0.1)])
def test_winding_number_of_the_stokes_loop(incl, want, clear):
    """The emitted vector is perpendicular to the projection of the photon direction onto the disc, in the frame of the gas.  That projection has two
    parts: the line of sight's, of size sin(i), fixed in the observer's frame, and the aberration's, of the size of the orbital speed (0.33 at r = 10),
    which points against the motion and so turns once per orbit.  Seen at 10 degrees the turning part wins: the angle makes a full turn per orbit and
    (Q, U) two loops about the origin, counter-clockwise for a prograde spot, clockwise for a retrograde pattern.  At 30 degrees (sin i = 0.5) the fixed
    part wins at r = 10: the angle swings to and fro (-42 ... +56 degrees) and the curve stays on one side of the origin: winding number 0.  `clear`:
    the curve keeps that fraction of max P away from the origin, so the integer does not hang on a sample."""
    rec, pol = traced_plane(incl)
    for sign in (1, -1):
        h = orbit_spot(omega_sign=sign)
        res = hs.hotspot_stokes(h, rec, pol, pol_law=(0, 0.3))
        assert res["used"] > 100 and res["bad_pol"] == 0
        gap = float(np.hypot(res["q"], res["u"]).min() / res["p"].max())
        w = hs.winding_number(res["q"], res["u"])
        print(f"incl {incl}, omega sign {sign}: used {res['used']}, winding number {w}, |(Q, U)| >= {gap:.3f} max P")
        assert gap > clear and w == sign * want
        assert hs.winding_number(*(hs.hotspot_stokes(orbit_spot(nt=96, omega_sign=sign), rec, pol, pol_law=(0, 0.3))[k] for k in ("q", "u"))) == w
