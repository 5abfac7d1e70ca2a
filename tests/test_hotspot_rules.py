"""CPU: the identities that pin the hot-spot rule of include/kr_trace.h (kr_hotspot) as tests/hotspot_rules.py states it, on the fixtures ip15 / ip16
(final__rk4, with g and mu from tests/angle_rules.py) and on synthetic records.  The device is held to this rule in tests/test_gpu_hotspot.py; here the
rule is held to what must be true of it."""
import math

import numpy as np
import pytest

import golden_cases as gc
import hotspot_rules as hr
from raytrace_cpu_amd import capi

SPIN, R_DISC = 0.998, 30.0
PI = math.pi


def r_isco():
    return gc.r_isco()


_REC = {}


def records(name):
    if name not in _REC:
        rays = np.ascontiguousarray(np.load(gc.golden_path(name))["final__rk4"])
        _REC[name] = hr.with_redshift(rays, -SPIN)
    return _REC[name]


def wide(rec, **kw):
    """The wide spot r_spot = 15, sigma = 4, cut = 3, sampled over two periods from the ring's median travel time."""
    args = dict(r_spot=15.0, sigma=4.0, cut=3.0, spin=SPIN, nt=32, g_index=4.0, r_isco=r_isco(), r_disc=R_DISC)
    args.update(kw)
    h = capi.hot_spot(**args)
    if "t0" not in kw:
        h.t0 = float(np.median(rec["t"][hr.disc_filter(h, rec) & hr.ring(h, rec)]))
    if "dt" not in kw:
        h.dt = 2 * (2 * PI / abs(h.omega)) / h.nt if h.omega else 1.0
    return h


def test_the_wide_spot_holds_most_of_the_disc_rays():
    rec, _, _ = records("ip16")
    h = wide(rec)
    res = hr.hotspot(h, rec)
    assert (res["on_disc"], res["used"]) == (42, 34)
    assert res["flux"].max() > 0 and res["pairs"] > res["used"]


@pytest.mark.parametrize("name", ["ip15", "ip16"])
@pytest.mark.parametrize("law", [(0, 0.0), (1, 2.06)])
def test_a_flat_static_spot_sums_the_weights(name, law):
    """(a) sigma = 1e8, cut = 40: s = 1 - exp(-800) to 1e-13 everywhere, so flux[k] = sum of limb g^-g_index over the rays used, for every k."""
    rec, mu, bad = records(name)
    h = wide(rec, sigma=1e8, cut=40.0, omega=0.0, dt=1.0, g_index=3.0)
    res = hr.hotspot(h, rec, law=law[0], coeff=law[1], mu=mu, bad=bad)
    keep = hr.disc_filter(h, rec) & (~bad if law[0] else True)
    assert res["used"] == keep.sum() > 30
    want = (hr.ar.limb_weight(law[0], law[1], mu)[keep] * rec["redshift"][keep] ** -3.0).sum()
    assert np.abs(res["flux"] / want - 1).max() <= 1e-13
    assert np.abs(res["sx"] / (hr.ar.limb_weight(law[0], law[1], mu)[keep] * rec["redshift"][keep] ** -3.0 * rec["alpha"][keep]).sum() - 1).max() <= 1e-12


@pytest.mark.parametrize("shear", [0, 1])
def test_periodicity(shear):
    """(b) dt = P / m and nt = 2 m: flux[k + m] = flux[k].  Under shear every radius has its own period, so the rigid spot only."""
    rec, _, _ = records("ip16")
    m = 12
    h = wide(rec, nt=2 * m, shear=0)
    h.dt = (2 * PI / h.omega) / m
    res = hr.hotspot(h, rec)
    assert res["flux"].max() > 0
    top = res["flux"].max()
    # the angle Om (T - t) ~ 300 rad carries 300 ulp of absolute error, times the sensitivity r r_spot / sigma^2 < 30
    assert np.abs(res["flux"][m:] - res["flux"][:m]).max() <= 1e-11 * top
    if shear:
        hs = wide(rec, nt=2 * m, shear=1, dt=h.dt)
        sheared = hr.hotspot(hs, rec)
        assert np.abs(sheared["flux"][m:] - sheared["flux"][:m]).max() > 1e-6 * top          # the arc winds up: no common period


def test_covariance_of_t0_and_phi0():
    """(c) the spot's azimuth is phi0 + Om (T - t): moving t0 by +delta moves it by +omega delta at every sample, which phi0 -> phi0 - omega delta undoes."""
    rec, _, _ = records("ip16")
    h = wide(rec, phi0=0.3)
    delta = 17.25
    moved = wide(rec, phi0=0.3 - h.omega * delta, t0=h.t0 + delta, dt=h.dt)
    a, b = hr.hotspot(h, rec), hr.hotspot(moved, rec)
    assert a["flux"].max() > 0 and a["used"] == b["used"]
    for k in ("flux", "sx", "sy"):
        assert hr.max_diff(b[k], a[k]) <= 1e-11
    shifted = wide(rec, phi0=0.3, t0=h.t0 + delta, dt=h.dt)
    assert hr.max_diff(hr.hotspot(shifted, rec)["flux"], a["flux"]) > 1e-3                   # without the counter-move the curve does change


@pytest.mark.parametrize("log_e", [False, True])
def test_the_spectrogram_sums_to_the_light_curve(log_e):
    """(d) on a grid that holds every ray, sum_e spec[k][e] = flux[k]."""
    rec, _, _ = records("ip16")
    grid = dict(e_min=0.1, de=1.1, ne=60, log_e=True) if log_e else dict(e_min=0.0, de=0.5, ne=60)
    h = wide(rec, line_energy=6.4, **grid)
    res = hr.hotspot(h, rec)
    ie = hr.energy_index(h, rec["redshift"][res["used_index"]])
    assert (ie >= 0).all() and len(set(ie)) > 3 and res["flux"].max() > 0
    assert hr.max_diff(res["spectrogram"].sum(axis=1), res["flux"]) <= 1e-14
    narrow = wide(rec, line_energy=6.4, e_min=0.0, de=0.5, ne=12)                             # E up to 6 only: the blue-shifted rays fall off the grid
    off = hr.hotspot(narrow, rec)
    assert (hr.energy_index(narrow, rec["redshift"][off["used_index"]]) < 0).any()
    assert np.array_equal(off["flux"], hr.hotspot(wide(rec), rec)["flux"])                   # ... and still add to the light curve
    assert (off["spectrogram"].sum(axis=1) <= off["flux"] * (1 + 1e-14)).all() and off["spectrogram"].sum() < 0.99 * off["flux"].sum()


def synthetic(n=200, seed=3):
    rng = np.random.default_rng(seed)
    return hr.synthetic_records(r=rng.uniform(7.0, 13.0, n), phi=rng.uniform(-PI, PI, n), g=rng.uniform(0.6, 1.3, n), t=rng.uniform(-50, 50, n),
                                x=rng.uniform(-10, 10, n), y=rng.uniform(-5, 5, n))


def test_mirror_symmetry():
    """(e) omega -> -omega with phi -> -phi and phi0 -> -phi0 leaves the curve unchanged (cos is even)."""
    rays = synthetic()
    h = capi.hot_spot(10.0, 1.5, phi0=0.4, omega=0.031, t0=-20.0, dt=3.0, nt=80, r_isco=1.3, r_disc=30.0)
    mirrored = rays.copy()
    mirrored["phi"] = -1 * rays["phi"]
    hm = capi.hot_spot(10.0, 1.5, phi0=-0.4, omega=-0.031, t0=-20.0, dt=3.0, nt=80, r_isco=1.3, r_disc=30.0)
    a, b = hr.hotspot(h, rays), hr.hotspot(hm, mirrored)
    assert a["used"] == b["used"] > 100 and a["flux"].max() > 0 and (a["flux"] == 0).sum() == 0
    for k in ("flux", "sx", "sy"):
        assert np.array_equal(a[k], b[k])                                                      # exact: every operation commutes with the sign


def test_the_peak_is_where_the_spot_passes_the_ray():
    """(f) records at r = r_spot, t = 0: the maximum over k falls on the sample with phi0 + omega T_k = phi (mod 2 pi)."""
    omega, nt = 0.05, 64
    dt = (2 * PI / omega) / nt
    for k_hit in (0, 5, 40, 63):
        phi = np.arctan2(math.sin(0.2 + omega * k_hit * dt), math.cos(0.2 + omega * k_hit * dt))
        rays = hr.synthetic_records(r=[10.0], phi=phi, t=0.0)
        h = capi.hot_spot(10.0, 1.0, phi0=0.2, omega=omega, t0=0.0, dt=dt, nt=nt, r_isco=1.3, r_disc=30.0)
        res = hr.hotspot(h, rays)
        assert res["used"] == 1 and int(np.argmax(res["flux"])) == k_hit
        assert abs(res["flux"][k_hit] - (1 - math.exp(-4.5))) <= 1e-12 and (res["flux"] == 0).sum() > nt // 2
    retro = capi.hot_spot(10.0, 1.0, phi0=0.2, omega=-omega, t0=0.0, dt=dt, nt=nt, r_isco=1.3, r_disc=30.0)
    rays = hr.synthetic_records(r=[10.0], phi=0.2 - omega * 5 * dt, t=0.0)
    assert int(np.argmax(hr.hotspot(retro, rays)["flux"])) == 5
    late = hr.synthetic_records(r=[10.0], phi=0.2, t=3 * dt)                                  # emitted 3 samples before it is seen
    assert int(np.argmax(hr.hotspot(h, late)["flux"])) == 3


@pytest.mark.parametrize("name", ["ip15", "ip16"])
def test_float64_noise_of_the_rule(name):
    """(g) float64 - longdouble, max-normalised, stays below 1e-12 on the fixtures with the wide spot."""
    rec, mu, bad = records(name)
    h = wide(rec, line_energy=6.4, e_min=0.0, de=0.5, ne=60)
    noise, lo, _ = hr.noise(h, rec, law=1, coeff=2.06, mu=mu, bad=bad)
    print(name, noise, lo["used"], lo["pairs"])
    assert lo["used"] > 20 and lo["flux"].max() > 0
    assert max(noise.values()) <= 1e-12


def test_keplerian_omega_and_the_constructor():
    from raytrace_cpu_amd import api
    assert api.keplerian_omega(10.0, 0.5) == 1 / (0.5 + 10.0 * math.sqrt(10.0))
    h = capi.hot_spot(10.0, 1.0, spin=0.5)
    assert h.omega == api.keplerian_omega(10.0, 0.5) and h.a_orbit == 0.5 and (h.nt, h.ne, h.shear, h.log_e) == (64, 0, 0, 0)
    assert capi.hot_spot(10.0, 1.0, omega=0.0).omega == 0.0
    assert api.hotspot_words(capi.hot_spot(10.0, 1.0, nt=7, ne=5)) == 7 * 8 + 4
    words = np.arange(7 * 8 + 4, dtype=np.float64)
    res = api.hotspot_from_words(capi.hot_spot(10.0, 1.0, nt=7, ne=5, t0=2.0, dt=0.5), words)
    assert res["spectrogram"].shape == (7, 5) and res["spectrogram"][1, 0] == 26 and (res["on_disc"], res["used"], res["bad_angle"]) == (56, 57, 58)
    assert np.isnan(res["x"][0]) and res["x"][1] == 8.0 and np.array_equal(res["time"], 2.0 + 0.5 * np.arange(7))
