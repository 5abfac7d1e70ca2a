"""CPU: the numpy statement of the source-to-observer link (tests/observer_rules.py) against the text of include/kr_trace.h (kr_observer_spec) and
against physics it does not contain: the closed form of the energy shift of a static emitter (which pins the sign and meaning of E_inf), conservation
of the tallies, the edges of the two index rules, that the first-order extrapolation of the direction earns its place, and the flat-space limit of
R_f.  No device; the oracle (tests/oracle_lib.py) traces where a trace is needed.  The measured figures are kept in profiles/observer_parity.json."""
import json
import math
import os

import numpy as np
import pytest

import golden_cases as gc
import observer_rules as obr
import oracle_lib as ol
from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = gc.cases()
FIXTURES = [(name, run) for name in ("ps_h5", "ps_h10") for run in ("euler", "rk4")]
EPS = 2.0 ** -52

# measured over FIXTURES (this file, test_shift_of_a_static_emitter_is_the_closed_form): the worst relative deviation of k / emit from the closed form is
# 2 ulp, rounding in emit (sixteen products and a sum) and in the closed form's own square root
SHIFT_DEV_MEASURED = 4.440892098500626e-16
SHIFT_BAR = 16 * SHIFT_DEV_MEASURED
# measured (test_the_extrapolation_earns_its_place): median |theta_obs(250) - theta_obs(4000)| = 1.82e-5 against median |theta(250) - theta(4000)| = 3.34e-2
EXTRAPOLATION_GAIN_MEASURED = 1832.0
# measured (test_flat_space_limit_of_the_reflection_fraction): R_f = 0.88513 against 0.82751 in flat space
FLAT_RF_DIFF_MEASURED = 0.0576


def golden(name, run):
    return np.ascontiguousarray(np.load(gc.golden_path(name))[f"final__{run}"])


def spec(spin=gc.SPIN, **kw):
    kw.setdefault("nmu", 20)
    return api.observer_spec(spin, gc.r_isco(), kw.pop("r_disc", 400.0), kw.pop("r_esc", 900.0), **kw)


def test_the_profile_keeps_the_measured_figures():
    prof = json.load(open(os.path.join(ROOT, "profiles", "observer_parity.json")))
    assert prof["shift_closed_form"]["worst_relative_deviation"] == SHIFT_DEV_MEASURED
    assert abs(prof["extrapolation"]["gain"] / EXTRAPOLATION_GAIN_MEASURED - 1) < 0.01
    assert abs(prof["flat_space_reflection_fraction"]["difference"] / FLAT_RF_DIFF_MEASURED - 1) < 0.01


def test_shift_of_a_static_emitter_is_the_closed_form():
    """V = 0: the emitter is at rest, so E_inf / E_emit = sqrt(g_tt) at the source for every ray.  E_inf = - k, or emit / k, would miss by a sign or
    by the square."""
    worst = 0.0
    for name, run in FIXTURES:
        src = CASES[name]["source"]
        assert src.V == 0.0
        want = obr.static_shift(src.pos[1], src.pos[2], gc.SPIN)
        p = obr.per_ray(spec(), golden(name, run))
        assert p["escape"].sum() > 300
        dev = float(np.abs(p["shift"][p["escape"]] / want - 1).max())
        print(f"{name} {run}: {int(p['escape'].sum())} escaping rays, shift {want:.15f}, worst deviation {dev:.3e}")
        worst = max(worst, dev)
        assert dev <= SHIFT_BAR, (name, run, dev)
    assert 0 < want < 1
    print(f"worst {worst:.3e} ({worst / EPS:.1f} ulp), bar {SHIFT_BAR:.3e}")


@pytest.mark.parametrize("name,run", FIXTURES)
def test_conservation(name, run):
    rays = golden(name, run)
    sp = spec(nmu=5, mu0=0.2, dmu=0.1, gamma=2.0, dist=1000.0, t0=1005.0, dt=1.5, nt=3)
    res = obr.observer(sp, rays)
    assert res["binned"] + res["outside_mu"] + res["inbound"] + res["bad_g"] == res["escape"] > 300
    assert res["return"] + res["escape"] + res["lost"] + res["other"] == res["ray_count"] == (rays["steps"] > 0).sum()
    assert res["outside_mu"] > 50 and 0 < res["outside_time"] < res["binned"] and res["count"].sum() == res["binned"]
    assert res["hist_n"].sum() + res["outside_time"] == res["binned"]
    # per bin: the time row and the weight outside the window make up sum_w (sums of a few hundred positive terms: 1e-13 is rounding)
    np.testing.assert_allclose(res["hist"].sum(axis=1) + res["outside_time_w"], res["sum_w"], rtol=1e-13, atol=0)
    # additivity over a split of the records
    cut = 517
    a, b = obr.observer(sp, rays[:cut]), obr.observer(sp, rays[cut:])
    for k in obr.TALLIES:
        assert a[k] + b[k] == res[k], k
    np.testing.assert_array_equal(a["count"] + b["count"], res["count"])
    for k in obr.SUMS:
        np.testing.assert_allclose(a[k] + b[k], res[k], rtol=1e-13, atol=0)
    # gamma = 0: every weight is one, the sums are the counts
    flat = obr.observer(spec(nmu=5, mu0=0.2, dmu=0.1), rays)
    np.testing.assert_array_equal(flat["sum_w"], flat["count"])
    assert flat["hist"].shape == (5, 0) and flat["outside_time"] == 0


def test_the_edges_of_the_inclination_bins():
    rays = obr.synthetic_records([3.0])
    outcomes = []
    for mu0, binned, imu in obr.mu_edge_cases():
        sp = api.observer_spec(0.0, 6.0, 400.0, 900.0, nmu=4, mu0=mu0, dmu=0.25)
        res = obr.observer(sp, rays)
        outcomes.append(bool(res["binned"]))
        assert (res["escape"], res["binned"], res["outside_mu"]) == (1, int(binned), int(not binned)), mu0
        assert list(np.flatnonzero(res["count"])) == ([imu] if binned else [])
        assert res["rays"]["theta_obs"][0] == math.pi / 3 and res["rays"]["phi_obs"][0] == 0.3
    assert outcomes == [False, True, False, True, True, True, False, True, False]


def test_the_edges_of_the_time_rows_and_what_is_binned_nowhere():
    """t0 = 8, dt = 0.5, nt = 4, dist = 0: ft = (t - 8) / 0.5 is exact for these t.  ft exactly 0 is row 0; just below 0 is outside; just below nt is row
    nt - 1; exactly nt is outside; a NaN t is outside -- and every one of them is in the four planes, where the NaN poisons sum_wt alone."""
    t = np.array([8.0, np.nextafter(8.0, 0.0), np.nextafter(10.0, 0.0), 10.0, np.nan, 9.25])
    sp = api.observer_spec(0.0, 6.0, 400.0, 900.0, nmu=2, mu0=0.0, dmu=0.5, gamma=2.0, t0=8.0, dt=0.5, nt=4)
    res = obr.observer(sp, obr.synthetic_records(t))
    assert list(res["rays"]["j"]) == [0, -1, 3, -1, -1, 2]
    assert (res["binned"], res["outside_time"], res["outside_mu"]) == (6, 3, 0) and list(res["count"]) == [0, 6]
    w = (1.0 / 1.25) ** 2
    assert list(res["hist"][1]) == [w, 0.0, w, w] and not res["hist"][0].any()
    assert res["sum_w"][1] == pytest.approx(6 * w, rel=1e-15) and res["sum_ws"][1] == pytest.approx(6 * w * 0.8, rel=1e-15) and math.isnan(res["sum_wt"][1])
    # pr = 0 (rdot_sign 0), an ingoing ray and a NaN constant: inbound.  shift = 0 (emit = inf), negative and NaN: bad_g.  steps = 0: not a ray.
    odd = obr.synthetic_records(np.full(8, 9.0))
    odd["rdot_sign"][:2] = 0, -1
    odd["k"][2] = np.nan
    odd["emit"][3:6] = np.inf, -1.0, np.nan
    odd["steps"][6] = 0
    res = obr.observer(sp, odd)
    assert (res["ray_count"], res["escape"], res["inbound"], res["bad_g"], res["binned"]) == (7, 7, 3, 3, 1)
    assert list(res["count"]) == [0, 1] and res["hist"][1][2] == w
    # the classes either side of their edges: on the disc from r_isco on and below r_disc, escaped beyond r_esc only, lost below r_isco only
    cls = obr.synthetic_records(np.full(7, 9.0), r=np.array([6.0, np.nextafter(400.0, 0.0), 400.0, 900.0, np.nextafter(900.0, 1e4), np.nextafter(6.0, 0.0), 6.0]),
                                theta=np.array([math.pi / 2] * 3 + [1.0] * 4))
    res = obr.observer(sp, cls)
    assert list(res["rays"]["cls"]) == [1, 1, -1, -1, 0, 2, -1]
    assert (res["return"], res["escape"], res["lost"], res["other"]) == (2, 1, 1, 3)


def test_the_self_zone_is_off_at_source_r_zero_and_on_otherwise():
    rays = obr.synthetic_records(np.full(2, 9.0), r=np.array([10.0, 10.9]), theta=math.pi / 2)
    off = obr.observer(api.observer_spec(0.0, 6.0, 400.0, 900.0), rays)
    on = obr.observer(api.observer_spec(0.0, 6.0, 400.0, 900.0, source_r=10.0, source_phi=0.25), rays)
    assert off["return"] == 2 and (on["return"], on["other"]) == (0, 2)
    far = obr.observer(api.observer_spec(0.0, 6.0, 400.0, 900.0, source_r=10.0, source_phi=0.45), rays)
    assert far["return"] == 2


@pytest.fixture(scope="module")
def h10_start():
    init = ol.oracle_pointsource(CASES["ps_h10"]["source"])
    ol.oracle().kro_redshift_start_f64(gc.SPIN, 0.0, 0, 0, ol.ptr(init), len(init))
    return init


def test_the_extrapolation_earns_its_place(h10_start):
    """The same rays stopped at r = 250 and at r = 4000: what is left of the way to infinity differs by a factor of 16, so the position angle moves by
    about b / 250 between the two, and theta_obs -- if the correction has the right sign and size -- by the second-order rest only."""
    runs = {}
    for r_max in (250.0, 4000.0):
        out, _ = ol.oracle_trace(gc._params(capi.RK4, r_max=r_max), h10_start)
        runs[r_max] = (out, obr.per_ray(spec(r_disc=100.0, r_esc=0.9 * r_max), out))
    (near, pn), (far, pf) = runs[250.0], runs[4000.0]
    both = pn["good"] & pf["good"]
    assert both.sum() > 400
    moved_obs = float(np.median(np.abs(pn["theta_obs"][both] - pf["theta_obs"][both])))
    moved_raw = float(np.median(np.abs(near["theta"][both] - far["theta"][both])))
    print(f"{int(both.sum())} rays escape in both runs: median |d theta_obs| = {moved_obs:.4e}, median |d theta| = {moved_raw:.4e}, gain {moved_raw / moved_obs:.1f}")
    assert moved_obs < moved_raw
    assert moved_raw / moved_obs > EXTRAPOLATION_GAIN_MEASURED / 4
    # and phi_obs likewise stays put where the position angle does not (a = 0.998 drags phi on the way out)
    assert np.median(np.abs(pn["phi_obs"][both] - pf["phi_obs"][both])) < np.median(np.abs(near["phi"][both] - far["phi"][both]))


def test_flat_space_limit_of_the_reflection_fraction():
    """A static source at h = 50 on the axis of a Schwarzschild hole, 40 x 63 rays, r_disc = 400, r_esc = 1000.  In flat space the classes are cones about
    the axis: `return` the annulus r_isco ... r_disc seen from h, `escape` everything that does not meet the plane inside r_esc.  The difference is light
    bending, of order a few M / h; a wrong class or a factor of 2 is an order of magnitude more."""
    h, r_disc, r_esc = 50.0, 400.0, 1000.0
    src = ol.pointsource_spec([0.0, h, 1e-3, 0.0], 0.0, 0.0, 1.99 / 40, 2 * np.pi / 63, cosalpha0=-0.995, cosalphamax=0.995, beta0=-np.pi, betamax=np.pi)
    init = ol.oracle_pointsource(src)
    ol.oracle().kro_redshift_start_f64(0.0, 0.0, 0, 0, ol.ptr(init), len(init))
    out, _ = ol.oracle_trace(gc._params(capi.RK4, spin=0.0, r_max=1.1 * r_esc), init)
    r_isco = gc.r_isco(0.0)
    res = obr.observer(api.observer_spec(0.0, r_isco, r_disc, r_esc), out)
    assert res["ray_count"] == 40 * 63 and res["inbound"] == res["bad_g"] == 0
    got = api.reflection_fraction(res)

    def cap(rho):                                                # the share of the sphere inside the cone from the source to radius rho on the plane
        return (1 - h / math.hypot(h, rho)) / 2
    flat = (cap(r_disc) - cap(r_isco)) / (1 - cap(r_esc))
    print(f"R_f = {got:.5f}, flat space {flat:.5f}, difference {got - flat:.5f}")
    assert abs(got - flat) <= 2 * FLAT_RF_DIFF_MEASURED
    assert got > flat                                            # bending towards the hole puts more of the sky on the disc
    # the direct flux of that source is close to isotropic: observer_flux is near 1 in the bins that no class edge cuts
    flux = api.observer_flux(api.observer_from_words(api.observer_spec(0.0, r_isco, r_disc, r_esc), words_of(res)))
    assert np.all(np.abs(flux[1:19] - 1) < 0.05)


def words_of(res):
    return np.concatenate([res["count"].astype(np.float64), res["sum_w"], res["sum_ws"], res["sum_wt"], res["hist"].ravel(), [float(res[k]) for k in obr.TALLIES]])


def test_word_layout_round_trip():
    sp = api.observer_spec(0.5, 4.2, 400.0, 900.0, nmu=3, mu0=0.1, dmu=0.2, nt=2, dt=1.0, t0=5.0)
    nw = api.observer_words(sp)
    assert nw == 3 * (4 + 2) + 10
    res = api.observer_from_words(sp, np.arange(nw, dtype=np.float64))
    assert list(res["count"]) == [0, 1, 2] and res["count"].dtype == np.int64 and list(res["sum_w"]) == [3.0, 4.0, 5.0] and list(res["sum_wt"]) == [9.0, 10.0, 11.0]
    assert res["hist"].tolist() == [[12.0, 13.0], [14.0, 15.0], [16.0, 17.0]]
    assert [res[k] for k in api.OBSERVER_TALLIES] == list(range(18, 28)) and api.OBSERVER_TALLIES == obr.TALLIES
    np.testing.assert_allclose(res["mu"], [0.2, 0.4, 0.6], rtol=1e-15)
    assert list(res["time"]) == [0.5, 1.5] and (res["mu0"], res["dmu"], res["t0"], res["dt"]) == (0.1, 0.2, 5.0, 1.0)
    assert api.observer_words(api.observer_spec(0.5, 4.2, 400.0, 900.0, nmu=7)) == 7 * 4 + 10
    default = api.observer_spec(0.5, 4.2, 400.0, 900.0, nmu=8, mu0=0.2)
    assert default.dmu == 0.1 and (default.cls.source_r, default.nt, default.gamma, default.dist) == (0.0, 0, 0.0, 0.0)


def test_direct_arrival_picks_the_bin_and_weighs_the_time():
    sp = api.observer_spec(0.0, 6.0, 400.0, 900.0, nmu=4, mu0=0.0, dmu=0.25, nt=3, dt=1.0, t0=100.0)
    words = np.zeros(api.observer_words(sp))
    res = api.observer_from_words(sp, words)
    res["count"][:] = [5, 0, 7, 9]
    res["sum_w"][:] = [2.0, 0.0, 4.0, 8.0]
    res["sum_ws"][:] = [1.0, 0.0, 3.0, 4.0]
    res["sum_wt"][:] = [200.0, 0.0, 404.0, 816.0]
    res["hist"][2] = [0.5, 3.0, 0.5]
    res.update({"ray_count": 64, "return": 30, "escape": 20})
    d = api.direct_arrival(res, 50.0)                            # cos(50 deg) = 0.643: bin 2
    assert d["bin"] == 2 and d["t0"] == 101.0 and d["shift"] == 0.75 and list(d["hist"]) == [0.5, 3.0, 0.5]
    assert d["flux"] == (4.0 / 64) / (0.25 / 2) == api.observer_flux(res)[2]
    assert api.direct_arrival(res, 10.0)["bin"] == 3 and api.direct_arrival(res, 10.0)["t0"] == 102.0
    assert api.direct_arrival(res, 89.0)["bin"] == 0
    assert api.reflection_fraction(res) == 1.5
    model_t0 = capi.response_model(capi.spectrum_model("table", 0.1, 0.1, 8, r_isco=6.0, r_disc=30.0, s=np.ones((1, 4)), s_e_min=0.05, s_de=1.5), d["t0"], 1.0, 4).t0
    assert model_t0 == 101.0                                     # what the response model takes as the arrival of the direct continuum
    with pytest.raises(capi.KrError, match="outside"):
        api.direct_arrival(res, 120.0)                           # below the plane: cos = -0.5, q = -2
    with pytest.raises(capi.KrError, match="no direct ray"):
        api.direct_arrival(res, 70.0)                            # cos = 0.342: bin 1, empty
    narrow = api.observer_from_words(api.observer_spec(0.0, 6.0, 400.0, 900.0, nmu=2, mu0=0.0, dmu=0.25), np.ones(18))
    with pytest.raises(capi.KrError, match="outside"):
        api.direct_arrival(narrow, 30.0)                         # cos = 0.866 beyond the last bin
    assert api.direct_arrival(narrow, 100.0)["bin"] == 0          # cos = -0.17: the band below the first edge belongs to bin 0
