"""CPU: the identities that pin the Stokes-spectra rule of include/kr_trace.h (STOKES SPECTRA under kr_spectrum_model) as tests/spectrum_stokes_rules.py
states it, on the fixtures ip15 / ip16 (final__rk4, a = 0.998 seen at 80 degrees, with g from tests/angle_rules.py and mu, c2, s2, bad-pol from
tests/polarisation_rules.py).  The device is held to this rule in tests/test_gpu_spectrum_stokes.py; here the rule is held to what must be true of it,
and to the physics it was written for: the degree of a thermal disc falls with energy and its angle at the soft end lies along the disc.

Each case first asserts that it is not vacuous: used > 30 and a non-zero Q or U."""
import math

import numpy as np
import pytest

import golden_cases as gc
import hotspot_rules as hr
import polarisation_rules as pr
import spectrum_rules as sr
import spectrum_stokes_rules as ss
from raytrace_cpu_amd import api, capi

SPIN, R_DISC, INC_DEG = 0.998, 30.0, 80.0
LAOR, CHANDRA = (1, 2.06), (1, 0.1171)
LIMBS = {"iso": (0, 0.0), "laor": LAOR, "bright": (2, 0.0)}
EMIS = dict(q1=3.0, rb1=4.0, q2=2.5, rb2=10.0, q3=3.0)

_REC = {}


def records(name):
    """(records with redshift and wrapped phi, polar(...) of them)."""
    if name not in _REC:
        rays = np.ascontiguousarray(np.load(gc.golden_path(name))["final__rk4"])
        rec, _, _ = hr.with_redshift(rays, -SPIN)
        _REC[name] = rec, ss.polar(rec, -SPIN, INC_DEG)
    return _REC[name]


def thermal_model(ne=24, e_min=0.05, e_max=20.0, nr=200):
    """10 solar masses, 1e18 g/s, f_col 1.7, ne log energies over [e_min, e_max]."""
    r_isco = gc.r_isco()
    dr = (R_DISC / r_isco) ** (1.0 / nr)
    kt = api.thermal_kt_table(SPIN, r_isco, dr, nr, 10.0, 1e18)
    return capi.spectrum_model("thermal", e_min, math.exp(math.log(e_max / e_min) / ne), ne, log_e=True, r_isco=r_isco, r_disc=R_DISC, f_col=1.7, table_r_min=r_isco,
                               table_dr=dr, table_kt=kt)


def table_model(ne=20, nz=2, s_ne=80):
    """A cut-off power law per zone on a log grid from 0.05 to 500."""
    s_de = math.exp(math.log(500.0 / 0.05) / (s_ne - 1))
    e = 0.05 * s_de ** np.arange(s_ne)
    S = np.array([e ** -(1.6 + 0.2 * z) * np.exp(-e / 100.0) for z in range(nz)])
    return capi.spectrum_model("table", 0.5, math.exp(math.log(100.0 / 0.5) / ne), ne, log_e=True, r_isco=gc.r_isco(), r_disc=R_DISC, s=S, s_e_min=0.05, s_de=s_de, **EMIS)


MODELS = {"thermal": thermal_model, "table": table_model}


def spoilt(rec, m):
    """A copy with three disc records made bad-pol, the way test_hotspot_stokes_rules.spoilt does it: Q x 1e4 twice (mu > 1: bad-angle) and
    alpha = beta = NaN once (no observer)."""
    idx = np.flatnonzero(sr.disc_filter(m, rec))[[1, 7, 20]]
    out = rec.copy()
    out["Q"][idx[:2]] *= 1e4
    out["alpha"][idx[2]] = out["beta"][idx[2]] = np.nan
    return out, idx


def lit(res):
    return res["used"] > 30 and (np.abs(res["q"]).max() > 0 or np.abs(res["u"]).max() > 0)


@pytest.mark.parametrize("name", ["ip15", "ip16"])
@pytest.mark.parametrize("kind", sorted(MODELS))
@pytest.mark.parametrize("pol_law", [(0, 0.3), (0, -0.3), CHANDRA])
def test_the_polarised_flux_bounds_q_and_u(name, kind, pol_law):
    """hypot(Q, U) <= P per energy (|sum w (c2, s2)| <= sum |w| for unit vectors), and P <= |coeff|_max I (|delta| <= |coeff| for mu in [0, 1])."""
    rec, pol = records(name)
    res = ss.spectrum_stokes(MODELS[kind](), rec, pol, limb=LAOR, pol_law=pol_law)
    assert lit(res) and res["bad_pol"] == 0 and res["p"].max() > 0
    assert (np.hypot(res["q"], res["u"]) <= res["p"] * (1 + 1e-12)).all()
    assert res["delta_max"] <= abs(pol_law[1])
    assert (res["p"] <= abs(pol_law[1]) * res["flux"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("name", ["ip15", "ip16"])
@pytest.mark.parametrize("kind", sorted(MODELS))
@pytest.mark.parametrize("limb", sorted(LIMBS))
def test_no_degree_gives_the_spectrum_rule_without_the_bad_pol_records(name, kind, limb):
    """Law 0 with coeff = 0: Q = U = 0 exactly, and I is the kr_spectrum_model rule's flux on the records that are not bad-pol (to rounding: the two
    rules order the thermal products differently, the header says where).  The fixtures alone have no bad-pol disc record, so three are spoilt."""
    rec0, pol0 = records(name)
    m = MODELS[kind]()
    assert ss.spectrum_stokes(m, rec0, pol0, limb=LIMBS[limb], pol_law=CHANDRA)["bad_pol"] == 0
    rec, idx = spoilt(rec0, m)
    rec, _, _ = hr.with_redshift(rec, -SPIN)                  # the spoilt constants of motion move g
    pol = ss.polar(rec, -SPIN, INC_DEG)
    res = ss.spectrum_stokes(m, rec, pol, limb=LIMBS[limb], pol_law=(0, 0.0))
    assert res["used"] > 30 and res["flux"].max() > 0                                     # (Q = U = 0 is the claim here: the other half of lit() is below)
    assert lit(ss.spectrum_stokes(m, rec, pol, limb=LIMBS[limb], pol_law=CHANDRA))
    assert res["bad_pol"] == 3 and sorted(res["bad_index"]) == sorted(idx)
    assert not res["q"].any() and not res["u"].any() and not res["p"].any()
    keep = np.ones(len(rec), dtype=bool)
    keep[idx] = False
    plain = sr.spectrum(m, rec[keep], law=LIMBS[limb][0], coeff=LIMBS[limb][1], mu=pol["mu"][keep], bad=np.zeros(int(keep.sum()), dtype=bool))
    assert res["used"] == plain["used"] and res["on_disc"] == plain["on_disc"] + 3
    assert sr.rel_diff(res["flux"], plain["flux"]) <= 1e-13
    if kind == "table":
        assert np.array_equal(res["flux"], plain["flux"])                                   # the table's products come in the same order in both rules


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_linear_in_the_coefficient(kind):
    """Law 0: coeff = d gives d x the sums of coeff = 1 to rounding, and coeff -> -coeff flips Q and U exactly."""
    rec, pol = records("ip16")
    m = MODELS[kind]()
    one = ss.spectrum_stokes(m, rec, pol, limb=LAOR, pol_law=(0, 1.0))
    assert lit(one)
    for d in (0.3, 0.1171, -0.7):
        res = ss.spectrum_stokes(m, rec, pol, limb=LAOR, pol_law=(0, d))
        for k in ("q", "u"):
            assert np.abs(res[k] - d * one[k]).max() <= 1e-13 * one["p"].max()
        assert np.array_equal(res["flux"], one["flux"])
    for pol_law in ((0, 0.3), CHANDRA):
        a = ss.spectrum_stokes(m, rec, pol, limb=LAOR, pol_law=pol_law)
        b = ss.spectrum_stokes(m, rec, pol, limb=LAOR, pol_law=(pol_law[0], -1 * pol_law[1]))
        assert lit(a)
        assert np.array_equal(b["q"], -1 * a["q"]) and np.array_equal(b["u"], -1 * a["u"])
        assert np.array_equal(a["flux"], b["flux"]) and np.array_equal(a["p"], b["p"])


@pytest.mark.parametrize("name", ["ip15", "ip16"])
@pytest.mark.parametrize("limb", sorted(LIMBS))
def test_a_flat_table_gives_the_stokes_line_summed_over_energy(name, limb):
    """S = 1 on a grid that covers every g E_i: Q[i] and U[i] do not depend on i, and equal the energy sums of the Stokes line's Q and U planes for
    the same emissivity (weight emis g^-3) and limb law."""
    rec, pol = records(name)
    r_isco = gc.r_isco()
    m = capi.spectrum_model("table", 1.0, 0.5, 8, r_isco=r_isco, r_disc=R_DISC, s=np.ones(64), s_e_min=1e-3, s_de=1.3, **EMIS)
    g = rec["redshift"][sr.disc_filter(m, rec)]
    E = sr.energies(m)
    assert (g.min() * E >= 1e-3).all() and (g.max() * E <= sr.last_node(m)).all()
    res = ss.spectrum_stokes(m, rec, pol, limb=LIMBS[limb], pol_law=CHANDRA)
    assert lit(res)
    for k in ("flux", "q", "u", "p"):
        assert (res[k] == res[k][0]).all(), k
    b = capi.line_bins(line_energy=1.0, e_min=1e-3, de=1.2, ne=80, log_e=True, r_isco=r_isco, r_disc=R_DISC, g_index=3.0, **EMIS)
    line = pr.stokes_line_rule(b, LIMBS[limb], CHANDRA, rec, -SPIN, INC_DEG, g=rec["redshift"])
    assert line["binned"] == line["on_disc"] == res["used"]
    for k, plane in (("flux", "I"), ("q", "Q"), ("u", "U")):
        assert abs(res[k][0] - line[plane].sum()) <= 1e-12 * res["p" if k != "flux" else "flux"][0], k


@pytest.mark.parametrize("name,ratio,angle", [("ip15", 6.0, 2.4), ("ip16", 4.7, 2.8)])
def test_the_degree_falls_with_energy_and_the_soft_angle_lies_along_the_disc(name, ratio, angle):
    """Thermal, 24 log energies 0.05 ... 20 keV, Laor, Chandrasekhar: the hot inner disc, whose light dominates the hard end, is the most strongly lensed
    and dragged and so the least polarised.  degree[0] >= 3 degree[-1] (measured: 6.0 x on ip15, 4.7 x on ip16) and |angle[0]| < 5 degrees from the
    image's x axis (measured 2.4 and 2.8)."""
    rec, pol = records(name)
    res = ss.spectrum_stokes(thermal_model(), rec, pol, limb=LAOR, pol_law=CHANDRA)
    assert lit(res)
    degree, ang = ss.degree_angle(res)
    print(f"{name}: used {res['used']}; degree {100 * degree[0]:.2f} % at {res['energy'][0]:.3f} keV, {100 * degree[-1]:.2f} % at {res['energy'][-1]:.1f} keV "
          f"({degree[0] / degree[-1]:.1f} x); angle {math.degrees(ang[0]):.1f} -> {math.degrees(ang[-1]):.1f} degrees")
    assert degree[0] >= 3 * degree[-1]
    assert abs(math.degrees(ang[0])) < 5
    assert abs(degree[0] / degree[-1] - ratio) < 0.1 and abs(abs(math.degrees(ang[0])) - angle) < 0.1           # the figures the issue quotes


@pytest.mark.parametrize("name", ["ip15", "ip16"])
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_float64_against_longdouble_noise(name, kind):
    rec, pol = records(name)
    noise, lo, hi = ss.noise(MODELS[kind](), rec, pol, limb=LAOR, pol_law=CHANDRA)
    print(f"{name} {kind}: used {lo['used']}; float64 - longdouble: " + ", ".join(f"{k} {v:.2e}" for k, v in noise.items()))
    assert lit(lo) and all(v < 1e-12 for v in noise.values())
    if np.finfo(np.longdouble).nmant > 52:
        assert max(noise.values()) > 0


def test_words_layout_and_text():
    m = capi.spectrum_model("table", 1.0, 1.0, 3, s=np.ones(4), s_e_min=0.5, s_de=2.0)
    assert api.spectrum_stokes_words(m) == 13
    words = np.arange(13, dtype=np.float64)
    got = ss.from_words(m, words)
    assert got["flux"].tolist() == [0, 1, 2] and got["q"].tolist() == [3, 4, 5] and got["u"].tolist() == [6, 7, 8]
    assert (got["on_disc"], got["used"], got["bad_pol"]) == (9, 10, 11)
    res = api.spectrum_stokes_from_words(m, words)
    assert res["q"].tolist() == [3, 4, 5] and (res["on_disc"], res["used"], res["bad_pol"]) == (9, 10, 11) and "bad_angle" not in res
    assert np.isnan(res["pol_degree"][0]) and np.isnan(res["pol_angle"][0])                # flux == 0
    assert res["pol_degree"][1] == math.hypot(4, 7) / 1 and res["pol_angle"][2] == 0.5 * math.atan2(8, 5)
    assert np.array_equal(res["energy"], [1.5, 2.5, 3.5])
    text = api.spectrum_text(res).splitlines()
    assert text[2].split() == ["#", "BAD_POL", "11"] and len(text) == 6 and all(len(row) == 80 for row in text[3:])
    assert [float(v) for v in text[4].split()] == [2.5, 1.0, 4.0, 7.0]
    plain = api.spectrum_from_words(m, np.arange(7, dtype=np.float64))
    assert api.spectrum_text(plain).splitlines()[2].split() == ["#", "BAD_ANGLE", "5"] and len(api.spectrum_text(plain).splitlines()[3]) == 40
