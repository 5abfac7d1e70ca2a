"""CPU: the per-record rule of the disc-surface passes (tests/surface_pass_rules.py; include/kr_trace.h, kr_disc_surface) on the reference-pinned
records of rays landed on three surfaces (tests/golden/thick_disc/: spin 0.5, reverse 0) and on synthetic equatorial records.  No GPU.

The figures asserted here were measured with this rule in numpy: landed 2336 / 2406 / 2265 with no bad-angle record, mu within 0.036 ... 0.834,
0.040 ... 0.823 and 0.017 ... 0.818, |E^2 - P_r^2 - P_th^2 - P_phi^2| <= 1.4e-15 E^2.  rk4_thin is NOT tied to the flat rule: its records sit a step past
the equator, which the flat rule ignores (mu differs by up to 0.0097)."""
import numpy as np
import pytest

import angle_rules as ar
import surface_pass_rules as sp
import surface_rules as su
from raytrace_cpu_amd import capi

RUNS = {"rk4_s005_m1": (2336, 0.036, 0.834), "rk4_s01_m0": (2406, 0.040, 0.823), "rk4_thin": (2265, 0.017, 0.818)}
EPS = 2.0 ** -52


def surface(name):
    slope, scale, _ = su.RUNS[name]
    return (su.r_in(), su.R_OUT, slope, scale)


_RULE = {}


def rule(name):
    """(records, frame, angles, the records as a fused pass leaves them, the landed mask), once per run."""
    if name not in _RULE:
        rays = su.load_records(name)
        f = sp.frame(rays, su.SPIN, 0)
        an = sp.angles(rays, su.SPIN, 0, surface(name), f=f)
        rec = sp.records_after(rays, su.SPIN, 0)
        _RULE[name] = (rays, f, an, rec, sp.on_surface(rec, su.r_in(), su.R_OUT))
    return _RULE[name]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_landed_counts_and_no_bad_angle(name):
    rays, f, an, rec, on = rule(name)
    landed, mu_lo, mu_hi = RUNS[name]
    assert len(rays) == 5168 and int(on.sum()) == landed
    assert int((sp.bad_angle(f, an) & on).sum()) == 0
    mu = an["mu"][on]
    assert abs(mu.min() - mu_lo) < 5e-4 and abs(mu.max() - mu_hi) < 5e-4, (mu.min(), mu.max())
    assert (mu > 0).all() and (mu < 1).all() and np.isfinite(an["chi"][on]).all()
    # the redshift of the rule's frame is the one the reference stored after redshift(&disc), and the filter is the surface reducers'
    assert np.array_equal(on, su.landed(rays) & (sp.rho_of(rays) >= su.r_in()) & (sp.rho_of(rays) < su.R_OUT))
    np.testing.assert_allclose(rec["redshift"][on], rays["redshift"][on], rtol=8 * EPS, atol=0)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_normal_is_orthogonal_to_the_gas(name):
    """n = n_r e3 + n_th e2 against the gas four-velocity e_t, with the metric: zero, because e2 and e3 have no t and no phi component.  Also
    g(n, n) = -nn^2: e2, e3 are unit and orthogonal."""
    rays, f, an, rec, on = rule(name)
    n = [an["n_r"] * f["e3"][c] + an["n_th"] * f["e2"][c] for c in range(4)]
    dot = ar.dot_product(f["metric"], n, f["et"])
    assert np.array_equal(dot[on], np.zeros(int(on.sum())))
    norm = ar.dot_product(f["metric"], n, n)
    np.testing.assert_allclose(-norm[on], an["nn"][on] ** 2, rtol=8 * EPS, atol=0)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_rotation_keeps_the_poloidal_momentum(name):
    """(P_n, P_s) is (P_r, P_th) turned: P_n^2 + P_s^2 = P_r^2 + P_th^2 (a few ulp: two quotients by nn, four products, two sums on either side)."""
    rays, f, an, rec, on = rule(name)
    lhs, rhs = (an["P_n"] ** 2 + an["P_s"] ** 2)[on], (f["P_r"] ** 2 + f["P_th"] ** 2)[on]
    np.testing.assert_allclose(lhs, rhs, rtol=16 * EPS, atol=0)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_momentum_is_null_in_the_frame(name):
    """E^2 - P_r^2 - P_th^2 - P_phi^2 = 0 to rounding: measured 1.4e-15 of E^2; the bar is 16 ulp of E^2, the four squares and three sums of terms <= E^2
    each carrying the few ulp of their sixteen-term dot products."""
    rays, f, an, rec, on = rule(name)
    null = (f["E"] ** 2 - f["P_r"] ** 2 - f["P_th"] ** 2 - f["P_phi"] ** 2)[on] / f["E"][on] ** 2
    worst = float(np.abs(null).max())
    print(f"{name}: |E^2 - P^2| / E^2 <= {worst:.2e}")
    assert worst <= 16 * EPS
    # and mu^2 + (P_s^2 + P_phi^2) / E^2 = 1 likewise
    one = (an["mu"] ** 2 + (an["P_s"] ** 2 + f["P_phi"] ** 2) / f["E"] ** 2)[on]
    np.testing.assert_allclose(one, 1.0, rtol=0, atol=32 * EPS)


def test_thin_records_are_not_the_flat_rule():
    """The records of the thin run sit a step past the equator: the flat rule, which takes the equatorial normal there, is another number."""
    rays, f, an, rec, on = rule("rk4_thin")
    flat_mu, _ = ar.mu_chi(ar.frame(rays, su.SPIN, -1.0, 0, 1))
    worst = float(np.abs(flat_mu[on] - an["mu"][on]).max())
    print(f"rk4_thin: |mu - flat mu| <= {worst:.4f}")
    assert 1e-3 < worst < 2e-2


def synthetic_equatorial():
    """Records at theta = pi / 2 over a range of radii with the constants of motion of fixture records (so that the momentum is a photon's)."""
    src = su.load_records("rk4_thin")
    pick = src[su.landed(src)][:400]
    rays = np.array(pick, copy=True)
    rays["theta"] = np.pi / 2
    rays["r"] = np.linspace(4.5, 60.0, len(rays))
    return rays


@pytest.mark.parametrize("reverse", [0, 1])
def test_flat_limit_on_equatorial_records(reverse):
    """theta = pi / 2, slope = scale = 0: |P_th| / E and atan2(P_phi, P_r) of angle_rules.mu_chi.  cos(pi / 2) is 6.1e-17 in double, not 0: n_th = -1
    and nn = 1 exactly (rhosq = r^2, sqrt exact), and n_r = sqrt(delta) / r x 6.1e-17 leaks |n_r P_r| <= 6.2e-17 |P_r| into P_n and |n_r P_th| into
    P_s, i.e. at most half an ulp of E each before rounding: mu within 2 ulp of 1, chi within 4 ulp of pi."""
    rays = synthetic_equatorial()
    f = sp.frame(rays, su.SPIN, reverse)
    an = sp.angles(rays, su.SPIN, reverse, (su.r_in(), su.R_OUT, 0.0, 0.0), f=f)
    flat = ar.frame(rays, su.SPIN, -1.0, reverse, 1)
    for k in ("E", "P_r", "P_th", "P_phi"):
        assert np.array_equal(f[k], flat[k]), k                                          # the same frame, to the bit
    mu, chi = ar.mu_chi(flat)
    assert np.isfinite(mu).all() and (an["Hp"] == 0).all() and (an["nn"] == 1).all() and (an["n_th"] == -1).all()
    assert float(np.abs(an["mu"] - mu).max()) <= 2 * EPS
    assert float(np.abs(an["chi"] - chi).max()) <= 4 * np.pi * EPS
    # and below the plane (theta a hair beyond pi / 2 changes sg, not the angles)
    assert not sp.bad_angle(f, an).any()


def test_bad_angle_adds_the_normal():
    """nn zero or not finite is bad-angle beside frame_bad_angle's tests; steps <= 0 is never judged."""
    rays = synthetic_equatorial()[:4]
    f = sp.frame(rays, su.SPIN, 0)
    an = sp.angles(rays, su.SPIN, 0, (su.r_in(), su.R_OUT, 0.1, 1.0), f=f)
    assert not sp.bad_angle(f, an).any()
    for v in (0.0, np.inf, np.nan):
        broken = dict(an, nn=np.where(np.arange(4) == 1, v, an["nn"]))
        assert sp.bad_angle(f, broken).tolist() == [False, True, False, False]
    big = dict(an, mu=np.where(np.arange(4) == 2, 1.5, an["mu"]))
    assert sp.bad_angle(f, big).tolist() == [False, False, True, False]
    dead = np.array(rays, copy=True)
    dead["steps"][0] = 0
    fd = sp.frame(dead, su.SPIN, 0)
    ad = sp.angles(dead, su.SPIN, 0, (su.r_in(), su.R_OUT, 0.1, 1.0), f=fd)
    assert np.isnan(ad["mu"][0]) and np.isnan(ad["chi"][0]) and not sp.bad_angle(fd, ad)[0]


def test_flat_equivalent_carries_the_surface_filter():
    """What the flat rules' filter sees of flat_equivalent(records) is the surface filter on the records."""
    import line_rules as lr
    rays, f, an, rec, on = rule("rk4_s005_m1")
    b = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=su.r_in(), r_disc=30.0)
    flat = sp.flat_equivalent(rec)
    assert np.array_equal(lr.disc_filter(b, flat), sp.on_surface(rec, su.r_in(), 30.0))
    assert 0 < sp.on_surface(rec, su.r_in(), 30.0).sum() < on.sum()
    assert np.array_equal(flat["t"], rec["t"]) and np.array_equal(flat["r"][on], sp.rho_of(rec)[on])
