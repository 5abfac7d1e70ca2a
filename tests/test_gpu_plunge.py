"""GPU: the disc flow "Keplerian, plunging inside the ISCO" (V = capi.V_PLUNGE, include/kr_trace.h) in every pass that takes it, against the numpy rule
of tests/plunge_rules.py -- never against the device itself -- and against the V = -1 pass where the two must agree to the bit.

Records: the fixtures' final__rk4_flatdisc of ps_h5_a05 and ps_h10_a0 (2604 each, 436 and 249 inside the ISCO, reverse = 0) pushed to the device, and one
33 x 33 image plane traced on the device through the api (a = 0.5, 60 degrees, x, y in [-8, 8], distance 1000, RK4 to the theta limit, reverse = 1).

Bars: 1e-12 absolute on mu and chi and relative on the redshift and on sums, the bars of tests/test_gpu_angles.py.  Near Delta -> 0 the rule's own float64
rounding exceeds that, so a bar is max(16 x noise, 1e-12) with noise = |the float64 rule - the same rule in np.longdouble| on those records (for a sum: the
sum's rule fed the float64 redshift against the same rule fed the longdouble one), the convention of the response tests.  The emissivity and image
reducers keep the bar of their own tests (parity.BIN_RTOL), the spectrum and the response theirs (max(16 x noise, floor) of their rules).  The worst
margins are recorded with parity.record_margin, which the session writes out with the suite's other margins (a copy: profiles/plunge_parity.json)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import angle_rules as ar
import golden_cases as gc
import line_rules as lr
import oracle_lib as ol
import parity
import plunge_rules as pr
import reducer_rules as rr
import test_gpu_angles as tga
import test_gpu_disc_spectrum as ds
import test_gpu_reducers as tgr
import test_gpu_reverb_response as rv
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi
VP = capi.V_PLUNGE
FLOOR = 1e-12
R_DISC = 30.0


def note(name, **extra):
    parity.record_margin("test_gpu_plunge", name, {"n_traced": 0, "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(extra.get("worst", 0.0))}, **extra)


def margin(name, worst, allowed, **extra):
    note(name, worst=float(worst), allowed=float(allowed), **extra)
    print(f"{name}: worst {worst:.3e}, allowed {allowed:.3e} {extra}")
    assert worst <= allowed, (name, worst, allowed)


def plane_spec():
    return ol.imageplane_spec(1000.0, 60.0, -8.0, 8.0, 0.5, -8.0, 8.0, 0.5, 0.5)


def plane_params():
    p = capi.default_params(-0.5)
    p.precision, p.integrator, p.theta_max, p.r_max = 100.0, capi.RK4, PI / 2, 1100.0
    p.stop_kind, p.flags = capi.STOP_THETA, capi.FLAG_HYBRID
    return p


_RECORDS = {}


def records(name):
    """(records that have not been through a V_PLUNGE pass, spin as the pass takes it, reverse).  The plane's come back from the api after a V = -1
    pass that rewrote only redshift and phi, which every pass under test computes again from the fields it left alone."""
    if name not in _RECORDS:
        if name == "plane":
            m = ds.table_model(ne=4)
            res = api.disc_spectrum(plane_spec(), plane_params(), m, return_records=True)
            assert len(res["records"]) == 33 * 33
            _RECORDS[name] = (np.ascontiguousarray(res["records"]), -0.5, 1)
        else:
            case = {"a05": "ps_h5_a05", "a0": "ps_h10_a0"}[name]
            c = gc.cases()[case]
            _RECORDS[name] = (np.ascontiguousarray(np.load(gc.golden_path(case))["final__rk4_flatdisc"]), c["runs"]["rk4_flatdisc"].spin, 0)
    return _RECORDS[name]


def metric_spin(name):
    _, spin, reverse = records(name)
    return -spin if reverse else spin


def r_in(name):
    """the programs' default inner edge with plunge = 1: 1.02 x the horizon radius"""
    return 1.02 * api.lib().kr_kerr_horizon(metric_spin(name))


def inside(name):
    """on the plane (steps > 0, |z| < 1e-2) and inside r_ms"""
    rays, spin, reverse = records(name)
    return pr.inside(rays, spin, reverse) & ar.disc_filter(rays, 0.0, 1e9)


_RULE = {}


def rule(name):
    """The float64 rule on the records, once: frame, mu, chi, bad-angle, redshift, the records as a V_PLUNGE pass leaves them (redshift, wrapped phi), the
    same records with the longdouble rule's redshift, and the noise of g, mu, chi."""
    if name not in _RULE:
        rays, spin, reverse = records(name)
        f = pr.frame(rays, spin, VP, reverse, 0)
        mu, chi = ar.mu_chi(f)
        g = pr.redshift_rule(rays, spin, VP, reverse)
        rec = rays.copy()
        rec["redshift"] = g
        rec["phi"] = rr.range_phi(rays["phi"], rays["steps"])
        rec_hi = rec.copy()
        ins = pr.inside(rays, spin, reverse)
        rec_hi["redshift"][ins] = pr.redshift_rule(rays[ins], spin, VP, reverse, dtype=np.longdouble).astype(np.float64)
        _RULE[name] = dict(f=f, mu=mu, chi=chi, bad=ar.bad_angle(f), g=g, rec=rec, rec_hi=rec_hi, noise=pr.noise(rays, spin, reverse))
    return _RULE[name]


def bar(noise):
    return max(16 * float(noise), FLOOR)


def same_words(x, y):
    """Two launches over more than one wave add their floating sums with atomics in an order that differs from launch to launch, so two results of the
    SAME pass on the same records agree in every count and tally and in the zero pattern, and in the sums to rounding: 1e-12 relative, the bar on sums."""
    return tga.flux_rel(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)) <= 1e-12


def doubled(twice, once):
    return same_words(twice, 2 * np.asarray(once))


def dev_redshift(rays, spin, V, reverse):
    L = api.lib()
    with DeviceScope(L) as dev:
        d = dev.upload(rays)
        capi.check(L, L.kr_redshift_dev_f64(spin, V, reverse, 0, 0, d, len(rays), None), "kr_redshift_dev")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(d, len(rays), rays.dtype)


# ---- the precondition of the image-plane cases ------------------------------------------------------------------------------------------------
def test_plane_has_rays_inside_the_isco(krlib):
    n = int(inside("plane").sum())
    print(f"plane: {n} of {33 * 33} rays end on the plane inside the ISCO")
    assert n >= 100
    assert int(inside("a05").sum()) == 436 and int(inside("a0").sum()) == 249


# ---- the redshift pass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a05", "a0", "plane"])
def test_redshift_pass(krlib, name):
    rays, spin, reverse = records(name)
    kep, got = dev_redshift(rays, spin, -1.0, reverse), dev_redshift(rays, spin, VP, reverse)
    ins = pr.inside(rays, spin, reverse) & (rays["steps"] > 0)
    assert got[~ins].tobytes() == kep[~ins].tobytes()                                      # r >= r_ms or steps <= 0: the V = -1 pass, byte for byte
    for field in rays.dtype.names:
        if field != "redshift":
            assert got[field].tobytes() == rays[field].tobytes(), field                   # only `redshift` is written
    want = rule(name)["g"]
    assert np.array_equal(np.isnan(got["redshift"][ins]), np.isnan(want[ins]))
    fin = ins & np.isfinite(want)
    assert fin.sum() >= 100 and not np.array_equal(got["redshift"][fin], kep["redshift"][fin])
    worst = float((np.abs(got["redshift"] - want)[fin] / np.abs(want[fin])).max())
    margin(f"redshift/{name}", worst, bar(rule(name)["noise"]["g"].max()), records=int(fin.sum()), noise=float(rule(name)["noise"]["g"].max()))
    # the host-array form: the same kernel
    host = rays.copy()
    api.redshift(spin, VP, reverse, 0, host)
    assert host.tobytes() == got.tobytes()


# ---- the angles pass --------------------------------------------------------------------------------------------------------------------------
def check_angles(name, sl=slice(None)):
    rays, spin, reverse = records(name)
    part = np.ascontiguousarray(rays[sl])
    R = rule(name)
    want_mu, want_chi, want_bad = R["mu"][sl], R["chi"][sl], R["bad"][sl]
    mu, chi, after = tga.dev_angles(part, spin, VP, reverse, 0)
    assert after.tobytes() == part.tobytes()                                              # read-only
    assert np.array_equal(np.isnan(mu), np.isnan(want_mu)) and np.array_equal(np.isnan(chi), np.isnan(want_chi))
    assert np.isnan(mu[part["steps"] <= 0]).all() and np.isnan(chi[part["steps"] <= 0]).all()
    with np.errstate(invalid="ignore"):
        bad = (part["steps"] > 0) & (~np.isfinite(mu) | (mu > 1) | np.signbit(mu))       # E <= 0 shows as a mu that is negative, -0 or not finite
    assert np.array_equal(bad, want_bad)
    inf = np.isinf(want_mu)
    assert np.array_equal(mu[inf], want_mu[inf])
    fin = np.isfinite(want_mu) & np.isfinite(want_chi)
    worst_mu, worst_chi = float(np.abs(mu - want_mu)[fin].max()), float(np.abs(chi - want_chi)[fin].max())
    return mu, chi, part, worst_mu, worst_chi, int(fin.sum())


@pytest.mark.parametrize("name", ["a05", "a0", "plane"])
def test_angles_pass(krlib, name):
    rays, spin, reverse = records(name)
    mu, chi, _, worst_mu, worst_chi, n = check_angles(name)
    noise = rule(name)["noise"]
    margin(f"angles-mu/{name}", worst_mu, bar(noise["mu"].max()), records=n, noise=float(noise["mu"].max()))
    margin(f"angles-chi/{name}", worst_chi, bar(noise["chi"].max()), records=n, noise=float(noise["chi"].max()))
    # outside r_ms the V = -1 pass, byte for byte; inside another frame
    k_mu, k_chi, _ = tga.dev_angles(rays, spin, -1.0, reverse, 0)
    out = ~pr.inside(rays, spin, reverse)
    assert mu[out].tobytes() == k_mu[out].tobytes() and chi[out].tobytes() == k_chi[out].tobytes()
    ins = inside(name)
    assert not np.array_equal(chi[ins], k_chi[ins])


@pytest.mark.parametrize("n", [0, 1, 257])
def test_angles_at_the_edges_of_a_workgroup(krlib, n):
    rays, spin, reverse = records("a05")
    ins = inside("a05")
    first = next(int(i) for i in np.flatnonzero(ins) if i + 257 <= len(rays))              # a slice whose first record is inside the ISCO
    if n == 0:
        L = api.lib()
        with DeviceScope(L) as dev:
            a = dev.upload(np.full(4, 7.0))
            capi.check(L, L.kr_angles_dev_f64(spin, VP, reverse, 0, 0, None, 0, a, None), "kr_angles_dev")
            assert (dev.fetch(a, 4) == 7.0).all()
        mu, chi = api.arrival_angles(rays[:0].copy(), spin, VP, reverse, 0)
        assert len(mu) == 0 and len(chi) == 0
        return
    mu, chi, part, worst_mu, worst_chi, _ = check_angles("a05", slice(first, first + n))
    noise = rule("a05")["noise"]
    assert len(mu) == n and np.isfinite(mu[0]) and worst_mu <= bar(noise["mu"].max()) and worst_chi <= bar(noise["chi"].max())
    h_mu, h_chi = api.arrival_angles(part, spin, VP, reverse, 0)                           # the host-array form, and the api on device records
    with DeviceScope(api.lib()) as dev:
        d_mu, d_chi = api.arrival_angles((dev.upload(part), n), spin, VP, reverse, 0)
    for got in (h_mu, d_mu):
        assert got.tobytes() == np.ascontiguousarray(mu).tobytes()
    for got in (h_chi, d_chi):
        assert got.tobytes() == np.ascontiguousarray(chi).tobytes()


# ---- the line, plain and limb-darkened --------------------------------------------------------------------------------------------------------
def line_bins(name, r_isco):
    # a logarithmic axis wide enough for every g of the fixtures (lamp post -> disc) and of the plane
    return capi.line_bins(line_energy=6.4, e_min=0.05, de=1.1, ne=120, log_e=True, r_isco=r_isco, r_disc=R_DISC, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0)


def line_rule(name, b, law_id, coeff, rec):
    rays, spin, reverse = records(name)
    return pr.line_limb_rule(b, law_id, coeff, rays, spin, VP, reverse, 0, g=rec["redshift"])


@pytest.mark.parametrize("name", ["a05", "plane"])
def test_line_with_and_without_limb_law(krlib, name):
    rays, spin, reverse = records(name)
    R = rule(name)
    post = (VP, reverse, 0)
    b = line_bins(name, r_in(name))
    plain, plain_rays = tga.plain_line(b, rays, spin, post)
    # the records: redshift of the redshift pass, phi wrapped, nothing else
    assert plain_rays["redshift"].tobytes() == dev_redshift(rays, spin, VP, reverse)["redshift"].tobytes()
    want_all, want_in = line_rule(name, b, 0, 0.0, R["rec"]), None
    only_inside = rays.copy()
    only_inside["steps"] = np.where(inside(name), rays["steps"], 0)
    for law_name, (law_id, coeff) in capi.LIMB_LAWS.items():
        law = capi.limb_law((law_id, coeff))
        got, after = tga.limb_line(b, law, rays, spin, post)
        assert after.tobytes() == plain_rays.tobytes(), law_name
        want = line_rule(name, b, law_id, coeff, R["rec"])
        assert (got["on_disc"], got["binned"], got["bad_angle"]) == (want["on_disc"], want["binned"], want["bad_angle"]), law_name
        assert np.array_equal(got["count"], want["count"]), law_name
        hi = line_rule(name, b, law_id, coeff, R["rec_hi"])
        assert np.array_equal(hi["count"], want["count"])
        margin(f"line-{law_name}/{name}", tga.flux_rel(got["flux"], want["flux"]), bar(tga.flux_rel(want["flux"], hi["flux"])), binned=int(got["binned"]))
        twice, _ = tga.limb_line(b, law, rays, spin, post, calls=2)
        assert doubled(twice["words"], got["words"]), law_name                              # the call adds
        if law_id == 0:
            assert np.array_equal(plain["count"], got["count"]) and (plain["on_disc"], plain["binned"]) == (got["on_disc"], got["binned"])
            assert tga.flux_rel(plain["flux"], want["flux"]) <= bar(tga.flux_rel(want["flux"], hi["flux"]))
    # at least one populated bin holds rays from inside the ISCO alone
    sub = R["rec"].copy()
    sub["steps"] = only_inside["steps"]
    want_in = lr.line_from_rays(b, sub)
    assert ((want_in["count"] > 0) & (want_in["count"] == want_all["count"])).any()
    assert want_all["on_disc"] > line_rule(name, line_bins(name, pr.r_ms(metric_spin(name))), 0, 0.0, R["rec"])["on_disc"]
    # fused == the redshift pass followed by the reduce form
    L = api.lib()
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(api.line_words(b) * 8)
        capi.check(L, L.kr_redshift_dev_f64(spin, VP, reverse, 0, 0, d, len(rays), None), "kr_redshift_dev")
        capi.check(L, L.kr_range_phi_dev_f64(-PI, PI, d, len(rays), None), "kr_range_phi_dev")
        capi.check(L, L.kr_reduce_line_dev_f64(C.byref(b), d, len(rays), h, None), "kr_reduce_line_dev")
        two, two_rays = api.line_from_words(b, dev.fetch(h, api.line_words(b))), dev.fetch(d, len(rays), rays.dtype)
    assert two_rays.tobytes() == plain_rays.tobytes()
    assert np.array_equal(two["count"], plain["count"]) and (two["on_disc"], two["binned"]) == (plain["on_disc"], plain["binned"])
    assert tga.flux_rel(two["flux"], plain["flux"]) <= 1e-12


def every_pass(name, rays, V, r_isco):
    """The output words of every pass that takes the flow, on `rays` with the inner edge r_isco, and the records the line pass leaves."""
    _, spin, reverse = records(name)
    L = api.lib()
    post = (V, reverse, 0)
    b = line_bins(name, r_isco)
    plain, after = tga.plain_line(b, rays, spin, post)
    limb, _ = tga.limb_line(b, capi.limb_law("laor"), rays, spin, post)
    h_plain, h_mu, m_words, _, _ = tga.run_emissivity_mu(emis_bins(name, r_isco), 5, rays, spin, post)
    ib = image_bins(r_isco)
    with DeviceScope(L) as dev:
        d, pl = dev.upload(rays), dev.zeros(api.image_words(ib) * 8)
        capi.check(L, L.kr_post_image_dev_f64(spin, V, reverse, 0, 0, -PI, PI, C.byref(ib), d, len(rays), pl, None), "kr_post_image")
        img = dev.fetch(pl, api.image_words(ib))
    s_words, _ = spectrum_fused(spectrum_model(r_isco), (1, 2.06), rays, spin, V, reverse)
    r_words, _ = response_fused(response_model(name, r_isco), (1, 2.06), rays, spin, V, reverse)
    words = [plain["count"], plain["flux"], limb["words"], h_plain, h_mu, m_words, img, s_words, r_words]
    # every count and tally word of those buffers, by the layouts of include/kr_trace.h
    nb, nr, npix = b.nt * b.ne, 30, ib.img_nx * ib.img_ny
    counts = [plain["count"], np.array([plain["on_disc"], plain["binned"]]), limb["words"][:nb], limb["words"][-3:], h_plain[:nr], h_plain[-1:], h_mu[:nr], h_mu[-1:],
              m_words[:nr * 5], m_words[-3:], img[:npix], img[-1:], s_words[-4:], r_words[-4:]]
    return words, after, [np.ascontiguousarray(c, dtype=np.float64) for c in counts]


@pytest.mark.parametrize("name", ["a05", "plane"])
def test_inner_edge_at_r_ms_gives_the_keplerian_words(krlib, name):
    """r_isco = r_ms: no record inside r_ms is binned, so the output words of a V_PLUNGE pass are the V = -1 pass's.  Byte for byte where the order of
    the additions is defined -- one wave of records, the first of them inside the ISCO -- and as same_words() has it on all the records."""
    rays, spin, reverse = records(name)
    rm = pr.r_ms(metric_spin(name))
    first = int(np.flatnonzero(inside(name))[0])
    wave = np.ascontiguousarray(rays[first:first + 64])
    assert len(wave) == 64 and (~pr.inside(wave, spin, reverse)).any()
    kep, _, _ = every_pass(name, wave, -1.0, rm)
    plunge, _, _ = every_pass(name, wave, VP, rm)
    for x, y in zip(kep, plunge):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    kep, kep_rays, kep_counts = every_pass(name, rays, -1.0, rm)
    plunge, plunge_rays, plunge_counts = every_pass(name, rays, VP, rm)
    for x, y in zip(kep_counts, plunge_counts):
        assert x.tobytes() == y.tobytes()                                                   # every count and tally word, byte for byte
    for x, y in zip(kep, plunge):
        assert same_words(x, y)
    assert kep[0].sum() > 100
    out = ~pr.inside(rays, spin, reverse)
    assert kep_rays[out].tobytes() == plunge_rays[out].tobytes()


# ---- emissivity, emissivity by angle, image ---------------------------------------------------------------------------------------------------
def emis_bins(name, r_isco, nr=30):
    b = capi.EmisBins()
    b.r_isco = b.r_min = r_isco
    b.dr = float(np.exp(np.log(500.0 / b.r_min) / nr))
    b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = 2.0, metric_spin(name), 2604.0, nr, 1
    return b


def image_bins(r_isco):
    ib = capi.ImageBins()
    ib.x0 = ib.y0 = -8.25
    ib.img_dx = ib.img_dy = 0.5
    ib.r_isco, ib.r_disc = r_isco, R_DISC
    ib.q1, ib.rb1, ib.q2, ib.rb2, ib.q3 = 3.0, 4.0, 3.0, 10.0, 3.0
    ib.img_nx = ib.img_ny = 33
    ib.flip_image = 1
    return ib


@pytest.mark.parametrize("name", ["a05", "a0"])
def test_emissivity_and_emissivity_by_angle(krlib, name):
    rays, spin, reverse = records(name)
    R = rule(name)
    b = emis_bins(name, r_in(name))
    post = (VP, reverse, 0)
    h_plain, h_mu, m_words, rays_plain, rays_mu = tga.run_emissivity_mu(b, 5, rays, spin, post)
    assert rays_mu.tobytes() == rays_plain.tobytes() == dev_redshift_and_phi(rays, spin, reverse).tobytes()
    hist_want, want = pr.emissivity_mu_rule(b, 5, rays, spin, VP, reverse, 0, g=R["rec"]["redshift"])
    got_plain, got_hist = tga.hist_dict(h_plain, b.nr), tga.hist_dict(h_mu, b.nr)
    for g in (got_plain, got_hist):
        rr.check_reduction(g, hist_want, "count", rr.EMIS_SUMS, parity.BIN_RTOL, name)
    got = ar.mu_from_words(b.nr, 5, m_words)
    assert np.array_equal(got["count2"], want["count2"])
    assert (got["disc_count"], got["binned"], got["bad_angle"]) == (want["disc_count"], want["binned"], want["bad_angle"])
    _, hi = pr.emissivity_mu_rule(b, 5, rays, spin, VP, reverse, 0, g=R["rec_hi"]["redshift"])
    noise = max(tga.flux_rel(want["flux2"], hi["flux2"]), float(R["noise"]["mu"].max()))
    margin(f"emissivity-mu/{name}", max(tga.flux_rel(got["flux2"], want["flux2"]), tga.flux_rel(got["sum_mu"], want["sum_mu"])), bar(noise), binned=got["binned"])
    # radial bins that lie wholly inside the ISCO are populated
    edges = b.r_min * b.dr ** np.arange(b.nr + 1)
    wholly = edges[1:] <= pr.r_ms(metric_spin(name))
    assert wholly.any() and (got_plain["count"][wholly] > 0).any() and (got["count2"].sum(axis=1)[wholly] > 0).any()
    # additivity, and the two-pass route
    L = api.lib()
    nh = 5 * b.nr + 1
    with DeviceScope(L) as dev:
        h2 = dev.zeros(nh * 8)
        for _ in range(2):
            d = dev.upload(rays)
            capi.check(L, L.kr_post_emissivity_dev_f64(spin, VP, reverse, 0, 0, -PI, PI, C.byref(b), d, len(rays), h2, None), "kr_post_emissivity")
        twice = dev.fetch(h2, nh)
        d, h3 = dev.upload(rays), dev.zeros(nh * 8)
        capi.check(L, L.kr_range_phi_dev_f64(-PI, PI, d, len(rays), None), "kr_range_phi_dev")
        capi.check(L, L.kr_redshift_dev_f64(spin, VP, reverse, 0, 0, d, len(rays), None), "kr_redshift_dev")
        capi.check(L, L.kr_reduce_emissivity_dev_f64(C.byref(b), d, len(rays), h3, None), "kr_reduce_emissivity_dev")
        two = dev.fetch(h3, nh)
    assert doubled(twice, h_plain)
    two = tga.hist_dict(two, b.nr)
    assert np.array_equal(two["count"], got_plain["count"]) and two["disc_count"] == got_plain["disc_count"]
    assert max(tga.flux_rel(two[k], got_plain[k]) for k in rr.EMIS_SUMS) <= 1e-12


def dev_redshift_and_phi(rays, spin, reverse):
    L = api.lib()
    with DeviceScope(L) as dev:
        d = dev.upload(rays)
        capi.check(L, L.kr_redshift_dev_f64(spin, VP, reverse, 0, 0, d, len(rays), None), "kr_redshift_dev")
        capi.check(L, L.kr_range_phi_dev_f64(-PI, PI, d, len(rays), None), "kr_range_phi_dev")
        return dev.fetch(d, len(rays), rays.dtype)


def test_image(krlib):
    name = "plane"
    rays, spin, reverse = records(name)
    R = rule(name)
    ib = image_bins(r_in(name))
    L = api.lib()
    nw = api.image_words(ib)
    with DeviceScope(L) as dev:
        d, pl, pl2 = dev.upload(rays), dev.zeros(nw * 8), dev.zeros(nw * 8)
        capi.check(L, L.kr_post_image_dev_f64(spin, VP, reverse, 0, 0, -PI, PI, C.byref(ib), d, len(rays), pl, None), "kr_post_image")
        after, words = dev.fetch(d, len(rays), rays.dtype), dev.fetch(pl, nw)
        for _ in range(2):
            d2 = dev.upload(rays)
            capi.check(L, L.kr_post_image_dev_f64(spin, VP, reverse, 0, 0, -PI, PI, C.byref(ib), d2, len(rays), pl2, None), "kr_post_image")
        twice = dev.fetch(pl2, nw)
        d3, pl3 = dev.upload(rays), dev.zeros(nw * 8)
        capi.check(L, L.kr_redshift_dev_f64(spin, VP, reverse, 0, 0, d3, len(rays), None), "kr_redshift_dev")
        capi.check(L, L.kr_range_phi_dev_f64(-PI, PI, d3, len(rays), None), "kr_range_phi_dev")
        capi.check(L, L.kr_reduce_image_dev_f64(C.byref(ib), d3, len(rays), pl3, None), "kr_reduce_image_dev")
        two = dev.fetch(pl3, nw)
    assert after.tobytes() == dev_redshift_and_phi(rays, spin, reverse).tobytes()
    want = rr.reduce_image(ib, R["rec"])
    got = tgr.image_dict(words, ib)
    worst = rr.check_reduction(got, want, "nrays", rr.IMAGE_SUMS, parity.BIN_RTOL, name)
    note("image/plane", worst=float(worst), allowed=parity.BIN_RTOL, counted=int(want["disc_count"]))
    assert got["disc_count"] == want["disc_count"]
    # one ray per pixel: the pixels of rays inside the ISCO are populated by them alone
    sub = R["rec"].copy()
    sub["steps"] = np.where(inside(name), sub["steps"], 0)
    only = rr.reduce_image(ib, sub)
    assert ((only["nrays"] > 0) & (only["nrays"] == want["nrays"])).sum() >= 50
    assert doubled(twice, words)
    two = tgr.image_dict(two, ib)
    assert np.array_equal(two["nrays"], got["nrays"]) and two["disc_count"] == got["disc_count"]
    assert max(tga.flux_rel(two[k], got[k]) for k in rr.IMAGE_SUMS) <= 1e-12


# ---- spectrum (table kind) and response -------------------------------------------------------------------------------------------------------
def spectrum_model(r_isco, ne=96):
    m = ds.table_model(ne=ne, e_min=0.05, e_max=100.0)
    m.r_isco, m.r_disc = r_isco, R_DISC
    return m


def response_model(name, r_isco, nt=60):
    rec = rule(name)["rec"]
    on = ar.disc_filter(rec, r_isco, R_DISC)
    t0 = math.floor(float(rec["t"][on].min())) - 2.25
    R = capi.response_model(spectrum_model(r_isco), t0, 1.0, nt)
    return R


def spectrum_fused(m, law, rays, spin, V, reverse, calls=1):
    L = api.lib()
    law = capi.limb_law(law)
    nw = api.spectrum_words(m)
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        for _ in range(calls):
            d = dev.upload(rays)
            capi.check(L, L.kr_post_spectrum_dev_f64(spin, V, reverse, 0, 0, -PI, PI, C.byref(m), C.byref(law), d, len(rays), h, None), "kr_post_spectrum")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(h, nw), dev.fetch(d, len(rays), rays.dtype)


def response_fused(R, law, rays, spin, V, reverse, calls=1):
    L = api.lib()
    law = capi.limb_law(law)
    nw = api.response_words(R)
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        for _ in range(calls):
            d = dev.upload(rays)
            capi.check(L, L.kr_post_response_dev_f64(spin, V, reverse, 0, 0, -PI, PI, C.byref(R), C.byref(law), d, len(rays), h, None), "kr_post_response")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(h, nw), dev.fetch(d, len(rays), rays.dtype)


def test_spectrum_table_kind(krlib):
    name = "plane"
    rays, spin, reverse = records(name)
    R = rule(name)
    m = spectrum_model(r_in(name))
    law = (1, 2.06)
    words, after = spectrum_fused(m, law, rays, spin, VP, reverse)
    assert after.tobytes() == dev_redshift_and_phi(rays, spin, reverse).tobytes()
    ds.against_the_rule("test_gpu_plunge", "spectrum-table-fused-laor", m, words, R["rec"], law, R["mu"], R["bad"])
    got = api.spectrum_from_words(m, words)
    kep_edge = spectrum_model(pr.r_ms(metric_spin(name)))
    assert got["on_disc"] >= 100 + api.spectrum_from_words(kep_edge, spectrum_fused(kep_edge, law, rays, spin, VP, reverse)[0])["on_disc"]
    twice, _ = spectrum_fused(m, law, rays, spin, VP, reverse, calls=2)
    assert doubled(twice, words)
    # the two-pass route: the isotropic fused pass against the redshift pass + the reduce form
    iso, _ = spectrum_fused(m, (0, 0.0), rays, spin, VP, reverse)
    two, _ = ds.reduced(m, dev_redshift_and_phi(rays, spin, reverse))
    assert np.array_equal(iso[-4:-2], two[-4:-2]) and ds.sr.rel_diff(iso[:m.ne], two[:m.ne]) <= 1e-12
    note("spectrum/plane", used=int(got["used"]), on_disc=int(got["on_disc"]))


def test_response(krlib):
    name = "plane"
    rays, spin, reverse = records(name)
    Rl = rule(name)
    R = response_model(name, r_in(name))
    law = (1, 2.06)
    words, after = response_fused(R, law, rays, spin, VP, reverse)
    assert after.tobytes() == dev_redshift_and_phi(rays, spin, reverse).tobytes()
    lo = rv.against_the_rule("test_gpu_plunge", "response-fused-laor", R, words, Rl["rec"], law, Rl["mu"], Rl["bad"])
    assert lo["used"] > 100
    # at least one populated time row is reached by rays from inside the ISCO alone: every cell of it lies wholly inside
    row, ins = np.full(len(rays), -1), inside(name)
    row[np.asarray(lo["used_index"])] = np.asarray(lo["row"])
    rows_in, rows_out = set(row[(row >= 0) & ins].tolist()), set(row[(row >= 0) & ~ins].tolist())
    print(f"response: rows reached from inside the ISCO {len(rows_in)}, of which from inside alone {len(rows_in - rows_out)}")
    assert len(rows_in - rows_out) >= 1
    got_resp = api.response_from_words(R, words)["resp"]
    assert all((got_resp[j] != 0).any() for j in rows_in - rows_out)
    twice, _ = response_fused(R, law, rays, spin, VP, reverse, calls=2)
    assert doubled(twice, words)
    iso, _ = response_fused(R, (0, 0.0), rays, spin, VP, reverse)
    two, _ = rv.reduced(R, dev_redshift_and_phi(rays, spin, reverse))
    assert np.array_equal(iso[-4:], two[-4:]) and ds.sr.rel_diff(iso[:-4], two[:-4]) <= 1e-12
    note("response/plane", used=int(lo["used"]), outside=int(lo["outside"]))


# ---- the api --------------------------------------------------------------------------------------------------------------------------------------
def test_api_takes_the_flow(krlib):
    spec, p = plane_spec(), plane_params()
    name = "plane"
    rays, spin, reverse = records(name)
    b = line_bins(name, r_in(name))
    got = api.line_profile(spec, p, b, limb="laor", V=VP)
    want, _ = tga.limb_line(b, capi.limb_law("laor"), rays, spin, (VP, reverse, 0))
    assert got["binned"] > 100 and np.array_equal(got["count"], want["count"]) and got["bad_angle"] == want["bad_angle"]
    np.testing.assert_allclose(got["flux"], want["flux"], rtol=1e-12, atol=0)
    kep = api.line_profile(spec, p, b, limb="laor")
    assert not np.array_equal(kep["flux"], got["flux"])
    plain = api.line_profile(spec, p, b, V=VP)
    assert np.array_equal(plain["count"], tga.plain_line(b, rays, spin, (VP, reverse, 0))[0]["count"])
    pix = api.line_profile(spec, p, b, mode="pixels", image_bins=image_bins(r_in(name)), V=VP)
    assert pix["binned"] > 100
    m = spectrum_model(r_in(name))
    s = api.disc_spectrum(spec, p, m, limb="laor", V=VP)
    words, _ = spectrum_fused(m, (1, 2.06), rays, spin, VP, reverse)
    assert (s["on_disc"], s["used"]) == tuple(int(w) for w in words[m.ne:m.ne + 2]) and ds.sr.rel_diff(s["flux"], words[:m.ne]) <= 1e-12
    R = response_model(name, r_in(name))
    r = api.disc_response(spec, p, R, limb="laor", V=VP)
    r_words, _ = response_fused(R, (1, 2.06), rays, spin, VP, reverse)
    assert r["used"] == int(r_words[-3]) and ds.sr.rel_diff(r["resp"].ravel(), r_words[:-4]) <= 1e-12


# ---- the programs ---------------------------------------------------------------------------------------------------------------------------------
def test_api_emissivity_angles_takes_the_flow(krlib):
    spec, p, b = lamp_post()
    hist, count2, flux2, mean_mu, tallies = api.emissivity_angles(spec, p, b, 5, V=VP)
    kep = api.emissivity_angles(spec, p, b, 5)
    edges = b.r_min * b.dr ** np.arange(b.nr + 1)
    below = edges[1:] <= pr.r_ms(0.5)
    assert below.sum() >= 3 and (hist["count"][below] > 0).all() and np.array_equal(hist["count"][~below], kep[0]["count"][~below])
    assert kep[0]["count"][0] == 0                                       # beside the horizon the circular orbit is not timelike: V = -1 has no redshift there
    assert np.array_equal(hist["flux"][~below][1:], kep[0]["flux"][~below][1:]) or tga.flux_rel(hist["flux"][~below][1:], kep[0]["flux"][~below][1:]) <= 1e-12
    assert not np.array_equal(hist["flux"][below], kep[0]["flux"][below])
    assert tallies["binned"] == hist["count"].sum() and count2.sum() == tallies["binned"] - tallies["bad_angle"]


def lamp_post():
    """The source, trace and bins of tests/golden/apps/emissivity.par at a = 0.5 with plunge = 1, as kr_emissivity sets them up."""
    spin = 0.5
    spec = ol.pointsource_spec([0.0, 10.0, 1e-3, 1.5707], 0.0, spin, 0.02, 0.02, cosalpha0=-0.995, cosalphamax=0.995, beta0=-PI, betamax=PI)
    p = capi.default_params(spin)
    p.integrator, p.theta_max, p.r_max, p.stop_kind, p.flags = capi.RK4, PI / 2, 1000.0, capi.STOP_THETA, capi.FLAG_HYBRID
    b = gc.emis_bins(spec)
    b.r_isco = b.r_min = 1.02 * api.lib().kr_kerr_horizon(spin)
    b.dr = float(np.exp(np.log(500.0 / b.r_min) / b.nr))
    return spec, p, b


def program(name):
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", name)
    assert os.path.exists(exe), f"{name} not built (__graft_entry__.build())"
    return exe


def header_rows(path, r_in_want):
    text = open(path).read().splitlines()
    assert text[0].split() == ["#", "PLUNGE", "1"] and text[1].split()[:2] == ["#", "R_IN"]
    assert abs(float(text[1].split()[2]) / r_in_want - 1) <= 1e-7
    return text[2:]


def test_line_profile_program_with_plunge_equals_api(krlib, tmp_path):
    exe = program("kr_line_profile")
    out = tmp_path / "line.dat"
    par = os.path.join(ROOT, "tests", "golden", "apps", "imageplane_rk4.par")
    plane = ["--spin=0.5", "--incl=60", "--dist=1000", "--x0=-8", "--xmax=8", "--y0=-8", "--ymax=8", "--Nx=33", "--line_mode=rays", "--e_min=1", "--e_max=10", "--ne=90"]
    r = subprocess.run([exe, f"--parfile={par}", f"--outfile={out}", "--limb=1", "--plunge=1"] + plane, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    edge = 1.02 * api.lib().kr_kerr_horizon(0.5)
    text = header_rows(out, edge)
    assert text[0].split() == ["#", "LIMB", "1"]
    rows = np.array([[float(x) for x in l.split()] for l in text[2:] if l.strip()])
    assert rows.shape == (90, 4)
    d = 16.0 / 33
    spec = ol.imageplane_spec(1000.0, 60.0, -8.0, 8.0, d, -8.0, 8.0, d, 0.5)
    b = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=edge, r_disc=30.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0)
    want = api.line_profile(spec, plane_params(), b, mode="rays", limb=(1, 2.06), V=VP)
    kep_edge = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=pr.r_ms(0.5), r_disc=30.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0)
    assert want["binned"] >= 100 + api.line_profile(spec, plane_params(), kep_edge, mode="rays", limb=(1, 2.06))["binned"]
    problems, m = lr.compare_line({"count": rows[None, :, 3], "flux": rows[None, :, 2]}, want, rtol=1e-6)
    assert problems == [], (problems, m)
    # plunge = 0 is the program without the key, byte for byte; r_in alone changes nothing
    plain, zero = tmp_path / "plain.dat", tmp_path / "zero.dat"
    for path, extra in ((plain, []), (zero, ["--plunge=0", "--r_in=2.5"])):
        r = subprocess.run([exe, f"--parfile={par}", f"--outfile={path}", "--limb=1"] + plane + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    assert open(plain, "rb").read() == open(zero, "rb").read() and open(plain).read().lstrip().startswith("# LIMB")
    # a program that does not take the flow says so
    pol = subprocess.run([program("kr_hotspot_lightcurve"), f"--parfile={os.path.join(ROOT, 'tests', 'golden', 'apps', 'hotspot_lightcurve.par')}", f"--outfile={tmp_path / 'x'}",
                          "--plunge=1"], capture_output=True, text=True, timeout=300)
    assert pol.returncode == 1 and "plunge" in pol.stderr


def test_emissivity_program_with_plunge_equals_api(krlib, tmp_path):
    exe = program("kr_emissivity")
    out, mu_out = tmp_path / "emis.dat", tmp_path / "emis_mu.dat"
    par = os.path.join(ROOT, "tests", "golden", "apps", "emissivity.par")
    r = subprocess.run([exe, f"--parfile={par}", f"--outfile={out}", "--integrator=rk4", "--spin=0.5", "--plunge=1", "--Nmu=5", f"--mu_outfile={mu_out}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    spec, p, b = lamp_post()
    header_rows(out, b.r_min)
    header_rows(mu_out, b.r_min)
    rows, mu_rows = np.loadtxt(out), np.loadtxt(mu_out)
    assert rows.shape == (30, 7) and mu_rows.shape == (30, 7)
    hist, count2, flux2, mean_mu, tallies = api.emissivity_angles(spec, p, b, 5, V=VP)
    edges = b.r_min * b.dr ** np.arange(b.nr + 1)
    np.testing.assert_allclose(rows[:, 0], edges[:-1], rtol=1e-7)
    assert np.array_equal(rows[:, 2], hist["count"]) and hist["count"].sum() > 5000
    area = rows[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_allclose(rows[:, 3], hist["flux"] / area, rtol=1e-6, equal_nan=True)
        np.testing.assert_allclose(rows[:, 4], hist["emis"] / area, rtol=1e-6, equal_nan=True)
        np.testing.assert_allclose(rows[:, 5], hist["sum_redshift"] / hist["count"], rtol=1e-6, equal_nan=True)
        np.testing.assert_allclose(mu_rows[:, 1:6], count2 / hist["count"][:, None], rtol=1e-7, equal_nan=True)
        np.testing.assert_allclose(mu_rows[:, 6], mean_mu, rtol=1e-7, equal_nan=True)
    # the area column: integrate_disc_area, whose plunge branch serves the annuli below the ISCO -- there it is not the circular orbits' area
    below = edges[1:] <= pr.r_ms(0.5)
    assert below.sum() >= 3 and (rows[below, 2] > 0).all()
    area_exe = os.path.join(ROOT, "tests", "cpp", "formats_test")
    assert os.path.exists(area_exe)
    for i in list(np.flatnonzero(below)) + [int(np.flatnonzero(~below)[1])]:
        a = float(subprocess.run([area_exe, "area", "0.5", repr(float(rows[i, 0])), repr(float(rows[i, 0] * b.dr))], capture_output=True, text=True, timeout=60).stdout)
        assert abs(area[i] / a - 1) <= 1e-6, (i, area[i], a)
    circular = api.surface_area(edges, b.r_min, 0.0, 0.0, 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):                 # (beside the horizon the circular orbits have no area at all)
        assert (np.abs(area[below] / circular[below] - 1) > 1e-3).all()
    assert np.abs(area[~below][1:] / circular[~below][1:] - 1).max() <= 1e-6
