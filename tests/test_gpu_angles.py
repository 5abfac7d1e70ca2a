"""GPU: the photon's angles in the disc frame (kr_angles_dev_f64, kr_post_line_limb_dev_f64, kr_post_emissivity_mu_dev_f64; api.arrival_angles,
api.line_profile(limb=...), api.emissivity_angles; the limb and Nmu keys of kr_line_profile and kr_emissivity) against the numpy rules of
tests/angle_rules.py, the passes they extend, and each other.  The records are the fixtures' final__* records pushed to the device: nothing is traced
except by the api and the programs."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import angle_rules as ar
import golden_cases as gc
import line_rules as lr
import oracle_lib as ol
import parity
import reducer_rules as rr
import test_gpu_line_profile as tlp
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPS = os.path.join(ROOT, "tests", "golden", "apps")
PI = math.pi


def fixture_run(case, run):
    """(records, spin as the trace stored it, (V, reverse, projradius) of the case's redshift pass)."""
    c = gc.cases()[case]
    return np.ascontiguousarray(np.load(gc.golden_path(case))[f"final__{run}"]), c["runs"][run].spin, c["post"]


def lds_limit():
    """The LDS budget of post_emissivity_mu_kernel in doubles, from the kernel's own source."""
    text = open(os.path.join(ROOT, "raytrace_cpu_amd", "csrc", "kr_angles.hip")).read()
    return int(re.search(r"constexpr int kMuLdsWords = (\d+);", text).group(1))


# ---- kr_angles_dev_f64 ----------------------------------------------------------------------------------------------------------------
def dev_angles(rays, spin, V, reverse, projradius):
    """kr_angles_dev_f64 on a device copy of `rays`: (mu, chi, the records after the call)."""
    L = api.lib()
    n = len(rays)
    with DeviceScope(L) as dev:
        d, a = dev.upload(rays), dev.upload(np.full(2 * n, 7.0))
        capi.check(L, L.kr_angles_dev_f64(spin, V, reverse, projradius, 0, d, n, a, None), "kr_angles_dev")
        capi.check(L, L.kr_synchronize(None), "sync")
        out, after = dev.fetch(a, 2 * n), dev.fetch(d, n, rays.dtype)
    return out[0::2], out[1::2], after


def check_angles(rays, spin, post, label):
    V, reverse, projradius = post
    f = ar.frame(rays, spin, V, reverse, projradius)
    want_mu, want_chi = ar.mu_chi(f)
    mu, chi, after = dev_angles(rays, spin, V, reverse, projradius)
    assert after.tobytes() == rays.tobytes(), label                                     # the call reads the records and never writes them
    assert np.array_equal(np.isnan(mu), np.isnan(want_mu)) and np.array_equal(np.isnan(chi), np.isnan(want_chi)), label
    assert np.isnan(mu[rays["steps"] <= 0]).all() and np.isnan(chi[rays["steps"] <= 0]).all(), label
    with np.errstate(invalid="ignore"):
        bad = (rays["steps"] > 0) & (~np.isfinite(mu) | (mu > 1))        # E <= 0 shows as mu < 0 or as a mu that is not finite
        bad |= (rays["steps"] > 0) & (mu < 0)
    assert np.array_equal(bad, ar.bad_angle(f)), label
    fin = np.isfinite(want_mu) & np.isfinite(want_chi)
    with np.errstate(invalid="ignore"):
        degenerate = fin & (np.hypot(f["P_r"], f["P_phi"]) < 1e-9 * f["E"])
    assert degenerate.sum() == 0, label                                                 # none on these fixtures: chi is defined wherever it is finite
    # inf - inf: a mu or chi that is infinite must be the same infinity
    inf = np.isinf(want_mu)
    assert np.array_equal(mu[inf], want_mu[inf]), label
    fin &= ~inf
    worst_mu, worst_chi = float(np.abs(mu - want_mu)[fin].max()), float(np.abs(chi - want_chi)[fin].max())
    print(f"{label}: {int(fin.sum())} records, |mu - rule| <= {worst_mu:.2e}, |chi - rule| <= {worst_chi:.2e}, {int(bad.sum())} bad-angle")
    assert worst_mu <= 1e-12 and worst_chi <= 1e-12, label
    return mu, chi


@pytest.mark.parametrize("case,run", [("ip15", "rk4"), ("ps_h10", "rk4"), ("ps_kep5k", "rk4"), ("ps_h5_a05", "rk4_flatdisc")])
def test_angles_match_the_rule(krlib, case, run):
    rays, spin, post = fixture_run(case, run)
    assert case != "ip15" or len(rays) == 256
    check_angles(rays, spin, post, f"{case}/{run}")


@pytest.mark.parametrize("n", [0, 1, 257])
def test_angles_at_the_edges_of_a_workgroup(krlib, n):
    rays, spin, post = fixture_run("ps_h10", "rk4")
    first = int(np.flatnonzero(ar.disc_filter(rays, gc.r_isco(), 500.0))[0])               # a record on the disc: its angles are finite
    assert first + 257 <= len(rays)
    part = np.ascontiguousarray(rays[first:first + n])
    if n == 0:
        L = api.lib()
        with DeviceScope(L) as dev:
            a = dev.upload(np.full(4, 7.0))
            capi.check(L, L.kr_angles_dev_f64(spin, post[0], post[1], post[2], 0, None, 0, a, None), "kr_angles_dev")
            capi.check(L, L.kr_angles_dev_f64(spin, post[0], post[1], post[2], 0, None, 0, None, None), "kr_angles_dev")
            assert (dev.fetch(a, 4) == 7.0).all()
        mu, chi = api.arrival_angles(part, spin, *post)
        assert len(mu) == 0 and len(chi) == 0
        return
    mu, chi = check_angles(part, spin, post, f"ps_h10/rk4 n={n}")
    assert len(mu) == n and np.isfinite(mu).sum() >= 1
    # the host-array form and the api's two forms give the same bits
    h_mu, h_chi = api.arrival_angles(part, spin, *post)
    with DeviceScope(api.lib()) as dev:
        d_mu, d_chi = api.arrival_angles((dev.upload(part), n), spin, *post)
    for got in (h_mu, d_mu):
        assert got.tobytes() == np.ascontiguousarray(mu).tobytes()
    for got in (h_chi, d_chi):
        assert got.tobytes() == np.ascontiguousarray(chi).tobytes()


# ---- the line with a limb law ---------------------------------------------------------------------------------------------------------
def limb_line(b, law, rays, spin, post, calls=1):
    """kr_post_line_limb_dev_f64 `calls` times into one histogram, each on a fresh device copy of `rays`: (dict + bad_angle, records after)."""
    L = api.lib()
    V, reverse, projradius = post
    nw = api.line_words(b) + 1
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        for _ in range(calls):
            with DeviceScope(L) as one:
                d = one.upload(rays)
                capi.check(L, L.kr_post_line_limb_dev_f64(spin, V, reverse, projradius, 0, -PI, PI, C.byref(b), C.byref(law), d, len(rays), h, None), "kr_post_line_limb")
                capi.check(L, L.kr_synchronize(None), "sync")
                after = one.fetch(d, len(rays), rays.dtype)
        words = dev.fetch(h, nw)
    out = api.line_from_words(b, words[:-1])
    out["bad_angle"] = int(words[-1])
    out["words"] = words
    return out, after


def plain_line(b, rays, spin, post):
    L = api.lib()
    V, reverse, projradius = post
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(api.line_words(b) * 8)
        capi.check(L, L.kr_post_line_dev_f64(spin, V, reverse, projradius, 0, -PI, PI, C.byref(b), d, len(rays), h, None), "kr_post_line")
        capi.check(L, L.kr_synchronize(None), "sync")
        after, words = dev.fetch(d, len(rays), rays.dtype), dev.fetch(h, api.line_words(b))
    return api.line_from_words(b, words), after


def flux_rel(got, want):
    g, w = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert np.array_equal(w == 0, g == 0)
    nz = w != 0
    return float((np.abs(g - w)[nz] / np.abs(w[nz])).max()) if nz.any() else 0.0


@pytest.mark.parametrize("case", ["ip15", "ip16"])
def test_line_with_limb_law(krlib, case):
    rays, spin, post = fixture_run(case, "rk4")
    b = tlp.line_bins()
    plain, plain_rays = plain_line(b, rays, spin, post)
    assert plain["binned"] > 30
    for name, (law_id, coeff) in capi.LIMB_LAWS.items():
        law = capi.limb_law((law_id, coeff))
        got, after = limb_line(b, law, rays, spin, post)
        assert after.tobytes() == plain_rays.tobytes(), (case, name)                    # rays[] exactly as after kr_post_line_dev_f64
        want = ar.line_limb_rule(b, law_id, coeff, rays, spin, *post, g=plain_rays["redshift"])
        assert (got["on_disc"], got["binned"], got["bad_angle"]) == (want["on_disc"], want["binned"], want["bad_angle"]), (case, name)
        assert np.array_equal(got["count"], want["count"]), (case, name)
        worst = flux_rel(got["flux"], want["flux"])
        print(f"{case} {name}: {got['binned']} binned, flux against the rule <= {worst:.2e}")
        assert worst <= 1e-12, (case, name)
        if law_id == 0:
            assert np.array_equal(got["count"], plain["count"]) and (got["on_disc"], got["binned"]) == (plain["on_disc"], plain["binned"])
            problems, m = lr.compare_line(got, plain, rtol=1e-12, slack=0, max_excluded=0)
            assert problems == [], (case, problems, m)
        else:
            assert not np.array_equal(got["flux"], plain["flux"])
        twice, _ = limb_line(b, law, rays, spin, post, calls=2)
        assert np.array_equal(twice["words"], 2 * got["words"]), (case, name)           # the call adds (x2 is exact: every partial sum doubles)


def test_line_leaves_bad_angle_rays_out(krlib):
    """ps_h10/euler seen with reverse = 0 (unphysical for a line, but its records carry the bad-angle rays): counted, and absent from the bins under
    a law that needs their angle."""
    rays, spin, _ = fixture_run("ps_h10", "euler")
    post = (-1.0, 0, 0)
    b = tlp.line_bins(r_disc=500.0, e_min=0.0, de=0.5, ne=90)
    _, plain_rays = plain_line(b, rays, spin, post)
    res = {}
    for law_id in (0, 1):
        got, after = limb_line(b, capi.limb_law((law_id, 2.06)), rays, spin, post)
        want = ar.line_limb_rule(b, law_id, 2.06, rays, spin, *post, g=plain_rays["redshift"])
        assert after.tobytes() == plain_rays.tobytes()
        assert (got["on_disc"], got["binned"], got["bad_angle"]) == (want["on_disc"], want["binned"], want["bad_angle"]), law_id
        assert np.array_equal(got["count"], want["count"]) and flux_rel(got["flux"], want["flux"]) <= 1e-12, law_id
        res[law_id] = (got, want)
    got0, got1 = res[0][0], res[1][0]
    f = ar.frame(rays, spin, *post)
    disc = ar.disc_filter(rays, b.r_isco, b.r_disc) & (plain_rays["redshift"] > 0)
    assert got1["bad_angle"] == int((ar.bad_angle(f) & disc).sum()) == 12 == got0["bad_angle"]
    assert got0["on_disc"] == got1["on_disc"] and 0 < got0["binned"] - got1["binned"] <= 12
    assert np.isfinite(got1["flux"]).all() and (got1["count"] <= got0["count"]).all()


# ---- emissivity by incidence angle ----------------------------------------------------------------------------------------------------
def hist_dict(words, nr):
    out = {"count": np.rint(words[:nr]).astype(np.int64), "disc_count": int(round(float(words[5 * nr])))}
    assert np.array_equal(out["count"], words[:nr])
    for q, k in enumerate(rr.EMIS_SUMS):
        out[k] = words[(q + 1) * nr:(q + 2) * nr]
    return out


def run_emissivity_mu(b, nmu, rays, spin, post):
    """(hist words of kr_post_emissivity_dev_f64, hist words and mu words of kr_post_emissivity_mu_dev_f64 called twice / 2, records after each)."""
    L = api.lib()
    V, reverse, projradius = post
    n, nh, nm = len(rays), 5 * b.nr + 1, api.emissivity_mu_words(b, nmu)
    mb = capi.MuBins(nmu, 0)
    with DeviceScope(L) as dev:
        d0, h0 = dev.upload(rays), dev.zeros(nh * 8)
        capi.check(L, L.kr_post_emissivity_dev_f64(spin, V, reverse, projradius, 0, -PI, PI, C.byref(b), d0, n, h0, None), "kr_post_emissivity")
        d1, h1, m1 = dev.upload(rays), dev.zeros(nh * 8), dev.zeros(nm * 8)
        capi.check(L, L.kr_post_emissivity_mu_dev_f64(spin, V, reverse, projradius, 0, -PI, PI, C.byref(b), C.byref(mb), d1, n, h1, m1, None), "kr_post_emissivity_mu")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(h0, nh), dev.fetch(h1, nh), dev.fetch(m1, nm), dev.fetch(d0, n, rays.dtype), dev.fetch(d1, n, rays.dtype)


def check_emissivity_mu(b, nmu, rays, spin, post, label):
    h_plain, h_mu, m_words, rays_plain, rays_mu = run_emissivity_mu(b, nmu, rays, spin, post)
    assert rays_mu.tobytes() == rays_plain.tobytes(), label
    hist_want, want = ar.emissivity_mu_rule(b, nmu, rays, spin, *post, g=rays_plain["redshift"])
    got_plain, got_hist = hist_dict(h_plain, b.nr), hist_dict(h_mu, b.nr)
    assert np.array_equal(got_hist["count"], got_plain["count"]) and got_hist["disc_count"] == got_plain["disc_count"], label
    for g in (got_plain, got_hist):
        rr.check_reduction(g, hist_want, "count", rr.EMIS_SUMS, parity.BIN_RTOL, label)
    got = ar.mu_from_words(b.nr, nmu, m_words)
    assert np.array_equal(m_words[:b.nr * nmu], np.rint(m_words[:b.nr * nmu])), label
    assert np.array_equal(got["count2"], want["count2"]), label
    assert (got["disc_count"], got["binned"], got["bad_angle"]) == (want["disc_count"], want["binned"], want["bad_angle"]), label
    worst = max(flux_rel(got["flux2"], want["flux2"]), flux_rel(got["sum_mu"], want["sum_mu"]))
    assert worst <= 1e-12, (label, worst)
    # the two marginal identities, exactly
    assert got["count2"].sum() == got["binned"] - got["bad_angle"], label
    assert np.array_equal(got["count2"].sum(axis=1), got_hist["count"] - want["bad_per_bin"]), label
    assert got["binned"] == got_hist["count"].sum() and got["disc_count"] == got_hist["disc_count"], label
    print(f"{label}: binned {got['binned']}, bad-angle {got['bad_angle']}, flux2 / sum_mu against the rule <= {worst:.2e}")
    return got


@pytest.mark.parametrize("nmu", [1, 5, 64])
@pytest.mark.parametrize("case,run,n_bad", [("ps_h10", "rk4", 2), ("ps_h10", "euler", 12), ("ps_kep5k", "rk4", 5)])
def test_emissivity_by_angle(krlib, case, run, n_bad, nmu):
    rays, spin, post = fixture_run(case, run)
    b = gc.emis_bins(gc.cases()[case]["source"])
    assert 5 * b.nr + 1 + api.emissivity_mu_words(b, nmu) <= lds_limit()                # the LDS instantiation
    got = check_emissivity_mu(b, nmu, rays, spin, post, f"{case}/{run} nmu={nmu}")
    assert got["bad_angle"] == n_bad
    if nmu == 5:
        assert (got["count2"].sum(axis=0) > 0).all()                                     # every fifth of the mu axis is populated


def test_emissivity_by_angle_beyond_the_lds(krlib):
    """nr x nmu from the kernel's own LDS budget: the first size whose two histograms do not fit it, against the rule and against the LDS
    instantiation's marginals."""
    rays, spin, post = fixture_run("ps_h10", "rk4")
    src = gc.cases()["ps_h10"]["source"]
    limit, nmu = lds_limit(), 64
    nr = next(nr for nr in range(30, 10000) if 5 * nr + 1 + (2 * nmu + 1) * nr + 3 > limit)
    small, big = gc.emis_bins(src, nr=nr - 1), gc.emis_bins(src, nr=nr)
    assert 5 * small.nr + 1 + api.emissivity_mu_words(small, nmu) <= limit < 5 * big.nr + 1 + api.emissivity_mu_words(big, nmu)
    g_small = check_emissivity_mu(small, nmu, rays, spin, post, f"nr={small.nr} (LDS)")
    g_big = check_emissivity_mu(big, nmu, rays, spin, post, f"nr={big.nr} (global)")
    assert np.array_equal(g_small["count2"].sum(axis=0), g_big["count2"].sum(axis=0)) and g_small["bad_angle"] == g_big["bad_angle"]


# ---- api and programs -----------------------------------------------------------------------------------------------------------------
def test_api_line_profile_with_limb_equals_the_c_abi_sequence(krlib):
    L = api.lib()
    spec, p, b = tlp.plane(16), tlp.image_params(), tlp.line_bins()
    got = api.line_profile(spec, p, b, limb="laor")
    n = api.imageplane_count(spec)[0]
    law = capi.limb_law((1, 2.06))
    nw = api.line_words(b) + 1
    with DeviceScope(L) as dev:
        d, h = dev.alloc(n * 144), dev.zeros(nw * 8)
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(spec), 0, 1, 0.0, 1, 0, d, n, None), "init")
        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d, n, None, None), "trace")
        capi.check(L, L.kr_post_line_limb_dev_f64(-tlp.SPIN, -1.0, 1, 0, 0, -PI, PI, C.byref(b), C.byref(law), d, n, h, None), "kr_post_line_limb")
        capi.check(L, L.kr_synchronize(None), "sync")
        words = dev.fetch(h, nw)
    want = api.line_from_words(b, words[:-1])
    assert got["binned"] > 30 and (got["on_disc"], got["binned"], got["bad_angle"]) == (want["on_disc"], want["binned"], int(words[-1]))
    assert np.array_equal(got["count"], want["count"])
    np.testing.assert_allclose(got["flux"], want["flux"], rtol=1e-12, atol=0)
    iso = api.line_profile(spec, p, b)                                                   # limb=None: today's path, today's keys
    assert "bad_angle" not in iso and np.array_equal(iso["count"], got["count"]) and not np.array_equal(iso["flux"], got["flux"])
    with pytest.raises(capi.KrError):
        api.line_profile(spec, p, b, mode="pixels", limb="laor")


def test_line_profile_app_with_limb_equals_api(krlib, tmp_path):
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_line_profile")
    assert os.path.exists(exe), "kr_line_profile not built (__graft_entry__.build())"
    out = tmp_path / "line.dat"
    r = subprocess.run([exe, f"--parfile={tlp.PAR}", f"--outfile={out}", "--line_mode=rays", "--e_min=1", "--e_max=10", "--ne=90", "--limb=1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(out).read().splitlines()
    assert text[0].split() == ["#", "LIMB", "1"] and text[1].split()[:2] == ["#", "LIMBCOEF"] and float(text[1].split()[2]) == 2.06
    rows = np.array([[float(x) for x in l.split()] for l in text[2:] if l.strip()])
    assert rows.shape == (90, 4)
    b = tlp.line_bins()
    want = api.line_profile(tlp.plane(31), tlp.image_params(), b, mode="rays", limb=(1, 2.06))
    assert want["binned"] > 50
    problems, m = lr.compare_line({"count": rows[None, :, 3], "flux": rows[None, :, 2]}, want, rtol=1e-6)
    assert problems == [], (problems, m)
    r = subprocess.run([exe, f"--parfile={tlp.PAR}", f"--outfile={out}", "--line_mode=pixels", "--limb=1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "line_mode = rays" in r.stderr


def test_emissivity_app_with_nmu_equals_api(krlib, tmp_path):
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_emissivity")
    assert os.path.exists(exe), "kr_emissivity not built (__graft_entry__.build())"
    out, mu_out = tmp_path / "emis.dat", tmp_path / "emis_mu.dat"
    r = subprocess.run([exe, f"--parfile={os.path.join(APPS, 'emissivity.par')}", f"--outfile={out}", "--integrator=rk4", "--Nmu=5", f"--mu_outfile={mu_out}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = np.loadtxt(mu_out)
    assert rows.shape == (30, 7)
    spin = 0.998
    spec = ol.pointsource_spec([0.0, 10.0, 1e-3, 1.5707], 0.0, spin, 0.02, 0.02, cosalpha0=-0.995, cosalphamax=0.995, beta0=-PI, betamax=PI)
    p = capi.default_params(spin)
    p.integrator, p.theta_max, p.r_max, p.stop_kind, p.flags = capi.RK4, PI / 2, 1000.0, capi.STOP_THETA, capi.FLAG_HYBRID
    b = gc.emis_bins(spec)
    hist, count2, flux2, mean_mu, tallies = api.emissivity_angles(spec, p, b, 5)
    assert tallies["binned"] == hist["count"].sum() > 5000 and count2.sum() == tallies["binned"] - tallies["bad_angle"]
    assert (flux2[count2 > 0] > 0).all() and (flux2[count2 == 0] == 0).all()
    np.testing.assert_allclose(rows[:, 0], b.r_min * b.dr ** np.arange(30), rtol=1e-7)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = count2 / hist["count"][:, None]
    np.testing.assert_allclose(rows[:, 1:6], share, rtol=1e-7, atol=0, equal_nan=True)
    np.testing.assert_allclose(rows[:, 6], mean_mu, rtol=1e-7, atol=0, equal_nan=True)
    # the 7-column table beside it is the one the program writes without Nmu
    plain = tmp_path / "plain.dat"
    r = subprocess.run([exe, f"--parfile={os.path.join(APPS, 'emissivity.par')}", f"--outfile={plain}", "--integrator=rk4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    a, c = np.loadtxt(out), np.loadtxt(plain)
    assert np.array_equal(a[:, :3], c[:, :3])
    np.testing.assert_allclose(a[:, 3:], c[:, 3:], rtol=1e-6, equal_nan=True)
