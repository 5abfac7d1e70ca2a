"""GPU: the polarisation of disc emission (kr_polarisation_dev_f64, kr_post_image_stokes_dev_f64, kr_post_line_stokes_dev_f64; api.polarisation,
api.stokes_image, api.stokes_line; the program kr_imageplane_polarisation) against the numpy rules of tests/polarisation_rules.py, the passes they
extend, and each other.  The records are the fixtures' final__* records pushed to the device unless a test says otherwise."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import angle_rules as ar
import fits_lite
import golden_cases as gc
import oracle_lib as ol
import polarisation_rules as pr
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPS = os.path.join(ROOT, "tests", "golden", "apps")
PI = math.pi
INC_DEG, R_DISC = 80.0, 30.0
SUM_RTOL = 1e-12                 # of the per-cell sum of absolute terms: the bar of the other reducer tests
LIMBS = {0: (0, 0.0), 1: (1, 2.06)}
POLS = {0: (0, 1.0), 1: (1, 0.1171)}


def fixture_run(case, run):
    """(records, spin as the trace stored it, (V, reverse, projradius) of the case's redshift pass)."""
    c = gc.cases()[case]
    return np.ascontiguousarray(np.load(gc.golden_path(case))[f"final__{run}"]), c["runs"][run].spin, c["post"]


def disc_index(rays):
    return np.flatnonzero(ar.disc_filter(rays, gc.r_isco(), R_DISC))


def lds_limit():
    """The LDS budget of the line kernels in doubles, from the kernels' own source."""
    text = open(os.path.join(ROOT, "raytrace_cpu_amd", "csrc", "kr_line.hip")).read()
    return int(re.search(r"constexpr int kLineLdsWords = (\d+);", text).group(1))


def image_bins(n_pix, flip=1):
    """n_pix x n_pix pixels over the 16 x 16 ray grid of ip15 (x = -30 + 4 i), every ray in the middle of its cell: 16 -> one ray per pixel, 4 -> 16."""
    b = capi.ImageBins()
    b.x0 = b.y0 = -32.0
    b.img_dx = b.img_dy = 64.0 / n_pix
    b.r_isco, b.r_disc = gc.r_isco(), R_DISC
    b.q1, b.rb1, b.q2, b.rb2, b.q3 = 3.0, 4.0, 3.0, 10.0, 3.0
    b.img_nx = b.img_ny = n_pix
    b.flip_image = flip
    return b


def line_bins(**kw):
    base = dict(line_energy=6.4, e_min=1.0, de=1.0, ne=8, r_isco=gc.r_isco(), r_disc=R_DISC, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0)
    base.update(kw)
    return capi.line_bins(**base)


# ---- a. the per-record pass ---------------------------------------------------------------------------------------------------------
def dev_polarisation(rays, spin, V, projradius, inc_deg=INC_DEG):
    """kr_polarisation_dev_f64 on a device copy of `rays`: (the four outputs as a dict, the records after the call)."""
    L = api.lib()
    n = len(rays)
    with DeviceScope(L) as dev:
        d, o = dev.upload(rays), dev.upload(np.full(4 * n, 7.0))
        capi.check(L, L.kr_polarisation_dev_f64(spin, V, 1, projradius, 0, inc_deg, d, n, o, None), "kr_polarisation_dev")
        capi.check(L, L.kr_synchronize(None), "sync")
        out, after = dev.fetch(o, 4 * n), dev.fetch(d, n, rays.dtype)
    return {k: out[q::4].copy() for q, k in enumerate(("kappa1", "kappa2", "c2", "s2"))}, after


def check_polarisation(rays, spin, post, label):
    V, reverse, projradius = post
    assert reverse == 1
    want = pr.polarisation(rays, spin, INC_DEG, V, reverse, projradius)
    got, after = dev_polarisation(rays, spin, V, projradius)
    assert after.tobytes() == rays.tobytes(), label                                     # the call reads the records and never writes them
    for k in ("kappa1", "kappa2", "c2", "s2"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (label, k, np.flatnonzero(np.isnan(got[k]) != np.isnan(want[k])))
        assert np.isnan(got[k][rays["steps"] <= 0]).all(), (label, k)
        inf = np.isinf(want[k])
        assert np.array_equal(got[k][inf], want[k][inf]), (label, k)
    fin = np.all([np.isfinite(want[k]) for k in ("kappa1", "kappa2", "c2", "s2")], axis=0)
    with np.errstate(invalid="ignore"):
        rel = np.hypot(got["kappa1"] - want["kappa1"], got["kappa2"] - want["kappa2"]) / np.hypot(want["kappa1"], want["kappa2"])
        dc, ds = np.abs(got["c2"] - want["c2"]), np.abs(got["s2"] - want["s2"])
    i = int(np.argmax(np.where(fin, rel, 0)))
    print(f"{label}: {int(fin.sum())} finite records, |kappa - rule| / |kappa| <= {rel[fin].max():.2e} (record {i}: r = {rays['r'][i]:.6g}, x = {rays['alpha'][i]}, "
          f"y = {rays['beta'][i]}), |c2 - rule| <= {dc[fin].max():.2e}, |s2 - rule| <= {ds[fin].max():.2e}, {int(want['bad'].sum())} bad-pol")
    assert rel[fin].max() <= 1e-12 and dc[fin].max() <= 1e-12 and ds[fin].max() <= 1e-12, label
    return got


@pytest.mark.parametrize("case,run", [("ip15", "rk4"), ("ip15", "euler"), ("ip15", "rk45"), ("ip15", "rk4_plane"), ("ip16", "rk4")])
def test_polarisation_matches_the_rule(krlib, case, run):
    rays, spin, post = fixture_run(case, run)
    assert len(rays) == (289 if case == "ip16" else 256)
    if case == "ip16":
        centre = (rays["alpha"] == 0) & (rays["beta"] == 0)
        assert centre.sum() == 1 and np.isnan(rays["Q"][centre]).all()                   # the (0, 0) pixel with NaN constants
    check_polarisation(rays, spin, post, f"{case}/{run}")


# ---- b. edge sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257])
def test_polarisation_at_the_edges_of_a_workgroup(krlib, n):
    rays, spin, post = fixture_run("ip15", "rk4")
    V, _, projradius = post
    on_disc = int(disc_index(rays)[0])
    part = np.ascontiguousarray({0: rays[:0], 1: rays[on_disc:on_disc + 1], 257: np.concatenate([rays, rays[on_disc:on_disc + 1]])}[n])
    assert len(part) == n
    if n == 0:
        L = api.lib()
        with DeviceScope(L) as dev:
            o = dev.upload(np.full(8, 7.0))
            capi.check(L, L.kr_polarisation_dev_f64(spin, V, 1, projradius, 0, INC_DEG, None, 0, o, None), "kr_polarisation_dev")
            capi.check(L, L.kr_polarisation_dev_f64(spin, V, 1, projradius, 0, INC_DEG, None, 0, None, None), "kr_polarisation_dev")
            capi.check(L, L.kr_synchronize(None), "sync")
            assert (dev.fetch(o, 8) == 7.0).all()
        assert all(len(v) == 0 for v in api.polarisation(part, spin, INC_DEG, V, projradius).values())
        return
    got = check_polarisation(part, spin, post, f"ip15/rk4 n={n}")
    assert all(np.isfinite(got[k][-1]) for k in got)                                    # the last record is a disc record
    if n == 257:
        assert all(got[k][-1].tobytes() == got[k][on_disc].tobytes() for k in got)
    host = api.polarisation(part, spin, INC_DEG, V, projradius)
    with DeviceScope(api.lib()) as dev:
        from_dev = api.polarisation((dev.upload(part), n), spin, INC_DEG, V, projradius)
    for other in (host, from_dev):
        assert sorted(other) == sorted(got) and all(other[k].tobytes() == got[k].tobytes() for k in got)


# ---- the reducers through the C ABI -------------------------------------------------------------------------------------------------
def stokes_image(b, limb, pol, rays, spin, post, calls=1, inc_deg=INC_DEG):
    """kr_post_image_stokes_dev_f64 `calls` times into one buffer, each on a fresh device copy of `rays`: (words, records after)."""
    L = api.lib()
    V, reverse, projradius = post
    law, plaw, nw = capi.limb_law(limb), capi.pol_law(pol), api.stokes_image_words(b)
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        for _ in range(calls):
            with DeviceScope(L) as one:
                d = one.upload(rays)
                capi.check(L, L.kr_post_image_stokes_dev_f64(spin, V, reverse, projradius, 0, -PI, PI, inc_deg, C.byref(b), C.byref(law), C.byref(plaw), d, len(rays), h, None),
                           "kr_post_image_stokes")
                capi.check(L, L.kr_synchronize(None), "sync")
                after = one.fetch(d, len(rays), rays.dtype)
        return dev.fetch(h, nw), after


def plain_image(b, rays, spin, post):
    L = api.lib()
    V, reverse, projradius = post
    nw = api.image_words(b)
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(nw * 8)
        capi.check(L, L.kr_post_image_dev_f64(spin, V, reverse, projradius, 0, -PI, PI, C.byref(b), d, len(rays), h, None), "kr_post_image")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(h, nw), dev.fetch(d, len(rays), rays.dtype)


def stokes_line(b, limb, pol, rays, spin, post, calls=1, inc_deg=INC_DEG):
    L = api.lib()
    V, reverse, projradius = post
    law, plaw, nw = capi.limb_law(limb), capi.pol_law(pol), api.stokes_line_words(b)
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        for _ in range(calls):
            with DeviceScope(L) as one:
                d = one.upload(rays)
                capi.check(L, L.kr_post_line_stokes_dev_f64(spin, V, reverse, projradius, 0, -PI, PI, inc_deg, C.byref(b), C.byref(law), C.byref(plaw), d, len(rays), h, None),
                           "kr_post_line_stokes")
                capi.check(L, L.kr_synchronize(None), "sync")
                after = one.fetch(d, len(rays), rays.dtype)
        return dev.fetch(h, nw), after


def plain_line(b, rays, spin, post):
    L = api.lib()
    V, reverse, projradius = post
    nw = api.line_words(b)
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(nw * 8)
        capi.check(L, L.kr_post_line_dev_f64(spin, V, reverse, projradius, 0, -PI, PI, C.byref(b), d, len(rays), h, None), "kr_post_line")
        capi.check(L, L.kr_synchronize(None), "sync")
        return api.line_from_words(b, dev.fetch(h, nw)), dev.fetch(d, len(rays), rays.dtype)


# ---- c. synthesised bad records -----------------------------------------------------------------------------------------------------
def test_bad_records(krlib):
    """A disc record and three spoilt copies of it: steps = 0 (dead), Q x 1e4 (mu > 1: bad-angle, hence bad-pol), alpha = beta = NaN (no observer)."""
    rays, spin, post = fixture_run("ip15", "rk4")
    V, _, projradius = post
    part = np.ascontiguousarray(rays[[int(disc_index(rays)[0])] * 4])
    part["steps"][1] = 0
    part["Q"][2] *= 1e4
    part["alpha"][3] = part["beta"][3] = np.nan
    want = pr.polarisation(part, spin, INC_DEG, *post)
    assert want["bad"].tolist() == [False, False, True, True] and want["mu"][2] > 1
    got = check_polarisation(part, spin, post, "bad records")
    assert all(np.isnan(got[k][1]) for k in got)                                           # four NaNs for the dead record
    assert all(np.isfinite(want[k][2]) and np.isfinite(got[k][2]) for k in got)            # as computed: the consumer filters
    assert np.isfinite(got["kappa1"][3]) and np.isfinite(got["kappa2"][3]) and np.isnan(got["c2"][3]) and np.isnan(got["s2"][3])

    b = image_bins(4)
    _, plain_rays = plain_image(b, part, spin, post)
    words, _ = stokes_image(b, LIMBS[1], POLS[1], part, spin, post)
    img = pr.stokes_image_from_words(4, 4, words)
    rule = pr.stokes_image_rule(b, LIMBS[1], POLS[1], part, spin, INC_DEG, *post, g=plain_rays["redshift"])
    pr.check_stokes(img, rule, "nrays", ("disc_count", "bad_pol"), SUM_RTOL, "bad records, image")
    # the NaN coordinates fail the pixel rule (dropped at the filter), the bad-angle record reaches its pixel and moves only the two tallies
    assert (img["disc_count"], img["bad_pol"], int(img["nrays"].sum())) == (2, 1, 1)
    assert np.isfinite(words).all() and sum(int((img[k] != 0).sum()) for k in ("I", "Q", "U")) <= 3

    lb = line_bins()
    words, _ = stokes_line(lb, LIMBS[1], POLS[1], part, spin, post)
    line = pr.stokes_line_from_words(lb, words)
    rule = pr.stokes_line_rule(lb, LIMBS[1], POLS[1], part, spin, INC_DEG, *post, g=plain_rays["redshift"])
    pr.check_stokes(line, rule, "count", ("on_disc", "binned", "bad_pol"), SUM_RTOL, "bad records, line")
    assert (line["on_disc"], line["binned"], line["bad_pol"], int(line["count"].sum())) == (3, 1, 2, 1)
    assert np.isfinite(words).all()


# ---- d. the Stokes image ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", [0, 1])
@pytest.mark.parametrize("limb", [0, 1])
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("n_pix", [16, 4])
def test_stokes_image_matches_the_rule(krlib, n_pix, flip, limb, pol):
    rays, spin, post = fixture_run("ip15", "rk4")
    b = image_bins(n_pix, flip)
    label = f"{n_pix} x {n_pix}, flip {flip}, limb {limb}, pol {pol}"
    plain_words, plain_rays = plain_image(b, rays, spin, post)
    words, after = stokes_image(b, LIMBS[limb], POLS[pol], rays, spin, post)
    assert after.tobytes() == plain_rays.tobytes(), label                               # rays[] exactly as after kr_post_image_dev_f64
    got = pr.stokes_image_from_words(n_pix, n_pix, words)
    want = pr.stokes_image_rule(b, LIMBS[limb], POLS[pol], rays, spin, INC_DEG, *post, g=plain_rays["redshift"])
    assert want["disc_count"] > 30 and (want["nrays"].max() == 1 if n_pix == 16 else want["nrays"].max() > 4)
    worst = pr.check_stokes(got, want, "nrays", ("disc_count", "bad_pol"), SUM_RTOL, label)
    print(f"{label}: {got['disc_count']} rays on the disc, {got['bad_pol']} bad-pol, I / Q / U against the rule <= {worst:.2e} of the sum of |terms|")
    assert np.array_equal(words[:n_pix * n_pix], np.rint(words[:n_pix * n_pix]))
    if limb == 0:
        plain = api.image_planes_from_words(plain_words, n_pix, n_pix)
        assert got["bad_pol"] == 0 and np.array_equal(got["nrays"], plain["nrays"]) and got["disc_count"] == plain["disc_count"], label
        np.testing.assert_allclose(got["I"], plain["flux"], rtol=1e-12, atol=0, err_msg=label)
    twice, _ = stokes_image(b, LIMBS[limb], POLS[pol], rays, spin, post, calls=2)
    if n_pix == 16:
        assert np.array_equal(twice, 2 * words), label                                  # one ray per pixel: every word doubles exactly
    else:                                                                               # the order of a pixel's additions is free: counts exactly, sums to the bar
        assert np.array_equal(twice[:16], 2 * words[:16]) and np.array_equal(twice[64:], 2 * words[64:]), label
        pr.check_stokes(pr.stokes_image_from_words(4, 4, twice / 2), want, "nrays", ("disc_count", "bad_pol"), SUM_RTOL, label + ", twice")


def test_flip_image_moves_pixels_and_nothing_else(krlib):
    """Q and U refer to the plane's own axes, flipped rows or not: the planes of flip_image = 1 are those of flip_image = 0 with iy reversed."""
    rays, spin, post = fixture_run("ip15", "rk4")
    w0, _ = stokes_image(image_bins(16, 0), LIMBS[1], POLS[1], rays, spin, post)
    w1, _ = stokes_image(image_bins(16, 1), LIMBS[1], POLS[1], rays, spin, post)
    for q in range(4):
        assert np.array_equal(w1[q * 256:(q + 1) * 256].reshape(16, 16), w0[q * 256:(q + 1) * 256].reshape(16, 16)[:, ::-1])
    assert np.array_equal(w0[1024:], w1[1024:])


# ---- e. the Stokes line -------------------------------------------------------------------------------------------------------------
def line_cases():
    rays, _, _ = fixture_run("ip15", "rk4")
    t = rays["t"][disc_index(rays)]
    t0, dt = float(t.min()), float((t.max() - t.min()) / 3 * 1.001)
    ne_big = next(ne for ne in range(8, 100000) if 4 * ne + 3 > lds_limit())
    return {"lds": line_bins(), "time-axis": line_bins(nt=3, t0=t0, dt=dt), "global": line_bins(ne=ne_big, de=8.0 / ne_big)}


@pytest.mark.parametrize("limb", [0, 1])
@pytest.mark.parametrize("which", ["lds", "time-axis", "global"])
def test_stokes_line_matches_the_rule(krlib, which, limb):
    rays, spin, post = fixture_run("ip15", "rk4")
    b = line_cases()[which]
    words_needed = 4 * b.nt * b.ne + 3
    assert api.stokes_line_words(b) == words_needed and (words_needed > lds_limit()) == (which == "global")
    label = f"{which} (nt {b.nt}, ne {b.ne}), limb {limb}"
    plain, plain_rays = plain_line(b, rays, spin, post)
    words, after = stokes_line(b, LIMBS[limb], POLS[1], rays, spin, post)
    assert after.tobytes() == plain_rays.tobytes(), label
    got = pr.stokes_line_from_words(b, words)
    want = pr.stokes_line_rule(b, LIMBS[limb], POLS[1], rays, spin, INC_DEG, *post, g=plain_rays["redshift"])
    assert want["binned"] > 30 and (which != "time-axis" or (want["count"].sum(axis=1) > 0).all())
    worst = pr.check_stokes(got, want, "count", ("on_disc", "binned", "bad_pol"), SUM_RTOL, label)
    print(f"{label}: {got['on_disc']} on the disc, {got['binned']} binned, {got['bad_pol']} bad-pol, I / Q / U against the rule <= {worst:.2e} of the sum of |terms|")
    if limb == 0:
        assert got["bad_pol"] == 0 and np.array_equal(got["count"], plain["count"]) and (got["on_disc"], got["binned"]) == (plain["on_disc"], plain["binned"]), label
        np.testing.assert_allclose(got["I"], plain["flux"], rtol=1e-12, atol=0, err_msg=label)
    twice, _ = stokes_line(b, LIMBS[limb], POLS[1], rays, spin, post, calls=2)
    half = pr.stokes_line_from_words(b, twice / 2)
    pr.check_stokes(half, want, "count", ("on_disc", "binned", "bad_pol"), SUM_RTOL, label + ", twice")


# ---- f. Stokes identities -----------------------------------------------------------------------------------------------------------
def test_stokes_identities(krlib):
    rays, spin, post = fixture_run("ip15", "rk4")
    w, _ = stokes_image(image_bins(16), LIMBS[1], POLS[0], rays, spin, post)            # fully polarised, one ray per pixel
    full = pr.stokes_image_from_words(16, 16, w)
    lit = full["nrays"] > 0
    assert lit.sum() > 30 and (full["nrays"] <= 1).all()
    rel = np.abs(full["Q"] ** 2 + full["U"] ** 2 - full["I"] ** 2)[lit] / full["I"][lit] ** 2
    print(f"fully polarised, one ray per pixel: |Q^2 + U^2 - I^2| / I^2 <= {rel.max():.2e} over {int(lit.sum())} pixels")
    assert rel.max() <= 1e-12
    w, _ = stokes_image(image_bins(4), LIMBS[1], POLS[1], rays, spin, post)
    img = pr.stokes_image_from_words(4, 4, w)
    lw, _ = stokes_line(line_bins(), LIMBS[1], POLS[1], rays, spin, post)
    line = pr.stokes_line_from_words(line_bins(), lw)
    for name, s in (("image", img), ("line", line)):
        assert (s["Q"] ** 2 + s["U"] ** 2 <= (0.1171 * s["I"]) ** 2 * (1 + 1e-12)).all(), name
        assert (s["I"] >= 0).all() and (s["I"] > 0).sum() >= 4, name


# ---- g. the Schwarzschild mirror ----------------------------------------------------------------------------------------------------
def test_schwarzschild_mirror(krlib):
    """At a = 0 the rays of pixel columns i and 15 - i differ only in the sign of h: r and theta agree, kappa1 and f_be change sign, so c2 is the
    same and s2 the opposite."""
    spec = ol.imageplane_spec(10000.0, INC_DEG, -30.0, 30.0, 4.0, -30.0, 30.0, 4.0, 0.0)
    rays = api.imageplane_init(spec)
    assert len(rays) == 256
    p = capi.default_params(-0.0)
    p.integrator, p.theta_max, p.r_max, p.stop_kind, p.flags = capi.RK4, PI / 2, 11000.0, capi.STOP_THETA, 0
    out, _ = api.trace(p, rays)
    pol = api.polarisation(out, -0.0, INC_DEG, V=0.0)
    grid = {k: v.reshape(16, 16) for k, v in pol.items()}
    disc = (ar.disc_filter(out, 6.0, R_DISC) & np.isfinite(pol["c2"]) & np.isfinite(pol["s2"])).reshape(16, 16)
    assert np.array_equal(out["alpha"].reshape(16, 16)[:8], -out["alpha"].reshape(16, 16)[:7:-1])
    both = disc[:8] & disc[:7:-1]
    pairs = int(both.sum())
    dc = np.abs(grid["c2"][:8] - grid["c2"][:7:-1])[both]
    ds = np.abs(grid["s2"][:8] + grid["s2"][:7:-1])[both]
    print(f"Schwarzschild mirror: {pairs} pairs, |c2 - c2'| <= {dc.max():.2e}, |s2 + s2'| <= {ds.max():.2e}")
    assert pairs >= 8
    assert dc.max() <= 1e-12 and ds.max() <= 1e-12
    assert np.abs(grid["s2"][:8][both]).max() > 0.1                                        # the sign has something to flip


# ---- h. the program -----------------------------------------------------------------------------------------------------------------
def test_polarisation_program_equals_api(krlib, tmp_path):
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_imageplane_polarisation")
    assert os.path.exists(exe), "kr_imageplane_polarisation not built (__graft_entry__.build())"
    out, spec_out = tmp_path / "pol.fits", tmp_path / "pol.dat"
    r = subprocess.run([exe, f"--parfile={os.path.join(APPS, 'imageplane_polarisation.par')}", f"--outfile={out}", f"--spec_outfile={spec_out}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    spin = 0.998
    plane = ol.imageplane_spec(10000.0, INC_DEG, -30.0, 30.0, 60.0 / 16, -30.0, 30.0, 60.0 / 16, spin)
    p = capi.default_params(-spin)
    p.precision, p.integrator, p.theta_max, p.r_max, p.stop_kind, p.flags = 100.0, capi.RK4, PI / 2, 1.1 * 10000.0, capi.STOP_THETA, capi.FLAG_HYBRID
    b = capi.ImageBins()
    b.x0 = b.y0 = -30.0
    b.img_dx = b.img_dy = 60.0 / 8
    b.r_isco, b.r_disc = api.lib().kr_kerr_isco(spin, 1), R_DISC
    b.q1, b.rb1, b.q2, b.rb2, b.q3 = 3.0, 4.0, 3.0, 10.0, 3.0
    b.img_nx = b.img_ny = 8
    b.flip_image = 1
    want = api.stokes_image(plane, p, b, (1, 0.1171), limb=(1, 2.06))
    assert want["disc_count"] > 30 and (want["I"] > 0).sum() >= 8
    hdus = fits_lite.read(str(out))
    assert [h["name"] for h in hdus] == ["PRIMARY", "NRAYS", "I", "Q", "U", "PDEG", "EVPA"]
    head = hdus[0]["header"]
    assert int(float(head["DISCRAYS"])) == want["disc_count"] and int(float(head["BADPOL"])) == want["bad_pol"] and int(float(head["POLLAW"])) == 1
    planes = {h["name"]: h["data"] for h in hdus[1:]}
    for name, key, scale in (("NRAYS", "nrays", 1.0), ("I", "I", 1.0), ("Q", "Q", 1.0), ("U", "U", 1.0), ("PDEG", "pdeg", 1.0), ("EVPA", "evpa", 180 / PI)):
        expect = np.asarray(want[key], dtype=np.float64).reshape(8, 8).T * scale
        assert planes[name].shape == (8, 8) and np.array_equal(np.isnan(planes[name]), np.isnan(expect)), name
        np.testing.assert_allclose(planes[name], expect, rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
    assert np.isnan(planes["PDEG"]).sum() == (want["I"] == 0).sum() > 0

    lb = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.5, ne=18, r_isco=b.r_isco, r_disc=R_DISC, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0, g_index=3.0)
    line = api.stokes_line(plane, p, lb, (1, 0.1171), limb=(1, 2.06))
    rows = np.loadtxt(spec_out)
    assert rows.shape == (18, 6) and line["binned"] > 30
    np.testing.assert_allclose(rows[:, 0], 1.0 + 0.5 * (np.arange(18) + 0.5), rtol=1e-7)
    for col, key, scale in ((1, "I", 1.0), (2, "Q", 1.0), (3, "U", 1.0), (4, "pdeg", 1.0), (5, "evpa", 180 / PI)):
        np.testing.assert_allclose(rows[:, col], line[key][0] * scale, rtol=1e-7, atol=0, equal_nan=True, err_msg=key)
