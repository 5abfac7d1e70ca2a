"""GPU: the Stokes light curves of the orbiting hot spot (kr_post_hotspot_stokes_dev_f64, kr_reduce_hotspot_stokes_dev_f64,
kr_reduce_hotspot_stokes_f64, api.hotspot_lightcurve(pol=...), apps/kr_hotspot_lightcurve with pol_law) against the numpy rule of
tests/hotspot_stokes_rules.py, the per-record polarisation pass, the line pass whose records it must leave, and itself.

The bar is the one of tests/test_gpu_hotspot.py.  Tallies are exact.  flux, sx, sy, Q, U and the spectrogram, each as a whole, stay within
max(16 x noise, floor) of the float64 rule: `noise` is the rule's own float64 - longdouble difference on the same records, `floor` is hot_floor of
tests/test_gpu_hotspot.py (what the number format alone allows; derived there), times the largest |delta| of a used record for Q and U, whose terms
are the flux's times delta c2 or delta s2.  Differences in Q and U are taken in units of max_k P[k], P = sum c |delta| s, the polarised flux without
cancellation; the others in units of the plane's largest magnitude.  Every case goes through parity.record_margin.

Records: those of tests/test_gpu_hotspot.py -- the fixtures ip15 and ip16 (80 degrees) and the 65 x 65 planes at 80 and at 30 degrees, traced once per
session -- and a copy of the 80-degree plane with three ring records spoilt into bad-pol records.  Each comparison first asserts on the RULE's output
that the case is not vacuous: `used` above 100 on the planes, max P > 0; the spoilt plane has bad-pol records in the ring."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hotspot_rules as hr
import hotspot_stokes_rules as hs
import parity
import test_gpu_hotspot as th
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope
from test_hotspot_stokes_rules import WINDING_AT_30_DEGREES

pytestmark = pytest.mark.gpu

PI, SPIN, POST = th.PI, th.SPIN, th.POST
LAOR, CHANDRA, CONSTANT = (1, 2.06), (1, 0.1171), (0, 0.3)
LIMBS = {"iso": (0, 0.0), "laor": LAOR, "bright": (2, 0.0)}
INCL = {"ip15": 80.0, "ip16": 80.0, "plane80": 80.0, "plane30": 30.0, "spoilt80": 80.0}

_RAW, _POL = {}, {}


def records(name):
    """th.records, and "spoilt80": plane80 with three records of the r = 10 ring made bad-pol -- Q x 1e4 twice (mu > 1: bad-angle), alpha = beta = NaN
    once (no observer).  A copy: the session's records stay as traced."""
    if name != "spoilt80":
        return th.records(name)
    if name not in _RAW:
        src = th.records("plane80")
        post, _ = th.post_line_records("plane80")
        h = th.spot()
        idx = np.flatnonzero(hr.disc_filter(h, post) & hr.ring(h, post))[[3, 50, 100]]
        rays = src.copy()
        rays["Q"][idx[:2]] *= 1e4
        rays["alpha"][idx[2]] = rays["beta"][idx[2]] = np.nan
        _RAW[name] = rays
    return _RAW[name]


def post_records(name):
    """rays[] after kr_post_line_dev_f64 (cached per name)."""
    if name == "spoilt80":
        if "post" not in _RAW:
            _RAW["post"] = th.post_line_records(records(name))[0]
        return _RAW["post"]
    return th.post_line_records(name)[0]


def polar(name):
    if name not in _POL:
        _POL[name] = hs.polar(post_records(name), -SPIN, INCL[name])
    return _POL[name]


def fused(h, limb, pol, rays, incl, calls=1):
    """kr_post_hotspot_stokes_dev_f64 `calls` times into one zeroed buffer, each on a fresh device copy of `rays`: (words, records after)."""
    L = api.lib()
    law, plaw = capi.limb_law(limb), capi.pol_law(pol)
    nw = api.hotspot_stokes_words(h)
    with DeviceScope(L) as dev:
        out = dev.zeros(nw * 8)
        after = rays
        for _ in range(calls):
            with DeviceScope(L) as one:
                d = one.upload(rays) if len(rays) else None
                capi.check(L, L.kr_post_hotspot_stokes_dev_f64(-SPIN, *POST, 0, -PI, PI, incl, C.byref(h), C.byref(law), C.byref(plaw), d, len(rays), out, None),
                           "kr_post_hotspot_stokes")
                capi.check(L, L.kr_synchronize(None), "sync")
                after = one.fetch(d, len(rays), rays.dtype) if len(rays) else rays
        return dev.fetch(out, nw), after


def reduced(h, limb, pol, rays, incl):
    """kr_reduce_hotspot_stokes_dev_f64 on a device copy of records that carry their redshift: (words, records after)."""
    L = api.lib()
    law, plaw = capi.limb_law(limb), capi.pol_law(pol)
    nw = api.hotspot_stokes_words(h)
    with DeviceScope(L) as dev:
        out = dev.zeros(nw * 8)
        d = dev.upload(rays) if len(rays) else None
        capi.check(L, L.kr_reduce_hotspot_stokes_dev_f64(-SPIN, POST[0], POST[1], POST[2], incl, C.byref(h), C.byref(law), C.byref(plaw), d, len(rays), out, None),
                   "kr_reduce_hotspot_stokes")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(out, nw), (dev.fetch(d, len(rays), rays.dtype) if len(rays) else rays)


def plane_guard(lo):
    return lo["used"] > 100 and lo["p"].max() > 0 and lo["flux"].max() > 0


def fixture_guard(lo):
    return lo["used"] > 20 and lo["p"].max() > 0 and lo["flux"].max() > 0


def against_the_rule(test, case, h, words, rec, pol, limb, pol_law, guard, rule=None):
    """The guard on the rule's output first (a vacuous case fails as vacuous), then tallies exact and every plane within max(16 x noise, floor) of the
    float64 rule (rule: (noise, lo, hi) taken before, for a second form on the same records); returns (noise, lo, hi)."""
    noise, lo, hi = rule if rule is not None else hs.noise(h, rec, pol, limb=limb, pol_law=pol_law)
    assert guard(lo), (test, case, "vacuous", lo["on_disc"], lo["used"], lo["bad_pol"], float(lo["p"].max()))
    got = hs.from_words(h, words)
    assert (got["on_disc"], got["used"], got["bad_pol"]) == (lo["on_disc"], lo["used"], lo["bad_pol"]), (test, case, got["on_disc"], got["used"], got["bad_pol"])
    assert words[-1] == 0.0 and np.isfinite(words).all(), (test, case)
    base = th.hot_floor(h, rec, lo["used_index"])
    for k in hs.PLANES:
        floor = base * lo["delta_max"] if k in ("q", "u") else base
        diff, allowed = hs.diff(got, lo, k), max(16 * noise[k], floor)
        print(f"{test} {case} {k}: used {got['used']} bad_pol {got['bad_pol']} pairs {lo['pairs']}; noise {noise[k]:.3e}, floor {floor:.3e}, device - rule {diff:.3e}, "
              f"device - longdouble rule {hs.diff(got, hi, k):.3e}")
        parity.record_margin(test, f"{case}-{k}", {"n_traced": int(len(rec)), "n_bad": 0, "frac_bad": 0.0, "worst_ok": diff}, allowed=allowed, noise=noise[k], floor=floor,
                             device_minus_rule=diff, device_minus_longdouble_rule=hs.diff(got, hi, k), used=got["used"], bad_pol=got["bad_pol"], pairs=lo["pairs"],
                             nt=int(h.nt), ne=int(h.ne), scale=hs.scale(lo, k))
        assert diff <= allowed, (test, case, k, diff, noise[k], floor)
    return noise, lo, hi


def both_forms(test, case, name, h, limb, pol_law, guard, rays=None, post=None, pol=None):
    """The fused form on the traced records (which must end as after kr_post_line_dev_f64) and the reduce form on those (which it must not write)."""
    rays = records(name) if rays is None else rays
    post = post_records(name) if post is None else post
    pol = polar(name) if pol is None else pol
    words, after = fused(h, limb, pol_law, rays, INCL[name])
    assert after.tobytes() == post.tobytes(), (test, case)
    rule = against_the_rule(test, f"{case}-fused", h, words, post, pol, limb, pol_law, guard)
    again, after = reduced(h, limb, pol_law, post, INCL[name])
    assert after.tobytes() == post.tobytes(), (test, case)
    against_the_rule(test, f"{case}-reduce", h, again, post, pol, limb, pol_law, guard, rule)
    return words, again, rule[1]


# ---- 1. device against the numpy rule: both forms x four kinds of motion x five record sets, pol laws and limb laws ------------------------------
@pytest.mark.parametrize("kind", ["rigid", "shear", "retro", "static"])
@pytest.mark.parametrize("name", ["ip15", "ip16", "plane80", "plane30", "spoilt80"])
def test_device_against_the_rule(krlib, name, kind):
    traced = name not in ("ip15", "ip16")
    h = th.spot(wide=not traced, kind=kind, **th.grid(16))
    pol_law = CHANDRA if kind in ("rigid", "retro") else CONSTANT
    words, again, lo = both_forms("test_device_against_the_rule", f"{name}-{kind}", name, h, LAOR, pol_law, plane_guard if traced else fixture_guard)
    if name == "spoilt80":
        assert lo["bad_pol"] == 3                                                         # the guard against a vacuous bad-pol case
    host = api.reduce_hotspot_stokes(h, post_records(name), -SPIN, INCL[name], pol_law, limb=LAOR)          # the host-record form: the same kernel
    assert (host["on_disc"], host["used"], host["bad_pol"]) == tuple(int(w) for w in again[-4:-1])
    dev = api.hotspot_stokes_from_words(h, again)
    for k in hs.PLANES:
        assert hr.max_diff(host[k], dev[k]) <= 1e-12


@pytest.mark.parametrize("limb", sorted(LIMBS))
@pytest.mark.parametrize("pol_law", [CONSTANT, CHANDRA, (0, -0.3)], ids=["constant", "chandrasekhar", "negative"])
@pytest.mark.parametrize("name", ["ip16", "plane30", "spoilt80"])
def test_pol_laws_and_limb_laws(krlib, name, pol_law, limb):
    traced = name != "ip16"
    h = th.spot(wide=not traced, **th.grid(8))
    _, _, lo = both_forms("test_pol_laws_and_limb_laws", f"{name}-pol{pol_law[0]}{'n' if pol_law[1] < 0 else ''}-{limb}", name, h, LIMBS[limb], pol_law,
                          plane_guard if traced else fixture_guard)
    assert lo["bad_pol"] == (3 if name == "spoilt80" else 0)                              # bad-pol records add to nothing under EVERY limb law


@pytest.mark.parametrize("nt", [300, 1025])
@pytest.mark.parametrize("kind", ["shear", "retro", "static"])
def test_every_motion_with_the_sparsity_test_compiled_in(krlib, kind, nt):
    """Two and eight slots over 1.7 periods: the folded head must skip nothing that the rule counts, for Q and U as for the flux."""
    h = th.spot(kind=kind, nt=nt, periods=1.7, **th.grid(4))
    guard = lambda lo: plane_guard(lo) and (kind == "static" or lo["pairs"] < 0.9 * lo["used"] * nt)
    both_forms("test_every_motion_with_the_sparsity_test", f"plane80-{kind}-nt{nt}", "plane80", h, LAOR, CHANDRA, guard)


# ---- 2. shapes where the kernel can go wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 63, 64, 65, 256, 257, 512, 1024, 4096])
def test_every_sample_count(krlib, nt):
    """Two periods in nt samples on ip16 with the wide spot: every slot count of the kernel (1, 2, 4, 8, 16), full and partial waves."""
    h = th.spot(wide=True, nt=nt, periods=2.0, **th.grid(3 if nt > 1025 else 5))
    both_forms("test_every_sample_count", f"nt{nt}", "ip16", h, LAOR, CHANDRA, fixture_guard)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 512, 513, 769])
def test_every_record_count(krlib, n):
    src, post_all, pol_all = records("spoilt80"), post_records("spoilt80"), polar("spoilt80")
    h = th.spot(nt=65, **th.grid(7))
    first = int(np.flatnonzero(hr.disc_filter(h, post_all) & hr.ring(h, post_all))[0])      # begin at a record in the ring
    rays, post = np.ascontiguousarray(src[first:first + n]), np.ascontiguousarray(post_all[first:first + n])
    pol = {k: (v[first:first + n] if isinstance(v, np.ndarray) else v) for k, v in pol_all.items()}
    assert len(rays) == n
    if n == 0:
        L = api.lib()
        law, plaw = capi.limb_law("laor"), capi.pol_law(CHANDRA)
        nw = api.hotspot_stokes_words(h)
        with DeviceScope(L) as dev:
            out = dev.upload(np.full(nw, 7.0))
            capi.check(L, L.kr_post_hotspot_stokes_dev_f64(-SPIN, *POST, 0, -PI, PI, 80.0, C.byref(h), C.byref(law), C.byref(plaw), None, 0, out, None), "kr_post_hotspot_stokes")
            capi.check(L, L.kr_reduce_hotspot_stokes_dev_f64(-SPIN, *POST, 80.0, C.byref(h), C.byref(law), C.byref(plaw), None, 0, out, None), "kr_reduce_hotspot_stokes")
            assert (dev.fetch(out, nw) == 7.0).all()                                         # n == 0 adds nothing
        host = api.reduce_hotspot_stokes(h, post, -SPIN, 80.0, CHANDRA, limb=LAOR)
        assert not any(host[k].any() for k in hs.PLANES) and (host["on_disc"], host["used"], host["bad_pol"]) == (0, 0, 0)
        return
    guard = lambda lo: lo["used"] >= 1 and lo["p"].max() > 0
    both_forms("test_every_record_count", f"n{n}", "spoilt80", h, LAOR, CHANDRA, guard, rays, post, pol)


@pytest.mark.parametrize("where", ["none", "lds", "global"])
def test_spectrogram_on_both_sides_of_the_lds_budget(krlib, where):
    """ne = 0; a block of nt rows padded to ne | 1 words that just stays in LDS (nt (ne | 1) <= kHotSpecLdsWords) beside the larger Stokes items; and one
    row more, where the pairs add to global memory.  The spectrogram is intensity only."""
    ne = 0 if where == "none" else 64
    budget, stride = th.lds_limit(), ne | 1
    nt = 40 if where == "none" else budget // stride if where == "lds" else budget // stride + 1
    if ne:
        assert (nt * stride <= budget) == (where == "lds") and (nt + 1) * stride > budget
    h = th.spot(nt=nt, periods=1.5, line_energy=6.4, e_min=2.0, de=10.0 / ne, ne=ne) if ne else th.spot(nt=nt, periods=1.5)
    words, _, lo = both_forms("test_spectrogram_on_both_sides_of_the_lds_budget", f"ne{ne}-{where}-nt{nt}", "plane80", h, LAOR, CHANDRA,
                              lambda lo: plane_guard(lo) and (ne == 0 or (lo["spectrogram"] > 0).sum() > nt))
    assert len(words) == nt * (5 + ne) + 4
    if ne:
        assert len(set(hr.energy_index(h, post_records("plane80")["redshift"][lo["used_index"]]))) > 2


def test_a_spot_outside_the_disc(krlib):
    h = th.spot(nt=70, r_spot=2 * th.R_DISC, **th.grid(4))
    ref = hs.hotspot_stokes(h, post_records("plane30"), polar("plane30"), limb=LAOR, pol_law=CHANDRA)
    assert ref["on_disc"] > 500 and ref["used"] == 0
    words, _ = fused(h, LAOR, CHANDRA, records("plane30"), 30.0)
    assert int(words[-4]) == ref["on_disc"] and int(words[-3]) == 0 and not words[:-4].any()


# ---- 3. against the per-record polarisation pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plane80", "plane30"])
def test_q_and_u_are_the_sums_over_the_per_record_pass(krlib, name):
    """Q[k] = sum_i c_i delta_i c2_i s_ik and U[k] with s2, where c2 and s2 are what kr_polarisation_dev_f64 gives on the device for the same records
    and c, delta, s are the rule's."""
    post, pol = post_records(name), polar(name)
    per_record = api.polarisation(post, -SPIN, INCL[name])
    used = np.flatnonzero(hr.disc_filter(th.spot(), post) & hr.ring(th.spot(), post) & ~pol["bad"])
    assert len(used) > 100 and np.abs(per_record["c2"][used] - pol["c2"][used]).max() <= 1e-12
    mixed = dict(pol, c2=per_record["c2"], s2=per_record["s2"])
    h = th.spot(nt=96, periods=1.3)
    words, _ = fused(h, LAOR, CHANDRA, records(name), INCL[name])
    against_the_rule("test_q_and_u_are_the_sums_over_the_per_record_pass", name, h, words, post, mixed, LAOR, CHANDRA, plane_guard)


def test_the_flux_is_the_hotspot_pass_without_the_bad_pol_records(krlib):
    """flux, sx, sy and the spectrogram against kr_post_hotspot_dev_f64: equal where no record is bad-pol, and on the spoilt plane equal to that pass on
    the records with the three bad-pol ones taken out (they are not bad-angle for the law-0 pass, which would use them)."""
    h = th.spot(nt=80, periods=1.2, **th.grid(6))
    for name in ("plane30", "spoilt80"):
        rays, post, pol = records(name), post_records(name), polar(name)
        keep = ~(pol["bad"] & hr.disc_filter(h, post) & hr.ring(h, post))
        assert (~keep).sum() == (3 if name == "spoilt80" else 0)
        got = api.hotspot_stokes_from_words(h, fused(h, LAOR, CHANDRA, rays, INCL[name])[0])
        plain = api.hotspot_from_words(h, th.fused(h, LAOR, np.ascontiguousarray(rays[keep]))[0])
        assert got["used"] == plain["used"] > 100 and got["on_disc"] == plain["on_disc"] + int((~keep).sum())
        for k in hr.PLANES:
            assert hr.max_diff(got[k], plain[k]) <= 1e-12, (name, k)


# ---- 4. additivity -----------------------------------------------------------------------------------------------------------------------
def test_shards_and_repeated_calls_add_up(krlib):
    rays = records("spoilt80")
    h = th.spot(nt=130, periods=1.2, **th.grid(9))
    L = api.lib()
    law, plaw = capi.limb_law("laor"), capi.pol_law(CHANDRA)
    nw = api.hotspot_stokes_words(h)
    whole, _ = fused(h, LAOR, CHANDRA, rays, 80.0)
    b = api.hotspot_stokes_from_words(h, whole)
    assert b["used"] > 100 and b["bad_pol"] == 3 and np.hypot(b["q"], b["u"]).max() > 0
    half = len(rays) // 2 + 7
    with DeviceScope(L) as dev:
        out = dev.zeros(nw * 8)
        for part in (rays[:half], rays[half:]):
            d = dev.upload(np.ascontiguousarray(part))
            capi.check(L, L.kr_post_hotspot_stokes_dev_f64(-SPIN, *POST, 0, -PI, PI, 80.0, C.byref(h), C.byref(law), C.byref(plaw), d, len(part), out, None), "kr_post_hotspot_stokes")
        capi.check(L, L.kr_synchronize(None), "sync")
        both = dev.fetch(out, nw)
    assert np.array_equal(both[-4:], whole[-4:])
    a, twice = api.hotspot_stokes_from_words(h, both), api.hotspot_stokes_from_words(h, fused(h, LAOR, CHANDRA, rays, 80.0, calls=2)[0])
    assert (twice["on_disc"], twice["used"], twice["bad_pol"]) == (2 * b["on_disc"], 2 * b["used"], 2 * b["bad_pol"])
    scale = {k: hs.scale(dict(b, p=np.hypot(b["q"], b["u"])), k) for k in hs.PLANES}
    for k in hs.PLANES:
        assert np.abs(a[k] - b[k]).max() <= parity.BIN_RTOL * scale[k] and np.abs(twice[k] - 2 * b[k]).max() <= parity.BIN_RTOL * 2 * scale[k], k


def test_two_spots_add_up_under_a_limb_law(krlib):
    """The further spots go through the Stokes reduce form, which takes the limb law: the isotropic restriction of the plain light curve is gone."""
    ip, p = th.plane(30.0, 32), th.image_params()
    one, two = th.spot(nt=50, **th.grid(6)), th.spot(nt=50, kind="shear", phi0=2.5, sigma=1.0, **th.grid(6))
    a, b = (api.hotspot_lightcurve(ip, p, s, limb="laor", pol=CHANDRA) for s in (one, [two]))
    both = api.hotspot_lightcurve(ip, p, [one, two], limb="laor", pol=CHANDRA)
    assert a["used"] > 10 and b["used"] > 5 and np.abs(a["q"]).max() > 0 and np.abs(b["u"]).max() > 0
    assert (both["on_disc"], both["used"], both["bad_pol"]) == (a["on_disc"] + b["on_disc"], a["used"] + b["used"], a["bad_pol"] + b["bad_pol"])
    for k in hs.PLANES:
        top = max(np.abs(a[k]).max(), np.abs(b[k]).max())
        assert np.abs(both[k] - (a[k] + b[k])).max() <= parity.BIN_RTOL * top, k
    with pytest.raises(api.KrError, match="must share"):
        api.hotspot_lightcurve(ip, p, [one, th.spot(nt=51, **th.grid(6))], pol=CHANDRA)
    with pytest.raises(api.KrError, match="kr_post_hotspot_stokes: sigma must be positive"):
        api.hotspot_lightcurve(ip, p, th.spot(nt=50, sigma=-1.0), pol=CHANDRA)
    with pytest.raises(api.KrError, match="kr_reduce_hotspot_stokes: cut must be positive"):
        api.hotspot_lightcurve(ip, p, [one, th.spot(nt=50, cut=0.0, **th.grid(6))], pol=CHANDRA)
    with pytest.raises(api.KrError, match="kr_post_hotspot_stokes: pol coefficient must lie in"):
        api.hotspot_lightcurve(ip, p, one, pol=(0, 1.5))


# ---- 5. api.hotspot_lightcurve end to end, and the program ---------------------------------------------------------------------------------
@pytest.mark.parametrize("incl", [80.0, 30.0])
def test_api_hotspot_lightcurve_end_to_end(krlib, incl):
    h = th.spot(nt=60, **th.grid(10))
    plain = api.hotspot_lightcurve(th.plane(incl), th.image_params(), h, limb="laor")
    assert "q" not in plain and "bad_pol" not in plain and "bad_angle" in plain            # pol=None: the result dict of before
    res = api.hotspot_lightcurve(th.plane(incl), th.image_params(), h, limb="laor", pol=capi.pol_law(CHANDRA), return_records=True)
    rec = res["records"]
    assert len(rec) == 65 * 65 and "bad_angle" not in res
    words = np.concatenate([res[k] for k in hs.CURVES] + [res["spectrogram"].ravel(), [res["on_disc"], res["used"], res["bad_pol"], 0.0]])
    against_the_rule("test_api_hotspot_lightcurve_end_to_end", f"incl{incl:.0f}", h, words, rec, hs.polar(rec, -SPIN, incl), LAOR, CHANDRA, plane_guard)
    for k in hr.PLANES:
        assert hr.max_diff(res[k], plain[k]) <= 1e-12                                     # no bad-pol record on these planes: the intensity is the plain pass's
    lit = res["flux"] != 0
    assert lit.any() and np.isfinite(res["pol_degree"][lit]).all() and np.isnan(res["pol_degree"][~lit]).all() and np.isnan(res["pol_angle"][~lit]).all()
    assert (res["pol_degree"][lit] <= CHANDRA[1] * (1 + 1e-12)).all() and (np.abs(res["pol_angle"][lit]) <= PI / 2).all()
    assert np.allclose(res["pol_degree"][lit], np.hypot(res["q"], res["u"])[lit] / res["flux"][lit], rtol=1e-15, atol=0)


def test_program_equals_api(krlib, tmp_path):
    exe = os.path.join(th.ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_hotspot_lightcurve")
    assert os.path.exists(exe), "kr_hotspot_lightcurve not built (__graft_entry__.build())"
    out = tmp_path / "hotspot_stokes.dat"
    par = os.path.join(th.APPS, "hotspot_stokes.par")
    r = subprocess.run([exe, f"--parfile={par}", f"--outfile={out}"], capture_output=True, text=True, timeout=300, cwd=th.APPS)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(out).read()
    h = capi.hot_spot(10.0, 2.0, cut=3.0, phi0=0.5, spin=SPIN, t0=10000.0, nt=24, g_index=3.0, line_energy=6.4, e_min=3.0, de=(9.0 - 3.0) / 12, ne=12,
                      r_isco=th.r_isco(), r_disc=th.R_DISC)
    h.dt = 1.0 * (2 * PI / abs(h.omega)) / 24
    res = api.hotspot_lightcurve(th.plane(30.0, 32), th.image_params(), h, limb=LAOR, pol=CHANDRA)
    assert res["used"] > 30 and np.abs(res["q"]).max() > 0 and np.abs(res["u"]).max() > 0 and res["spectrogram"].max() > 0
    assert text == api.hotspot_text(res)
    lines = text.splitlines()
    assert len(lines) == 3 + 24 + 24 * 13 and lines[2].split()[:2] == ["#", "BAD_POL"] and len(lines[3].split()) == 6
    # without the keys: the file of before, byte for byte what api.hotspot_text gives for the plain result
    plain = subprocess.run([exe, f"--parfile={os.path.join(th.APPS, 'hotspot_lightcurve.par')}", f"--outfile={out}", "--incl=30"], capture_output=True, text=True,
                           timeout=300, cwd=th.APPS)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    old = open(out).read()
    assert old == api.hotspot_text(api.hotspot_lightcurve(th.plane(30.0, 32), th.image_params(), h, limb=LAOR))
    assert old.splitlines()[2].split()[:2] == ["#", "BAD_ANGLE"] and len(old.splitlines()[3].split()) == 4
    for a, b in zip(old.splitlines()[3:27], lines[3:27]):
        assert b.startswith(a)                                                               # the four columns of before, then Q U


# ---- 6. one physics check ------------------------------------------------------------------------------------------------------------------
def test_the_winding_number_of_the_stokes_loop_at_30_degrees(krlib):
    """(Q[k], U[k]) of a prograde spot at r = 10 over one period on the 30-degree plane: the device reproduces the integer that the rule gives on
    oracle-traced records (tests/test_hotspot_stokes_rules.py, which says why it is 0 there and 2 near face-on)."""
    h = th.spot(nt=64)
    post, pol = post_records("plane30"), polar("plane30")
    lo = hs.hotspot_stokes(h, post, pol, pol_law=CONSTANT)
    assert plane_guard(lo) and np.hypot(lo["q"], lo["u"]).min() > 0.1 * lo["p"].max()
    assert hs.winding_number(lo["q"], lo["u"]) == WINDING_AT_30_DEGREES
    got = hs.from_words(h, fused(h, "isotropic", CONSTANT, records("plane30"), 30.0)[0])
    assert got["used"] == lo["used"]
    assert hs.winding_number(got["q"], got["u"]) == WINDING_AT_30_DEGREES
    retro = hs.from_words(h, reduced(th.spot(nt=64, kind="retro"), "isotropic", CONSTANT, post, 30.0)[0])
    assert hs.winding_number(retro["q"], retro["u"]) == -1 * WINDING_AT_30_DEGREES
