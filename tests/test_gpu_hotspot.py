"""GPU: the orbiting hot spot (kr_hotspot; kr_post_hotspot_dev_f64, kr_reduce_hotspot_dev_f64, kr_reduce_hotspot_f64, api.hotspot_lightcurve,
apps/kr_hotspot_lightcurve) against the numpy rule of tests/hotspot_rules.py, the line pass it extends, and itself.

The bar.  Tallies are exact.  The sums -- flux, sx, sy and the spectrogram, each as a whole -- stay within max(16 x noise, floor) of the float64 rule,
where `noise` is the rule's own float64 - longdouble difference on the same records and both differences are normalised by the largest magnitude of the
plane.  Not element-wise: a sample near a zero of the shifted Gaussian is a small difference of nearly equal numbers, and no zero pattern is asserted.
`floor` is what the number format alone allows (hot_floor below), derived, not tuned.  Every case goes through parity.record_margin.

Records: the fixtures ip15 and ip16 (traced, not yet redshifted) and a 65 x 65 ray plane at 80 and at 30 degrees, traced once per session."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import angle_rules as ar
import golden_cases as gc
import hotspot_rules as hr
import parity
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPS = os.path.join(ROOT, "tests", "golden", "apps")
PI = math.pi
SPIN, DIST, R_DISC = 0.998, 10000.0, 30.0
POST = (-1.0, 1, 0)                       # V, reverse, projradius of an image plane's redshift pass
EPS = 2.0 ** -52
LAOR = (1, 2.06)


def r_isco():
    return api.lib().kr_kerr_isco(SPIN, 1)


def lds_limit():
    """The LDS budget of the spectrogram block in doubles, from the kernel's own source; a block of nt rows of (ne | 1) words stays in LDS up to it."""
    text = open(os.path.join(ROOT, "raytrace_cpu_amd", "csrc", "kr_hotspot.hip")).read()
    return int(re.search(r"constexpr int kHotSpecLdsWords = (\d+);", text).group(1))


def plane(incl, nx=64):
    s = capi.ImagePlaneSpec()
    d = 2 * R_DISC / nx
    s.dist, s.inc_deg, s.x0, s.xmax, s.dx, s.y0, s.ymax, s.dy, s.spin, s.phi0, s.precision = DIST, incl, -R_DISC, R_DISC, d, -R_DISC, R_DISC, d, SPIN, 0.0, 100.0
    return s


def image_params():
    p = capi.default_params(-SPIN)
    p.precision, p.integrator, p.theta_max, p.r_max = 100.0, capi.RK4, PI / 2, 1.1 * DIST
    p.stop_kind, p.flags = capi.STOP_THETA, capi.FLAG_HYBRID
    return p


def spot(wide=False, kind="rigid", nt=48, periods=1.0, **kw):
    """r_spot = 10, sigma = 1.5 (the traced planes) or the wide spot r_spot = 15, sigma = 4 (the fixtures' few rays); kind: rigid (Keplerian), shear,
    retro (omega < 0) or static (omega = 0).  The nt samples span `periods` Keplerian periods from t0 = DIST, about a ray's own travel time."""
    args = dict(r_spot=15.0, sigma=4.0) if wide else dict(r_spot=10.0, sigma=1.5)
    args.update(cut=3.0, phi0=0.4, spin=SPIN, t0=DIST, nt=nt, g_index=4.0, r_isco=r_isco(), r_disc=R_DISC)
    args.update(kw)
    h = capi.hot_spot(**args)
    if "dt" not in kw:
        h.dt = periods * (2 * PI * (SPIN + h.r_spot ** 1.5)) / nt
    if kind == "shear":
        h.shear = 1
    elif kind == "retro":
        h.omega = -1 * h.omega
    elif kind == "static":
        h.omega = 0.0
    return h


def grid(ne):
    """Energy bins that hold every ray of these discs (g from 0.1 to 1.6 of a 6.4 line)."""
    return dict(line_energy=6.4, e_min=0.5, de=(64.0 - 0.5) / ne, ne=ne) if ne else {}


_RECORDS = {}


def records(name):
    """Traced records that have not been through the redshift pass: the fixtures' final__rk4, or a 65 x 65 plane traced here (its records come back
    after a pass that rewrites only redshift and phi, which the passes under test compute again from the fields it left alone; wrapping is idempotent)."""
    if name not in _RECORDS:
        if name in ("ip15", "ip16"):
            _RECORDS[name] = np.ascontiguousarray(np.load(gc.golden_path(name))["final__rk4"])
        else:
            res = api.hotspot_lightcurve(plane({"plane80": 80.0, "plane30": 30.0}[name]), image_params(), spot(nt=4), return_records=True)
            assert len(res["records"]) == 65 * 65 and res["on_disc"] > 500
            _RECORDS[name] = res["records"]
    return _RECORDS[name]


_POST = {}


def post_line_records(name_or_rays):
    """rays[] after kr_post_line_dev_f64, and its line with g_index = 3, a flat emissivity and an energy range that holds every ray."""
    key = name_or_rays if isinstance(name_or_rays, str) else None
    if key in _POST:
        return _POST[key]
    rays = records(key) if key else name_or_rays
    L = api.lib()
    b = capi.line_bins(line_energy=1.0, e_min=1e-3, de=1.2, ne=80, log_e=True, r_isco=r_isco(), r_disc=R_DISC, q1=0.0, rb1=4.0, q2=0.0, rb2=10.0, q3=0.0, g_index=3.0)
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(api.line_words(b) * 8)
        capi.check(L, L.kr_post_line_dev_f64(-SPIN, *POST, 0, -PI, PI, C.byref(b), d, len(rays), h, None), "kr_post_line")
        out = dev.fetch(d, len(rays), rays.dtype), api.line_from_words(b, dev.fetch(h, api.line_words(b)))
    if key:
        _POST[key] = out
    return out


def fused(h, law, rays, calls=1, motion=0):
    """kr_post_hotspot_dev_f64 `calls` times into one zeroed buffer, each on a fresh device copy of `rays`: (words, records after)."""
    L = api.lib()
    law = capi.limb_law(law)
    nw = api.hotspot_words(h)
    with DeviceScope(L) as dev:
        out = dev.zeros(nw * 8)
        after = rays
        for _ in range(calls):
            with DeviceScope(L) as one:
                d = one.upload(rays) if len(rays) else None
                capi.check(L, L.kr_post_hotspot_dev_f64(-SPIN, *POST, motion, -PI, PI, C.byref(h), C.byref(law), d, len(rays), out, None), "kr_post_hotspot")
                capi.check(L, L.kr_synchronize(None), "sync")
                after = one.fetch(d, len(rays), rays.dtype) if len(rays) else rays
        return dev.fetch(out, nw), after


def reduced(h, rays):
    """kr_reduce_hotspot_dev_f64 on a device copy of records that carry their redshift: (words, records after)."""
    L = api.lib()
    nw = api.hotspot_words(h)
    with DeviceScope(L) as dev:
        out = dev.zeros(nw * 8)
        d = dev.upload(rays) if len(rays) else None
        capi.check(L, L.kr_reduce_hotspot_dev_f64(C.byref(h), d, len(rays), out, None), "kr_reduce_hotspot")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(out, nw), (dev.fetch(d, len(rays), rays.dtype) if len(rays) else rays)


_ANGLES = {}


def angles(name_or_rays):
    key = name_or_rays if isinstance(name_or_rays, str) else None
    if key in _ANGLES:
        return _ANGLES[key]
    f = ar.frame(records(key) if key else name_or_rays, -SPIN, *POST)
    out = ar.mu_chi(f)[0], ar.bad_angle(f)
    if key:
        _ANGLES[key] = out
    return out


def hot_floor(h, rec, used_index):
    """What the number format alone allows, in units of the largest value of a plane.  A term c s carries
      the angle      phi - (phi0 + Om (T - t)) is built from four operations on magnitudes up to A = |Om| max |T_k - t| + |phi0| + pi, so up to 4 ulp of A,
                     and d s / d angle = (r r_spot / sigma^2) sin(.) exp(.) <= S = r r_spot / sigma^2:   4 A S
      the cosine     2 ulp of a value <= 1, times d d2 / d cos = 2 r r_spot, times 1 / (2 sigma^2):       2 S
      the exponent   d2 / (2 sigma^2) <= cut^2 / 2 with the reciprocal rounded once and the product (2 ulp): cut^2
      pow, exp, the subtraction and the two products: about 8 ulp
      the sum        up to `used` terms taken one after the other: used / 2
    (4 A S + 2 S + cut^2 + 8 + used / 2) ulp, doubled for the rule's own error."""
    if len(used_index) == 0:
        return 0.0
    r, t = rec["r"][used_index], rec["t"][used_index]
    T = hr.times(h)
    Om = np.abs(hr.pattern_speed(h, r)).max()
    A = Om * max(np.abs(T.max() - t).max(), np.abs(T.min() - t).max()) + abs(h.phi0) + PI
    S = r.max() * h.r_spot / (h.sigma * h.sigma)
    return 2 * (4 * A * S + 2 * S + h.cut * h.cut + 8 + len(used_index) / 2) * EPS


def against_the_rule(test, case, h, words, rec, law=(0, 0.0), mu=None, bad=None, guard=lambda lo: lo["flux"].max() > 0):
    """The guard on the rule's output first (a vacuous case fails as vacuous), then tallies exact and every plane within max(16 x noise, floor) of the
    float64 rule; returns the float64 rule's result."""
    noise, lo, hi = hr.noise(h, rec, law=law[0], coeff=law[1], mu=mu, bad=bad)
    assert guard(lo), (test, case, "vacuous", lo["on_disc"], lo["used"], float(lo["flux"].max()))
    got = api.hotspot_from_words(h, words)
    assert (got["on_disc"], got["used"], got["bad_angle"]) == (lo["on_disc"], lo["used"], lo["bad_angle"]), (test, case)
    assert words[-1] == 0.0, (test, case)
    floor = hot_floor(h, rec, lo["used_index"])
    worst = 0.0
    for k in hr.PLANES:
        diff = hr.max_diff(got[k], lo[k])
        allowed = max(16 * noise[k], floor)
        print(f"{test} {case} {k}: used {got['used']} pairs {lo['pairs']}; noise {noise[k]:.3e}, floor {floor:.3e}, device - rule {diff:.3e}, "
              f"device - longdouble rule {hr.max_diff(got[k], hi[k]):.3e}")
        parity.record_margin(test, f"{case}-{k}", {"n_traced": int(len(rec)), "n_bad": 0, "frac_bad": 0.0, "worst_ok": diff}, allowed=allowed, noise=noise[k], floor=floor,
                             device_minus_rule=diff, device_minus_longdouble_rule=hr.max_diff(got[k], hi[k]), used=got["used"], pairs=lo["pairs"], nt=int(h.nt), ne=int(h.ne))
        assert diff <= allowed, (test, case, k, diff, noise[k], floor)
        worst = max(worst, diff)
    return lo


# ---- 1. device against the numpy rule: fused (laor) and reduce forms x four kinds of motion x four record sets -------------------------------------------
@pytest.mark.parametrize("kind", ["rigid", "shear", "retro", "static"])
@pytest.mark.parametrize("name", ["ip15", "ip16", "plane80", "plane30"])
def test_device_against_the_rule(krlib, name, kind):
    traced = name.startswith("plane")
    h = spot(wide=not traced, kind=kind, **grid(16))
    rays = records(name)
    post, _ = post_line_records(name)
    mu, bad = angles(name)
    guard = (lambda lo: lo["used"] > 100 and lo["flux"].max() > 0) if traced else (lambda lo: lo["used"] > 20 and lo["flux"].max() > 0)
    words, after = fused(h, LAOR, rays)
    assert after.tobytes() == post.tobytes()                                              # rays[] as after kr_post_line_dev_f64
    against_the_rule("test_device_against_the_rule", f"{name}-{kind}-fused-laor", h, words, post, LAOR, mu, bad, guard)
    words, after = reduced(h, post)
    assert after.tobytes() == post.tobytes()                                              # the reduce form never writes
    against_the_rule("test_device_against_the_rule", f"{name}-{kind}-reduce", h, words, post, guard=guard)
    host = api.reduce_hotspot(h, post)                                                    # the host-record form: the same kernel
    assert (host["on_disc"], host["used"], host["bad_angle"]) == tuple(int(w) for w in words[-4:-1])
    dev = api.hotspot_from_words(h, words)
    for k in hr.PLANES:
        assert hr.max_diff(host[k], dev[k]) <= 1e-12


@pytest.mark.parametrize("nt", [300, 1025])
@pytest.mark.parametrize("kind", ["shear", "retro", "static"])
@pytest.mark.parametrize("name", ["ip16", "plane80"])
def test_every_motion_with_the_sparsity_test_compiled_in(krlib, name, kind, nt):
    """From two samples per lane the kernel skips pairs by the folded head {psi, om, half}: the per-item om of a sheared spot, a negative om and om = 0
    must skip nothing that the rule counts.  Two and eight slots, 1.7 periods (so the samples are not commensurate with the orbit)."""
    traced = name.startswith("plane")
    h = spot(wide=not traced, kind=kind, nt=nt, periods=1.7, **grid(4))
    rays = records(name)
    post, _ = post_line_records(name)
    mu, bad = angles(name)
    guard = lambda lo: lo["used"] > (100 if traced else 20) and lo["flux"].max() > 0 and (kind == "static" or lo["pairs"] < 0.9 * lo["used"] * nt)
    words, _ = fused(h, LAOR, rays)
    against_the_rule("test_every_motion_with_the_sparsity_test", f"{name}-{kind}-nt{nt}-fused", h, words, post, LAOR, mu, bad, guard)
    words, _ = reduced(h, post)
    against_the_rule("test_every_motion_with_the_sparsity_test", f"{name}-{kind}-nt{nt}-reduce", h, words, post, guard=guard)


# ---- 2. shapes where the kernel can go wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 63, 64, 65, 255, 256, 257, 1025, 4096])
def test_every_sample_count(krlib, nt):
    """Two periods in nt samples on ip16 with the wide spot: every slot count of the kernel, full and partial waves."""
    rays = records("ip16")
    post, _ = post_line_records("ip16")
    mu, bad = angles("ip16")
    h = spot(wide=True, nt=nt, periods=2.0, **grid(3 if nt > 1025 else 5))
    words, after = fused(h, LAOR, rays)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_every_sample_count", f"nt{nt}-fused", h, words, post, LAOR, mu, bad, lambda lo: lo["used"] > 20 and lo["flux"].max() > 0)
    words, _ = reduced(h, post)
    against_the_rule("test_every_sample_count", f"nt{nt}-reduce", h, words, post, guard=lambda lo: lo["used"] > 20 and lo["flux"].max() > 0)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3 * 256 + 1])
def test_every_record_count(krlib, n):
    src = records("plane80")
    post_all, _ = post_line_records("plane80")
    h = spot(nt=65, **grid(7))
    first = int(np.flatnonzero(hr.disc_filter(h, post_all) & hr.ring(h, post_all))[0])      # begin at a record in the ring
    rays, post = np.ascontiguousarray(src[first:first + n]), np.ascontiguousarray(post_all[first:first + n])
    assert len(rays) == n
    if n == 0:
        L = api.lib()
        with DeviceScope(L) as dev:
            out = dev.upload(np.full(api.hotspot_words(h), 7.0))
            law = capi.limb_law("laor")
            capi.check(L, L.kr_post_hotspot_dev_f64(-SPIN, *POST, 0, -PI, PI, C.byref(h), C.byref(law), None, 0, out, None), "kr_post_hotspot")
            capi.check(L, L.kr_reduce_hotspot_dev_f64(C.byref(h), None, 0, out, None), "kr_reduce_hotspot")
            assert (dev.fetch(out, api.hotspot_words(h)) == 7.0).all()                      # n == 0 adds nothing
        host = api.reduce_hotspot(h, post)
        assert not host["flux"].any() and not host["spectrogram"].any() and (host["on_disc"], host["used"], host["bad_angle"]) == (0, 0, 0)
        return
    mu, bad = angles(rays)
    guard = lambda lo: lo["used"] >= 1 and lo["flux"].max() > 0
    words, after = fused(h, LAOR, rays)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_every_record_count", f"n{n}-fused", h, words, post, LAOR, mu, bad, guard)
    words, after = reduced(h, post)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_every_record_count", f"n{n}-reduce", h, words, post, guard=guard)


def test_tiles_without_rays_and_with_only_the_last_lane(krlib):
    """Three tiles of 256 records: in the first no ray is in the ring, in the second only the last lane's is, the third is as traced."""
    src = records("plane80")
    post_all, _ = post_line_records("plane80")
    h = spot(nt=300, periods=2.0, **grid(5))
    on = hr.disc_filter(h, post_all) & hr.ring(h, post_all)
    last = next(j for j in np.flatnonzero(on) if j >= 511 and j + 257 <= len(src) and on[j + 1:j + 257].sum() > 10)      # the record of lane 255 of the second tile
    rays = src[last - 511:last + 257].copy()                                                    # (a copy: the session's records stay as traced)
    dead = np.ones(768, dtype=bool)
    dead[511:] = False
    rays["steps"][dead] = -1 * np.abs(rays["steps"][dead])                                      # steps <= 0: filtered
    assert rays["steps"][511] > 0
    post, _ = post_line_records(rays)
    f = hr.disc_filter(h, post) & hr.ring(h, post)
    assert not f[:256].any() and list(np.flatnonzero(f[256:512])) == [255] and f[512:].sum() > 10
    mu, bad = angles(rays)
    words, after = fused(h, LAOR, rays)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_tiles", "fused", h, words, post, LAOR, mu, bad, lambda lo: lo["used"] > 11 and lo["flux"].max() > 0)
    words, _ = fused(h, LAOR, np.ascontiguousarray(rays[:512]))
    assert int(words[-4]) == 1 and int(words[-3]) == 1
    words, _ = fused(h, LAOR, np.ascontiguousarray(rays[:256]))
    assert not words.any()


@pytest.mark.parametrize("ne", [0, 1, 7, 64])
def test_every_energy_count(krlib, ne):
    rays = records("plane30")
    post, _ = post_line_records("plane30")
    mu, bad = angles("plane30")
    h = spot(nt=40, **grid(ne))
    words, _ = fused(h, LAOR, rays)
    assert len(words) == 40 * (3 + ne) + 4
    lo = against_the_rule("test_every_energy_count", f"ne{ne}", h, words, post, LAOR, mu, bad, lambda lo: lo["used"] > 100 and lo["flux"].max() > 0)
    if ne:
        assert hr.max_diff(api.hotspot_from_words(h, words)["spectrogram"].sum(axis=1), lo["flux"]) <= 1e-12      # identity (d) on the device


@pytest.mark.parametrize("ne", [7, 64])
@pytest.mark.parametrize("where", ["lds", "global"])
def test_spectrogram_on_both_sides_of_the_lds_budget(krlib, ne, where):
    """The block of nt rows, each padded to ne | 1 words, stays in LDS up to kHotSpecLdsWords; one row more and the pairs add to global memory."""
    budget, stride = lds_limit(), ne | 1
    nt = budget // stride if where == "lds" else budget // stride + 1
    assert (nt * stride <= budget) == (where == "lds") and (nt + 1) * stride > budget
    rays = records("plane80")
    post, _ = post_line_records("plane80")
    mu, bad = angles("plane80")
    h = spot(nt=nt, periods=1.5, line_energy=6.4, e_min=2.0, de=10.0 / ne, ne=ne)            # bins fine enough for the rays to spread over several
    words, _ = fused(h, LAOR, rays)
    lo = against_the_rule("test_spectrogram_on_both_sides_of_the_lds_budget", f"ne{ne}-{where}-nt{nt}", h, words, post, LAOR, mu, bad,
                          lambda lo: lo["used"] > 100 and (lo["spectrogram"] > 0).sum() > nt)
    assert len(set(hr.energy_index(h, post["redshift"][lo["used_index"]]))) > 2
    words, _ = reduced(h, post)
    against_the_rule("test_spectrogram_on_both_sides_of_the_lds_budget", f"ne{ne}-{where}-nt{nt}-reduce", h, words, post, guard=lambda lo: lo["used"] > 100)


def test_a_ray_off_the_energy_grid_adds_to_the_light_curve_only(krlib):
    rays = records("plane80")
    post, _ = post_line_records("plane80")
    mu, bad = angles("plane80")
    narrow = spot(nt=40, line_energy=6.4, e_min=0.5, de=0.5, ne=11)                             # E up to 6: the blue-shifted rays fall off the grid
    whole = spot(nt=40, **grid(16))
    words, _ = fused(narrow, LAOR, rays)
    lo = against_the_rule("test_off_grid", "plane80", narrow, words, post, LAOR, mu, bad, lambda lo: lo["used"] > 100 and lo["flux"].max() > 0)
    ie = hr.energy_index(narrow, post["redshift"][lo["used_index"]])
    assert (ie < 0).any() and (ie >= 0).any()
    got, ref = api.hotspot_from_words(narrow, words), api.hotspot_from_words(whole, fused(whole, LAOR, rays)[0])
    assert hr.max_diff(got["flux"], ref["flux"]) <= 1e-12                                      # the light curve does not know the grid
    assert got["spectrogram"].sum() < 0.99 * got["flux"].sum()


def test_a_spot_outside_the_disc(krlib):
    rays = records("plane30")
    h = spot(nt=70, r_spot=2 * R_DISC, **grid(4))
    ref = hr.hotspot(h, post_line_records("plane30")[0])
    assert ref["on_disc"] > 500 and ref["used"] == 0
    words, _ = fused(h, LAOR, rays)
    assert int(words[-4]) == ref["on_disc"] and int(words[-3]) == 0 and not words[:-4].any()


# ---- 3. additivity -----------------------------------------------------------------------------------------------------------------------
def test_two_shards_add_up_to_one_call(krlib):
    rays = records("plane30")
    h = spot(nt=130, periods=1.2, **grid(9))
    L = api.lib()
    law = capi.limb_law("laor")
    nw = api.hotspot_words(h)
    whole, _ = fused(h, "laor", rays)
    assert whole[-3] > 100 and whole[:h.nt].max() > 0
    half = len(rays) // 2 + 7
    with DeviceScope(L) as dev:
        out = dev.zeros(nw * 8)
        for part in (rays[:half], rays[half:]):
            d = dev.upload(np.ascontiguousarray(part))
            capi.check(L, L.kr_post_hotspot_dev_f64(-SPIN, *POST, 0, -PI, PI, C.byref(h), C.byref(law), d, len(part), out, None), "kr_post_hotspot")
        capi.check(L, L.kr_synchronize(None), "sync")
        both = dev.fetch(out, nw)
    assert np.array_equal(both[-4:], whole[-4:])
    a, b, twice = api.hotspot_from_words(h, both), api.hotspot_from_words(h, whole), api.hotspot_from_words(h, fused(h, "laor", rays, calls=2)[0])
    assert (twice["on_disc"], twice["used"], twice["bad_angle"]) == (2 * b["on_disc"], 2 * b["used"], 2 * b["bad_angle"])
    for k in hr.PLANES:
        assert hr.max_diff(a[k], b[k]) <= parity.BIN_RTOL and hr.max_diff(twice[k], 2 * b[k]) <= parity.BIN_RTOL


def test_two_spots_add_up(krlib):
    ip, p = plane(80.0, 32), image_params()
    one, two = spot(nt=50, **grid(6)), spot(nt=50, kind="shear", phi0=2.5, sigma=1.0, **grid(6))
    a, b = api.hotspot_lightcurve(ip, p, one), api.hotspot_lightcurve(ip, p, [two])
    both = api.hotspot_lightcurve(ip, p, [one, two])
    assert a["used"] > 10 and b["used"] > 5 and a["flux"].max() > 0 and b["flux"].max() > 0
    assert (both["on_disc"], both["used"]) == (a["on_disc"] + b["on_disc"], a["used"] + b["used"])
    for k in hr.PLANES:
        assert hr.max_diff(both[k], a[k] + b[k]) <= parity.BIN_RTOL
    with pytest.raises(api.KrError):
        api.hotspot_lightcurve(ip, p, [one, two], limb="laor")
    for other in (spot(nt=50, t0=DIST + 1.0, **grid(6)), spot(nt=50, periods=2.0, **grid(6)), spot(nt=50, **grid(6) | {"e_min": 0.6}), spot(nt=50), spot(nt=51, **grid(6))):
        with pytest.raises(api.KrError, match="must share"):                                  # other times or another grid would be mislabelled
            api.hotspot_lightcurve(ip, p, [one, other])
    for bad, why in ((spot(nt=50, sigma=-1.0), "kr_post_hotspot: sigma must be positive"), (spot(nt=5000), "kr_post_hotspot: nt must be in 1 ... 4096")):
        with pytest.raises(api.KrError, match=re.escape(why)):
            api.hotspot_lightcurve(ip, p, bad)
    with pytest.raises(api.KrError, match=re.escape("kr_reduce_hotspot: cut must be positive")):
        api.hotspot_lightcurve(ip, p, [one, spot(nt=50, cut=0.0, **grid(6))])


# ---- 4. against an independent existing pass, and the identities on the device -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ip16", "plane80", "plane30"])
def test_flat_static_limit_equals_the_line_pass_flux(krlib, name):
    """Identity (a): sigma = 1e8, cut = 40, omega = 0, g_index = 3 -- s = 1 to 1e-13 and every disc ray is in the ring, so flux[k] is the sum of g^-3:
    the flux plane of kr_post_line_dev_f64 with q1 = q2 = q3 = 0 (emissivity 1), summed over a grid that holds every ray."""
    rays = records(name)
    post, line = post_line_records(name)
    assert line["binned"] == line["on_disc"] > 30
    h = spot(nt=70, sigma=1e8, cut=40.0, omega=0.0, dt=1.0, g_index=3.0)
    words, _ = fused(h, "isotropic", rays)
    got = api.hotspot_from_words(h, words)
    want = line["flux"].sum()
    worst = float(np.abs(got["flux"] / want - 1).max())
    print(f"{name}: flat static spot against the line pass's flux plane: {worst:.2e}")
    assert got["on_disc"] == line["on_disc"] == got["used"]
    assert worst <= parity.BIN_RTOL


def test_periodicity_and_covariance_on_the_device(krlib):
    """Identities (b) and (c), to the floor: flux[k + m] = flux[k] with dt = P / m; (t0 + delta, phi0 - omega delta) gives the curve of (t0, phi0).
    (hot_floor is one evaluation's error doubled: what the difference of two device evaluations can carry.)  The figures go to the margins file."""
    rays = records("plane80")
    post, _ = post_line_records("plane80")
    m = 40
    h = spot(nt=2 * m, periods=2.0)
    a = api.hotspot_from_words(h, fused(h, LAOR, rays)[0])
    floor = hot_floor(h, post, np.flatnonzero(hr.disc_filter(h, post) & hr.ring(h, post)))
    assert a["used"] > 100 and a["flux"].max() > 0 and 0 < floor < 1e-9

    def held(case, k, got, want):
        diff = hr.max_diff(got, want)
        print(f"test_periodicity_and_covariance_on_the_device {case} {k}: floor {floor:.3e}, device - device {diff:.3e}")
        parity.record_margin("test_periodicity_and_covariance_on_the_device", f"{case}-{k}", {"n_traced": int(len(post)), "n_bad": 0, "frac_bad": 0.0, "worst_ok": diff},
                             allowed=floor, noise=0.0, floor=floor, device_minus_rule=diff, device_minus_longdouble_rule=diff, used=a["used"], pairs=0, nt=int(h.nt),
                             ne=int(h.ne))
        assert diff <= floor, (case, k, diff, floor)

    for k in ("flux", "sx", "sy"):
        held("periodicity", k, a[k][m:], a[k][:m])
    delta = 17.25
    moved = spot(nt=2 * m, periods=2.0, t0=DIST + delta, phi0=0.4 - h.omega * delta)
    b = api.hotspot_from_words(moved, fused(moved, LAOR, rays)[0])
    for k in ("flux", "sx", "sy"):
        held("covariance", k, b[k], a[k])
    still = spot(nt=2 * m, periods=2.0, t0=DIST + delta)
    assert hr.max_diff(api.hotspot_from_words(still, fused(still, LAOR, rays)[0])["flux"], a["flux"]) > 1e-3


# ---- 5. limb laws ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ip15", "plane80"])
def test_limb_laws(krlib, name):
    traced = name.startswith("plane")
    rays, h = records(name), spot(wide=not traced, **grid(8))
    post, _ = post_line_records(name)
    mu, bad = angles(name)
    res = {}
    for law_name, (law_id, coeff) in capi.LIMB_LAWS.items():
        words, after = fused(h, (law_id, coeff), rays)
        assert after.tobytes() == post.tobytes()
        against_the_rule("test_limb_laws", f"{name}-{law_name}", h, words, post, (law_id, coeff), mu, bad, lambda lo: lo["used"] > 20 and lo["flux"].max() > 0)
        assert int(words[-2]) == int((bad & hr.disc_filter(h, post)).sum())
        res[law_id] = words
    iso, _ = reduced(h, post)
    assert np.array_equal(iso[-4:-2], res[0][-4:-2]) and iso[-2] == 0
    a, b = api.hotspot_from_words(h, res[0]), api.hotspot_from_words(h, iso)
    for k in hr.PLANES:
        assert hr.max_diff(a[k], b[k]) <= 1e-12                                                # law 0: the reduce form on the post-pass records
    assert not np.array_equal(res[1][:h.nt], res[0][:h.nt]) and not np.array_equal(res[2][:h.nt], res[0][:h.nt])


def test_bad_angle_rays_are_left_out_under_a_law_that_needs_them(krlib):
    """ps_h10/euler seen with reverse = 0 carries bad-angle rays on the disc (tests/test_gpu_angles.py): counted under every law, used only under law 0."""
    rays = np.ascontiguousarray(np.load(gc.golden_path("ps_h10"))["final__euler"])
    spin = gc.cases()["ps_h10"]["runs"]["euler"].spin
    h = capi.hot_spot(250.0, 1e8, cut=40.0, omega=0.0, t0=0.0, dt=1.0, nt=5, g_index=3.0, r_isco=gc.r_isco(), r_disc=500.0)      # flat: every disc ray is used
    L = api.lib()
    f = ar.frame(rays, spin, -1.0, 0, 0)
    mu, bad = ar.mu_chi(f)[0], ar.bad_angle(f)
    nw = api.hotspot_words(h)
    res = {}
    for law_id in (0, 1):
        law = capi.limb_law((law_id, 2.06))
        with DeviceScope(L) as dev:
            d, out = dev.upload(rays), dev.zeros(nw * 8)
            capi.check(L, L.kr_post_hotspot_dev_f64(spin, -1.0, 0, 0, 0, -PI, PI, C.byref(h), C.byref(law), d, len(rays), out, None), "kr_post_hotspot")
            post, words = dev.fetch(d, len(rays), rays.dtype), dev.fetch(out, nw)
        against_the_rule("test_bad_angle_rays", f"ps_h10-euler-law{law_id}", h, words, post, (law_id, 2.06), mu, bad, lambda lo: lo["used"] > 12 and lo["flux"].max() > 0)
        res[law_id] = words
    assert res[0][-2] == res[1][-2] == 12 and res[0][-4] == res[1][-4]
    assert 0 < res[0][-3] - res[1][-3] <= 12 and np.isfinite(res[1]).all()


def test_motion_1_takes_the_plain_redshift(krlib):
    rays = records("ip16")
    L = api.lib()
    b = capi.line_bins(line_energy=1.0, e_min=1e-3, de=1.2, ne=80, log_e=True, r_isco=r_isco(), r_disc=R_DISC)
    with DeviceScope(L) as dev:
        d, out = dev.upload(rays), dev.zeros(api.line_words(b) * 8)
        capi.check(L, L.kr_post_line_dev_f64(-SPIN, 0.1, 1, 0, 1, -PI, PI, C.byref(b), d, len(rays), out, None), "kr_post_line")
        post = dev.fetch(d, len(rays), rays.dtype)
    h = spot(wide=True)
    law = capi.limb_law("isotropic")
    nw = api.hotspot_words(h)
    with DeviceScope(L) as dev:
        d, out = dev.upload(rays), dev.zeros(nw * 8)
        capi.check(L, L.kr_post_hotspot_dev_f64(-SPIN, 0.1, 1, 0, 1, -PI, PI, C.byref(h), C.byref(law), d, len(rays), out, None), "kr_post_hotspot")
        after, words = dev.fetch(d, len(rays), rays.dtype), dev.fetch(out, nw)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_motion_1_takes_the_plain_redshift", "ip16", h, words, post, guard=lambda lo: lo["used"] > 10 and lo["flux"].max() > 0)


# ---- 6. one physical sanity check --------------------------------------------------------------------------------------------------------
def mean_energy(res, k):
    row = res["spectrogram"][k]
    return float((row * res["energy"]).sum() / row.sum())


def test_the_bright_phase_is_the_blue_phase(krlib):
    """80 degrees, r_spot = 10, one period: the flux-weighted mean observed energy of the spectrogram row at the brightest sample exceeds that at the
    faintest sample that still has flux (Doppler boosting: bright = approaching).  Asserted on the rule first, then on the device."""
    rays = records("plane80")
    post, _ = post_line_records("plane80")
    h = spot(nt=32, **grid(64))
    lo = hr.hotspot(h, post)
    lo["energy"] = api.hotspot_energies(h)
    lit = np.flatnonzero(lo["flux"] != 0)
    assert (lo["spectrogram"].sum(axis=1)[lit] > 0).all()                                     # the grid holds every ray: a lit sample has a mean energy
    bright, faint = int(np.argmax(lo["flux"])), int(lit[np.argmin(lo["flux"][lit])])
    print(f"rule: brightest sample {bright} (flux {lo['flux'][bright]:.3e}, <E> {mean_energy(lo, bright):.3f}), faintest lit sample {faint} "
          f"(flux {lo['flux'][faint]:.3e}, <E> {mean_energy(lo, faint):.3f})")
    assert lo["used"] > 100 and bright != faint
    assert mean_energy(lo, bright) > mean_energy(lo, faint)
    got = api.hotspot_from_words(h, reduced(h, post)[0])
    assert int(np.argmax(got["flux"])) == bright
    assert mean_energy(got, bright) > mean_energy(got, faint)
    assert abs(mean_energy(got, bright) - mean_energy(lo, bright)) <= 1e-9 * mean_energy(lo, bright)


# ---- 7. api.hotspot_lightcurve end to end, and the program -------------------------------------------------------------------------------
@pytest.mark.parametrize("incl", [80.0, 30.0])
def test_api_hotspot_lightcurve_end_to_end(krlib, incl):
    h = spot(nt=60, **grid(10))
    res = api.hotspot_lightcurve(plane(incl), image_params(), h, limb="laor", return_records=True)
    rec = res["records"]
    assert len(rec) == 65 * 65
    mu, bad = angles(rec)
    words = np.concatenate([res["flux"], res["sx"], res["sy"], res["spectrogram"].ravel(), [res["on_disc"], res["used"], res["bad_angle"], 0.0]])
    against_the_rule("test_api_hotspot_lightcurve_end_to_end", f"incl{incl:.0f}", h, words, rec, LAOR, mu, bad, lambda lo: lo["used"] > 100 and lo["flux"].max() > 0)
    assert np.array_equal(res["time"], hr.times(h))
    lit = res["flux"] != 0
    assert lit.any() and np.isfinite(res["x"][lit]).all() and np.isnan(res["x"][~lit]).all()
    assert (np.abs(res["x"][lit]) <= R_DISC).all() and (np.abs(res["y"][lit]) <= R_DISC).all()


def test_program_equals_api(krlib, tmp_path):
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_hotspot_lightcurve")
    assert os.path.exists(exe), "kr_hotspot_lightcurve not built (__graft_entry__.build())"
    out = tmp_path / "hotspot.dat"
    r = subprocess.run([exe, f"--parfile={os.path.join(APPS, 'hotspot_lightcurve.par')}", f"--outfile={out}"], capture_output=True, text=True, timeout=300, cwd=APPS)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(out).read()
    h = capi.hot_spot(10.0, 2.0, cut=3.0, phi0=0.5, spin=SPIN, t0=10000.0, nt=24, g_index=3.0, line_energy=6.4, e_min=3.0, de=(9.0 - 3.0) / 12, ne=12,
                      r_isco=r_isco(), r_disc=R_DISC)
    h.dt = 1.0 * (2 * PI / abs(h.omega)) / 24
    res = api.hotspot_lightcurve(plane(80.0, 32), image_params(), h, limb=(1, 2.06))
    assert res["used"] > 30 and res["flux"].max() > 0 and res["spectrogram"].max() > 0
    assert text == api.hotspot_text(res)
    assert len(text.splitlines()) == 3 + 24 + 24 * 13
    shifted = subprocess.run([exe, f"--parfile={os.path.join(APPS, 'hotspot_lightcurve.par')}", f"--outfile={out}", "--spot_phi0=2.0", "--ne=0"], capture_output=True,
                             text=True, timeout=300, cwd=APPS)
    assert shifted.returncode == 0, shifted.stdout + shifted.stderr
    h.phi0, h.ne = 2.0, 0
    assert open(out).read() == api.hotspot_text(api.hotspot_lightcurve(plane(80.0, 32), image_params(), h, limb=(1, 2.06)))
