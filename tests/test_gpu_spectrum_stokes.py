"""GPU: the Stokes spectra of the disc continuum (kr_post_spectrum_stokes_dev_f64, kr_reduce_spectrum_stokes_dev_f64, kr_reduce_spectrum_stokes_f64,
api.disc_spectrum(pol=...), apps/kr_disc_spectrum with pol_law) against the numpy rule of tests/spectrum_stokes_rules.py, the per-record polarisation
pass, the spectrum and Stokes-line passes, the line pass whose records it must leave, and itself.

The bar.  Tallies are exact.  I stays within max(16 x noise, floor) of the float64 rule, relative to I per energy; Q and U get the same bar, but
relative to P[i] = sum |cd| X_i, the polarised flux without cancellation, not to |Q|: Q crosses zero, and a quotient there means nothing.  `noise` is the
rule's own float64 - longdouble difference on the same records.  `floor` is what the number format alone allows (floors() below has the derivation).
Every comparison goes through parity.record_margin.

Records: the fixtures ip15 / ip16 (80 degrees), the 65 x 65 planes at 80 and 30 degrees that tests/test_gpu_disc_spectrum.py describes, traced here once per
session, and a copy of the 80-degree plane with three disc records spoilt into bad-pol records."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import parity
import polarisation_rules as pr
import spectrum_rules as sr
import spectrum_stokes_rules as ss
import test_gpu_disc_spectrum as td
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

PI, SPIN, POST, EPS = td.PI, td.SPIN, td.POST, td.EPS
LAOR, CHANDRA, CONSTANT, NEGATIVE = (1, 2.06), (1, 0.1171), (0, 0.3), (0, -0.3)
LIMBS = {"iso": (0, 0.0), "laor": LAOR, "bright": (2, 0.0)}
POLS = {"constant": CONSTANT, "negative": NEGATIVE, "chandrasekhar": CHANDRA}
INCL = {"ip15": 80.0, "ip16": 80.0, "plane80": 80.0, "plane30": 30.0, "spoilt80": 80.0}

_RAW, _POST, _POL = {}, {}, {}


def records(name):
    """The fixtures' final__rk4 (td.records); the 65 x 65 planes at 80 and 30 degrees, traced here once per session as td.records traces them (a trace of
    this module's own: tests elsewhere write into theirs); and "spoilt80": plane80 with three disc records made bad-pol -- Q x 1e4 twice (mu > 1:
    bad-angle), alpha = beta = NaN once (no observer)."""
    if name in ("ip15", "ip16"):
        return td.records(name)
    if name not in _RAW:
        if name == "spoilt80":
            idx = np.flatnonzero(sr.disc_filter(td.thermal_model(), post_records("plane80")))[[3, 50, 100]]
            rays = records("plane80").copy()
            rays["Q"][idx[:2]] *= 1e4
            rays["alpha"][idx[2]] = rays["beta"][idx[2]] = np.nan
        else:
            res = api.disc_spectrum(td.plane(INCL[name]), td.image_params(), td.thermal_model(ne=4), return_records=True)
            assert len(res["records"]) == 65 * 65 and res["on_disc"] > 500
            rays = res["records"]
        _RAW[name] = rays
    return _RAW[name]


def post_records(name):
    """rays[] after kr_post_line_dev_f64 (cached per name)."""
    if name not in _POST:
        _POST[name] = td.post_line_records(records(name))[0]
    return _POST[name]


def polar(name):
    if name not in _POL:
        _POL[name] = ss.polar(post_records(name), -SPIN, INCL[name])
    return _POL[name]


def fused(m, limb, pol, rays, incl, calls=1):
    """kr_post_spectrum_stokes_dev_f64 `calls` times into one zeroed buffer, each on a fresh device copy of `rays`: (words, records after)."""
    L = api.lib()
    law, plaw = capi.limb_law(limb), capi.pol_law(pol)
    nw = api.spectrum_stokes_words(m)
    with DeviceScope(L) as dev:
        out = dev.zeros(nw * 8)
        after = rays
        for _ in range(calls):
            with DeviceScope(L) as one:
                d = one.upload(rays) if len(rays) else None
                capi.check(L, L.kr_post_spectrum_stokes_dev_f64(-SPIN, *POST, 0, -PI, PI, incl, C.byref(m), C.byref(law), C.byref(plaw), d, len(rays), out, None),
                           "kr_post_spectrum_stokes")
                capi.check(L, L.kr_synchronize(None), "sync")
                after = one.fetch(d, len(rays), rays.dtype) if len(rays) else rays
        return dev.fetch(out, nw), after


def reduced(m, limb, pol, rays, incl):
    """kr_reduce_spectrum_stokes_dev_f64 on a device copy of records that carry their redshift: (words, records after)."""
    L = api.lib()
    law, plaw = capi.limb_law(limb), capi.pol_law(pol)
    nw = api.spectrum_stokes_words(m)
    with DeviceScope(L) as dev:
        out = dev.zeros(nw * 8)
        d = dev.upload(rays) if len(rays) else None
        capi.check(L, L.kr_reduce_spectrum_stokes_dev_f64(-SPIN, POST[0], POST[1], POST[2], incl, C.byref(m), C.byref(law), C.byref(plaw), d, len(rays), out, None),
                   "kr_reduce_spectrum_stokes")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(out, nw), (dev.fetch(d, len(rays), rays.dtype) if len(rays) else rays)


def floors(m, rec):
    """{plane: floor}: what the number format alone allows, whatever the records' own noise happens to be.
    I: td.shape_floor, derived there -- thermal 2 (4 (x_max + 1) + 8) ulp for the exponent's inputs (E_i through pow, g E_i, the reciprocal of f_col kT)
    amplified by d ln B / d ln x <= x + 1 and the 8 ulp of expm1, cube, g^-3, products and quotient; table 2 (4 s_ne slope + 8) ulp for the node
    position -- relative to every term c X > 0, hence to their sum I.
    Q, U: a term cq X = ((c delta) c2) X carries the same X and c and three more roundings (delta's quotient counts two: the device divides where numpy
    divides, but 1 + 3.582 mu and coeff (1 - mu) round before it; the two products cd, cq one each): 4 ulp more, doubled for the rule's own error, relative
    to |cd| X >= |cq X|, hence to their sum P."""
    base = td.shape_floor(m, rec)
    return {"flux": base, "q": base + 8 * EPS, "u": base + 8 * EPS}


def plane_guard(lo):
    return lo["used"] > 500 and lo["p"].max() > 0 and (np.abs(lo["q"]).max() > 0 or np.abs(lo["u"]).max() > 0)


def fixture_guard(lo):
    return lo["used"] > 30 and lo["p"].max() > 0 and (np.abs(lo["q"]).max() > 0 or np.abs(lo["u"]).max() > 0)


def some_guard(lo):
    return lo["used"] >= 1 and lo["p"].max() > 0


def against_the_rule(test, case, m, words, rec, pol, limb, pol_law, guard, rule=None):
    """The guard on the rule's output first (a vacuous case fails as vacuous), then tallies exact and I, Q, U within max(16 x noise, floor) of the float64
    rule (rule: (noise, lo, hi) taken before, for a second form on the same records); returns (noise, lo, hi)."""
    noise, lo, hi = rule if rule is not None else ss.noise(m, rec, pol, limb=limb, pol_law=pol_law)
    assert guard(lo), (test, case, "vacuous", lo["on_disc"], lo["used"], lo["bad_pol"], float(lo["p"].max()))
    got = ss.from_words(m, words)
    assert (got["on_disc"], got["used"], got["bad_pol"]) == (lo["on_disc"], lo["used"], lo["bad_pol"]), (test, case, got["on_disc"], got["used"], got["bad_pol"])
    assert words[-1] == 0.0 and np.isfinite(words).all(), (test, case)
    floor = floors(m, rec)
    for k in ss.PLANES:
        diff, allowed = ss.diff(got, lo, k), max(16 * noise[k], floor[k])
        print(f"{test} {case} {k}: used {got['used']} bad_pol {got['bad_pol']}; noise {noise[k]:.3e}, floor {floor[k]:.3e}, device - rule {diff:.3e}, "
              f"device - longdouble rule {ss.diff(got, hi, k):.3e}")
        parity.record_margin(test, f"{case}-{k}", {"n_traced": int(len(rec)), "n_bad": 0, "frac_bad": 0.0, "worst_ok": diff}, allowed=allowed, noise=noise[k], floor=floor[k],
                             device_minus_rule=diff, device_minus_longdouble_rule=ss.diff(got, hi, k), used=got["used"], bad_pol=got["bad_pol"], ne=int(m.ne))
        assert diff <= allowed, (test, case, k, diff, noise[k], floor[k])
    return noise, lo, hi


def both_forms(test, case, name, m, limb, pol_law, guard, rays=None, post=None, pol=None):
    """The fused form on the traced records (which must end as after kr_post_line_dev_f64) and the reduce form on those (which it must not write)."""
    rays = records(name) if rays is None else rays
    post = post_records(name) if post is None else post
    pol = polar(name) if pol is None else pol
    words, after = fused(m, limb, pol_law, rays, INCL[name])
    assert after.tobytes() == post.tobytes(), (test, case)
    rule = against_the_rule(test, f"{case}-fused", m, words, post, pol, limb, pol_law, guard)
    again, after = reduced(m, limb, pol_law, post, INCL[name])
    assert after.tobytes() == post.tobytes(), (test, case)
    against_the_rule(test, f"{case}-reduce", m, again, post, pol, limb, pol_law, guard, rule)
    return words, again, rule[1]


# ---- 1. device against the numpy rule: both forms x six kinds of model x three record sets ---------------------------------------------------------
def global_table():
    """nz = 3 zones of 1500 nodes: 4500 words, above the LDS budget."""
    m = td.table_model(nz=3, s_ne=1500)
    assert m.nz * m.s_ne > td.lds_limit()
    return m


MODELS = dict(td.MODELS)            # thermal (log), thermal-linear, table (nz = 2, 600 words: LDS), table-linear-emis (nz = 3, table_emis)
MODELS["table-global-nz3"] = global_table


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("name", ["ip15", "plane80", "plane30"])
def test_device_against_the_rule(krlib, name, model):
    m = MODELS[model]()
    traced = name != "ip15"
    pol_law = CHANDRA if model.startswith("thermal") else CONSTANT
    words, again, lo = both_forms("test_device_against_the_rule", f"{name}-{model}", name, m, LAOR, pol_law, plane_guard if traced else fixture_guard)
    if model.startswith("table") and model != "table":
        assert len(set(sr.zone_of(m, post_records(name)["r"][lo["used_index"]]))) == 3
    host = api.reduce_spectrum_stokes(m, post_records(name), -SPIN, INCL[name], pol_law, limb=LAOR)          # the host-record form: the same kernel
    assert (host["on_disc"], host["used"], host["bad_pol"]) == tuple(int(w) for w in again[-4:-1])
    dev = api.spectrum_stokes_from_words(m, again)
    for k in ss.PLANES:
        assert np.abs(host[k] - dev[k]).max() <= 1e-12 * np.abs(lo["p" if k != "flux" else "flux"]).max()


@pytest.mark.parametrize("limb", sorted(LIMBS))
@pytest.mark.parametrize("pol_law", sorted(POLS))
@pytest.mark.parametrize("name", ["ip16", "spoilt80"])
def test_pol_laws_and_limb_laws(krlib, name, pol_law, limb):
    """Bad-pol records add to nothing under EVERY limb law, law 0 included (where the spectrum pass uses a bad-angle ray)."""
    m = td.thermal_model(ne=40) if pol_law != "negative" else td.table_model(ne=40)
    _, _, lo = both_forms("test_pol_laws_and_limb_laws", f"{name}-{pol_law}-{limb}", name, m, LIMBS[limb], POLS[pol_law], plane_guard if name == "spoilt80" else fixture_guard)
    assert lo["bad_pol"] == (3 if name == "spoilt80" else 0)                              # the guard against a vacuous bad-pol case: the RULE counts 3
    if name == "spoilt80":
        clean = ss.spectrum_stokes(m, post_records("plane80"), polar("plane80"), limb=LIMBS[limb], pol_law=POLS[pol_law])
        assert clean["bad_pol"] == 0 and clean["used"] == lo["used"] + 3 and clean["on_disc"] == lo["on_disc"]


# ---- 2. shapes where the kernel can go wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["thermal", "table"])
@pytest.mark.parametrize("ne", [1, 255, 256, 257, 512, 513, 1025, 2049, 4096])
def test_every_energy_count(krlib, kind, ne):
    """Every slot boundary: one, two, four, eight and sixteen energies per lane, and waves that own no energy in the last slot."""
    m = td.shape_model(kind, ne)
    words, _, _ = both_forms("test_every_energy_count", f"{kind}-ne{ne}", "ip16", m, LAOR, CHANDRA, fixture_guard)
    assert len(words) == 3 * ne + 4


@pytest.mark.parametrize("kind", ["thermal", "table"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, 1000])
def test_every_record_count(krlib, kind, n):
    src, post_all, pol_all = records("plane80"), post_records("plane80"), polar("plane80")
    first = int(np.flatnonzero(sr.disc_filter(td.thermal_model(), post_all))[0])              # begin at a record on the disc
    rays, post = np.ascontiguousarray(src[first:first + n]), np.ascontiguousarray(post_all[first:first + n])
    pol = {k: (v[first:first + n] if isinstance(v, np.ndarray) and len(v) == len(src) else v) for k, v in pol_all.items()}
    assert len(rays) == n
    m = td.shape_model(kind, 65)
    if n == 0:
        L = api.lib()
        law, plaw = capi.limb_law("laor"), capi.pol_law(CHANDRA)
        with DeviceScope(L) as dev:
            h = dev.upload(np.full(api.spectrum_stokes_words(m), 7.0))
            capi.check(L, L.kr_post_spectrum_stokes_dev_f64(-SPIN, *POST, 0, -PI, PI, 80.0, C.byref(m), C.byref(law), C.byref(plaw), None, 0, h, None), "kr_post_spectrum_stokes")
            capi.check(L, L.kr_reduce_spectrum_stokes_dev_f64(-SPIN, *POST, 80.0, C.byref(m), C.byref(law), C.byref(plaw), None, 0, h, None), "kr_reduce_spectrum_stokes")
            assert (dev.fetch(h, api.spectrum_stokes_words(m)) == 7.0).all()                 # n == 0 adds nothing
        host = api.reduce_spectrum_stokes(m, post, -SPIN, 80.0, CHANDRA, limb=LAOR)
        assert not host["flux"].any() and not host["q"].any() and (host["on_disc"], host["used"], host["bad_pol"]) == (0, 0, 0)
        return
    both_forms("test_every_record_count", f"{kind}-n{n}", "plane80", m, LAOR, CHANDRA, some_guard, rays=rays, post=post, pol=pol)


@pytest.mark.parametrize("kind", ["thermal", "table"])
def test_tiles_without_rays_and_with_only_the_last_lane(krlib, kind):
    """Three tiles of 256 records: in the first no ray passes the filter, in the second only the last lane's does, the third is as traced; then the
    same with the live tile first, so that the tile without a live record sits in the middle of the launch."""
    src, post_all = records("plane80"), post_records("plane80")
    on = sr.disc_filter(td.thermal_model(), post_all)
    last = next(j for j in np.flatnonzero(on) if j >= 511 and j + 257 <= len(src) and on[j + 1:j + 257].sum() > 10)      # the record of lane 255 of the second tile
    rays = src[last - 511:last + 257].copy()                                                   # (a copy: the session's records stay as traced)
    dead = np.ones(768, dtype=bool)
    dead[511:] = False
    rays["steps"][dead] = -1 * np.abs(rays["steps"][dead])                                      # steps <= 0: filtered
    m = td.shape_model(kind, 300)
    for order, tiles in (("dead-last-live", (0, 1, 2)), ("live-dead-last", (2, 0, 1))):
        part = np.ascontiguousarray(np.concatenate([rays[256 * t:256 * (t + 1)] for t in tiles]))
        post = td.post_line_records(part)[0]
        f = sr.disc_filter(m, post).reshape(3, 256)
        assert not f[tiles.index(0)].any() and list(np.flatnonzero(f[tiles.index(1)])) == [255] and f[tiles.index(2)].sum() > 10
        both_forms("test_tiles", f"{kind}-{order}", "plane80", m, LAOR, CHANDRA, some_guard, rays=part, post=post, pol=ss.polar(post, -SPIN, 80.0))
    only, _ = fused(m, LAOR, CHANDRA, np.ascontiguousarray(rays[:512]), 80.0)
    assert int(only[-4]) == 1 and int(only[-3]) == 1 and only[:m.ne].any()
    none, _ = fused(m, LAOR, CHANDRA, np.ascontiguousarray(rays[:256]), 80.0)
    assert not none.any()


@pytest.mark.parametrize("nz", [1, 3])
@pytest.mark.parametrize("where", ["lds", "global"])
def test_table_on_both_sides_of_the_lds_budget(krlib, nz, where):
    budget = td.lds_limit()
    s_ne = budget // nz if where == "lds" else budget // nz + 1
    assert (nz * s_ne <= budget) == (where == "lds") and nz * (s_ne + 1) > budget
    s_de, S = td.smooth_table(nz, s_ne)
    m = capi.spectrum_model("table", 0.05, 1.05, 130, log_e=True, r_isco=td.r_isco(), r_disc=td.R_DISC, s=S, s_e_min=0.01, s_de=s_de)
    _, _, lo = both_forms("test_table_on_both_sides_of_the_lds_budget", f"nz{nz}-{where}-s_ne{s_ne}", "ip16", m, LAOR, CONSTANT, fixture_guard)
    assert len(set(sr.zone_of(m, post_records("ip16")["r"][lo["used_index"]]))) == nz


# ---- 3. against independent kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["thermal", "table"])
@pytest.mark.parametrize("name", ["ip15", "plane80", "plane30"])
def test_q_and_u_are_the_sums_of_the_per_record_pass(krlib, name, kind):
    """Q(E), U(E) formed in numpy from kr_polarisation_dev_f64's per-record c2, s2 (another kernel) with the rule's weights and X."""
    m, post = td.MODELS[kind](), post_records(name)
    per_record = api.polarisation(post, -SPIN, INCL[name])
    pol = dict(polar(name))
    live = post["steps"] > 0
    assert np.array_equal(per_record["c2"][live & ~pol["bad"]], pol["c2"][live & ~pol["bad"]])        # (the per-record pass is bit-exact against its rule)
    pol["c2"], pol["s2"] = per_record["c2"], per_record["s2"]
    want = ss.spectrum_stokes(m, post, pol, limb=LAOR, pol_law=CHANDRA)
    assert (plane_guard if name != "ip15" else fixture_guard)(want)
    words, _ = fused(m, LAOR, CHANDRA, records(name), INCL[name])
    got = ss.from_words(m, words)
    noise, _, _ = ss.noise(m, post, polar(name), limb=LAOR, pol_law=CHANDRA)
    floor = floors(m, post)
    for k in ("q", "u"):
        assert ss.diff(got, want, k) <= max(16 * noise[k], floor[k]), (name, kind, k)


@pytest.mark.parametrize("kind", ["thermal", "table"])
@pytest.mark.parametrize("limb", sorted(LIMBS))
@pytest.mark.parametrize("name", ["ip16", "plane80", "plane30"])
def test_the_i_block_is_the_spectrum_pass(krlib, name, limb, kind):
    """On records without bad-pol the I block equals kr_post_spectrum_dev_f64's flux within the bar, the tallies agree, and so do the records' bytes."""
    m, rays, post = td.MODELS[kind](), records(name), post_records(name)
    plain, after_plain = td.fused(m, LIMBS[limb], rays)
    words, after = fused(m, LIMBS[limb], CHANDRA, rays, INCL[name])
    assert after.tobytes() == after_plain.tobytes() == post.tobytes()
    noise, lo, _ = ss.noise(m, post, polar(name), limb=LIMBS[limb], pol_law=CHANDRA)
    assert lo["bad_pol"] == 0 and lo["used"] > 30 and plain[-2] == 0
    assert np.array_equal(words[-4:-2], plain[-4:-2])
    diff = sr.rel_diff(words[:m.ne], plain[:m.ne])
    print(f"{name} {kind} {limb}: I block against kr_post_spectrum_dev_f64: {diff:.2e}")
    assert diff <= max(16 * noise["flux"], floors(m, post)["flux"])


@pytest.mark.parametrize("name", ["ip16", "plane80", "plane30"])
def test_a_flat_table_is_the_stokes_line_summed_over_energy(krlib, name):
    rays, post = records(name), post_records(name)
    emis = dict(q1=3.0, rb1=4.0, q2=2.5, rb2=10.0, q3=3.0)
    m = capi.spectrum_model("table", 1.0, 0.5, 8, r_isco=td.r_isco(), r_disc=td.R_DISC, s=np.ones(64), s_e_min=1e-3, s_de=1.3, **emis)
    g = post["redshift"][sr.disc_filter(m, post)]
    E = sr.energies(m)
    assert (g.min() * E >= 1e-3).all() and (g.max() * E <= sr.last_node(m)).all()
    b = capi.line_bins(line_energy=1.0, e_min=1e-3, de=1.2, ne=80, log_e=True, r_isco=td.r_isco(), r_disc=td.R_DISC, g_index=3.0, **emis)
    L = api.lib()
    law, plaw = capi.limb_law(LAOR), capi.pol_law(CHANDRA)
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(api.stokes_line_words(b) * 8)
        capi.check(L, L.kr_post_line_stokes_dev_f64(-SPIN, *POST, 0, -PI, PI, INCL[name], C.byref(b), C.byref(law), C.byref(plaw), d, len(rays), h, None), "kr_post_line_stokes")
        line = pr.stokes_line_from_words(b, dev.fetch(h, api.stokes_line_words(b)))
    words, _ = fused(m, LAOR, CHANDRA, rays, INCL[name])
    got = ss.from_words(m, words)
    assert got["used"] == line["binned"] == line["on_disc"] > 30 and got["bad_pol"] == line["bad_pol"] == 0
    want = ss.spectrum_stokes(m, post, polar(name), limb=LAOR, pol_law=CHANDRA)
    for k, plane in (("flux", "I"), ("q", "Q"), ("u", "U")):
        scale = want["flux" if k == "flux" else "p"][0]
        worst = float(np.abs(got[k] - line[plane].sum()).max() / scale)
        print(f"{name}: flat table {k} against the Stokes line's {plane} plane: {worst:.2e}")
        assert worst <= parity.BIN_RTOL and np.abs(got[k] - got[k][0]).max() <= 1e-12 * scale


# ---- 4. additivity and the thermal tail -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["thermal", "table"])
def test_two_shards_and_two_calls_add_up(krlib, kind):
    rays, m = records("plane30"), td.MODELS[kind]()
    L = api.lib()
    law, plaw = capi.limb_law(LAOR), capi.pol_law(CHANDRA)
    nw, ne = api.spectrum_stokes_words(m), m.ne
    whole, _ = fused(m, LAOR, CHANDRA, rays, 30.0)
    half = len(rays) // 2 + 7
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        for part in (rays[:half], rays[half:]):
            d = dev.upload(np.ascontiguousarray(part))
            capi.check(L, L.kr_post_spectrum_stokes_dev_f64(-SPIN, *POST, 0, -PI, PI, 30.0, C.byref(m), C.byref(law), C.byref(plaw), d, len(part), h, None), "kr_post_spectrum_stokes")
        capi.check(L, L.kr_synchronize(None), "sync")
        both = dev.fetch(h, nw)
    twice, _ = fused(m, LAOR, CHANDRA, rays, 30.0, calls=2)
    P = ss.spectrum_stokes(m, post_records("plane30"), polar("plane30"), limb=LAOR, pol_law=CHANDRA)["p"]
    scale = np.concatenate([whole[:ne], P, P])
    assert whole[-3] > 500 and np.abs(whole[ne:3 * ne]).max() > 0
    assert np.array_equal(both[-4:], whole[-4:]) and np.array_equal(twice[-4:], 2 * whole[-4:])
    assert (np.abs(both[:-4] - whole[:-4]) <= parity.BIN_RTOL * scale).all()
    assert (np.abs(twice[:-4] - 2 * whole[:-4]) <= parity.BIN_RTOL * scale).all()


def test_thermal_tail_leaves_q_and_u_finite(krlib):
    """Out to E = 20000 kT_max the expm1 overflows to inf: X = E'^3 / inf = 0 and I, Q, U stay finite, zero or tiny, never NaN."""
    rays, post = records("plane30"), post_records("plane30")
    r_min, dr, kt = td.kt_table()
    kt_max = float(np.nanmax(kt))
    m = capi.spectrum_model("thermal", 0.0, 20000 * kt_max / 256, 256, r_isco=td.r_isco(), r_disc=td.R_DISC, f_col=1.0, table_r_min=r_min, table_dr=dr, table_kt=kt)
    g_min = post["redshift"][sr.disc_filter(m, post)].min()
    assert g_min * sr.energies(m)[-1] / kt_max > 710                                       # past the overflow of expm1 for every ray
    want = ss.spectrum_stokes(m, post, polar("plane30"), limb=LAOR, pol_law=CHANDRA)
    assert plane_guard(want) and want["flux"][-1] == 0 and want["q"][-1] == 0
    for words, _ in (fused(m, LAOR, CHANDRA, rays, 30.0), reduced(m, LAOR, CHANDRA, post, 30.0)):
        got = ss.from_words(m, words)
        assert np.isfinite(words).all() and (got["flux"] >= 0).all() and got["used"] == want["used"]
        assert got["flux"][-1] == 0 and got["q"][-1] == 0 and got["u"][-1] == 0
        shallow = want["flux"] > 1e-200 * want["flux"].max()
        assert shallow.sum() > 3
        for k in ss.PLANES:
            scale = want["flux" if k == "flux" else "p"][shallow]
            assert (np.abs(got[k][shallow] - want[k][shallow]) <= 1e-11 * scale).all(), k  # (x up to ~480: 480 x a few ulp)
            assert (np.abs(got[k][~shallow]) <= 1e-190 * want["flux"].max()).all(), k


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["thermal", "table"])
@pytest.mark.parametrize("incl", [80.0, 30.0])
def test_api_disc_spectrum_with_pol_equals_fused_on_records(krlib, incl, kind):
    m = td.MODELS[kind]()
    res = api.disc_spectrum(td.plane(incl), td.image_params(), m, limb="laor", pol=CHANDRA, return_records=True)
    rec = res["records"]
    assert len(rec) == 65 * 65 and res["used"] > 500 and "bad_angle" not in res
    words, after = fused(m, LAOR, CHANDRA, rec, incl)                                         # (the pass computes g and the wrapped phi again from what it left alone)
    assert after.tobytes() == rec.tobytes()
    got = ss.from_words(m, words)
    assert (res["on_disc"], res["used"], res["bad_pol"]) == (got["on_disc"], got["used"], got["bad_pol"])
    P = ss.spectrum_stokes(m, rec, ss.polar(rec, -SPIN, incl), limb=LAOR, pol_law=CHANDRA)["p"]
    for k in ss.PLANES:                                                                      # (the same kernel on the same records: only the order of the atomic adds differs)
        assert (np.abs(res[k] - got[k]) <= 1e-13 * (got["flux"] if k == "flux" else P)).all(), k
    with np.errstate(all="ignore"):
        assert np.array_equal(res["pol_degree"], np.hypot(res["q"], res["u"]) / res["flux"]) and np.array_equal(res["pol_angle"], 0.5 * np.arctan2(res["u"], res["q"]))
    assert np.array_equal(res["energy"], sr.energies(m))


def test_the_degree_falls_with_energy_on_the_plane_at_80_degrees(krlib):
    """The physics of tests/test_spectrum_stokes_rules.py on the traced plane: thermal, 24 log energies 0.05 ... 20 keV, Laor, Chandrasekhar.  Asserted on
    the rule's output first, so a vacuous case fails as vacuous."""
    m = td.thermal_model(ne=24)
    want = ss.spectrum_stokes(m, post_records("plane80"), polar("plane80"), limb=LAOR, pol_law=CHANDRA)
    assert plane_guard(want)
    for label, res in (("rule", want), ("device", ss.from_words(m, fused(m, LAOR, CHANDRA, records("plane80"), 80.0)[0]))):
        degree, ang = ss.degree_angle(res)
        print(f"plane80 {label}: degree {100 * degree[0]:.2f} % -> {100 * degree[-1]:.2f} % ({degree[0] / degree[-1]:.1f} x), angle {math.degrees(ang[0]):.1f} -> "
              f"{math.degrees(ang[-1]):.1f} degrees")
        assert degree[0] >= 3 * degree[-1] and abs(math.degrees(ang[0])) < 5, label


def test_program_with_pol_keys_equals_api(krlib, tmp_path):
    exe = os.path.join(td.ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_disc_spectrum")
    assert os.path.exists(exe), "kr_disc_spectrum not built (__graft_entry__.build())"
    out = tmp_path / "spectrum.dat"
    r = subprocess.run([exe, f"--parfile={os.path.join(td.APPS, 'disc_spectrum_stokes.par')}", f"--outfile={out}"], capture_output=True, text=True, timeout=300, cwd=td.APPS)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(out).read()
    nr = 200
    dr = (td.R_DISC / td.r_isco()) ** (1.0 / nr)
    kt = api.thermal_kt_table(SPIN, td.r_isco(), dr, nr, 10.0, 1e18, f_col=1.7)
    m = capi.spectrum_model("thermal", 0.05, math.exp(math.log(20 / 0.05) / 24), 24, log_e=True, r_isco=td.r_isco(), r_disc=td.R_DISC, f_col=1.7, table_r_min=td.r_isco(),
                            table_dr=dr, table_kt=kt)
    res = api.disc_spectrum(td.plane(80.0, 32), td.image_params(), m, limb=(1, 2.06), pol=CHANDRA)
    assert res["used"] > 100 and res["flux"].max() > 0 and np.abs(res["q"]).max() > 0
    assert text == api.spectrum_text(res)
    assert text.splitlines()[2].split()[:2] == ["#", "BAD_POL"] and len(text.splitlines()[3].split()) == 4
    plain = tmp_path / "plain.dat"                                                           # without the keys: the file the spectrum pass always wrote
    r = subprocess.run([exe, f"--parfile={os.path.join(td.APPS, 'disc_spectrum_thermal.par')}", f"--outfile={plain}"], capture_output=True, text=True, timeout=300, cwd=td.APPS)
    assert r.returncode == 0 and open(plain).read().splitlines()[2].split()[:2] == ["#", "BAD_ANGLE"]
