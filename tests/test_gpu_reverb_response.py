"""GPU: the reverberation response of the disc (kr_response_model; kr_post_response_dev_f64, kr_reduce_response_dev_f64, kr_reduce_response_f64,
api.disc_response, apps/kr_reverb_response) against the numpy rule of tests/response_rules.py, against the spectrum and the line pass, and against itself.

The bar: the tallies and the zero / non-zero pattern of resp are exact, and every non-zero cell lies within max(16 x noise, floor) of the float64 rule.
`noise` is the rule's own float64-vs-longdouble difference on the same records (response_rules.noise), `floor` the table floor that shape_floor derives
in tests/test_gpu_disc_spectrum.py: a cell often holds ONE record, whose node position carries the few ulp by which the device's log differs from
numpy's.  The tables have S > 0, so a cell is a sum of positive terms.  Precondition, asserted in every comparison: no used record has its radial-table
coordinate fi, its zone coordinate fz or its time coordinate ft within 1e-9 of an integer -- a last-bit difference must not move a record to another bin,
zone or row -- and no cell and no record is left out.  Every case goes through parity.record_margin; scripts/response_parity_worst.py picks
the worst case per test from the margins file of a run for profiles/reverb_response_parity.json.

Records and helpers: those of tests/test_gpu_disc_spectrum.py (ip15, ip16 and the 65 x 65 planes at 80 and 30 degrees, traced once per session).  The
fixtures' disc rays have t of about 9990 ... 10046 at dist = 1e4: with dt = 0.25 or 1 nearly every consecutive item starts a new row, with one wide row the
whole launch is one run."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import fits_lite
import parity
import response_rules as rr
import spectrum_rules as sr
import test_gpu_disc_spectrum as ds
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

PI = math.pi
SPIN, POST, R_DISC = ds.SPIN, ds.POST, ds.R_DISC
T0 = 9950.0                                # every disc ray of the fixtures and planes arrives later, also with the source delay below
EMIS40 = np.linspace(2.0, 0.1, 40)
TIME40 = 12.0 + 9.0 * np.sqrt(np.arange(40) / 40.0)          # a source -> disc delay that grows outwards, 12 ... 21


def response_model(dt=1.0, nt=200, t0=T0, tables=False, **kw):
    """A response over ds.table_model(**kw) (a cut-off power law in two zones, S > 0); tables: table_emis and table_time in 40 log bins over the disc."""
    spec = ds.table_model(table_emis=EMIS40 if tables else None, **kw)
    return capi.response_model(spec, t0, dt, nt, table_time=TIME40 if tables else None)


def fused(R, law, rays, calls=1):
    """kr_post_response_dev_f64 `calls` times into one zeroed buffer, each on a fresh device copy of `rays`: (words, records after)."""
    L = api.lib()
    law = capi.limb_law(law)
    nw = api.response_words(R)
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        after = rays
        for _ in range(calls):
            with DeviceScope(L) as one:
                d = one.upload(rays) if len(rays) else None
                capi.check(L, L.kr_post_response_dev_f64(-SPIN, *POST, 0, -PI, PI, C.byref(R), C.byref(law), d, len(rays), h, None), "kr_post_response")
                capi.check(L, L.kr_synchronize(None), "sync")
                after = one.fetch(d, len(rays), rays.dtype) if len(rays) else rays
        return dev.fetch(h, nw), after


def reduced(R, rays):
    """kr_reduce_response_dev_f64 on a device copy of records that carry their redshift: (words, records after)."""
    L = api.lib()
    nw = api.response_words(R)
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        d = dev.upload(rays) if len(rays) else None
        capi.check(L, L.kr_reduce_response_dev_f64(C.byref(R), d, len(rays), h, None), "kr_reduce_response")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(h, nw), (dev.fetch(d, len(rays), rays.dtype) if len(rays) else rays)


def away_from_integers(x):
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x)]
    return x.size == 0 or float(np.abs(x - np.round(x)).min()) >= 1e-9


def against_the_rule(test, case, R, words, rec, law=(0, 0.0), mu=None, bad=None):
    """The bar of the module docstring; returns the float64 rule's result."""
    noise, lo, hi = rr.noise(R, rec, law=law[0], coeff=law[1], mu=mu, bad=bad)
    assert away_from_integers(lo["fi"]) and away_from_integers(lo["fz"]) and away_from_integers(lo["ft"]), (test, case, "precondition")
    got = api.response_from_words(R, words)
    assert got["resp"].shape == (R.nt, R.spec.ne)
    assert (got["on_disc"], got["used"], got["bad_angle"], got["outside"]) == rr.tallies(lo), (test, case)
    assert np.array_equal(got["resp"] == 0, lo["resp"] == 0), (test, case)
    assert (lo["resp"] >= 0).all()
    floor = ds.shape_floor(R.spec, rec)
    d = rr.cell_diff(got["resp"], lo["resp"])
    diff = float(d.max()) if d.size else 0.0
    allowed = max(16 * noise, floor)
    cells = int((lo["resp"] != 0).sum())
    print(f"{test} {case}: on_disc {got['on_disc']} used {got['used']} bad_angle {got['bad_angle']} outside {got['outside']}; rows "
          f"{len(set(lo['row'][lo['row'] >= 0]))}, non-zero cells {cells}; noise {noise:.3e}, floor {floor:.3e}, device - rule {diff:.3e}")
    parity.record_margin(test, case, {"n_traced": int(len(rec)), "n_bad": 0, "frac_bad": 0.0, "worst_ok": diff}, allowed=allowed, noise=noise, floor=floor,
                               device_minus_rule=diff, device_minus_longdouble_rule=float(rr.cell_diff(got["resp"], hi["resp"]).max()) if d.size else 0.0,
                               used=got["used"], outside=got["outside"], cells=cells, nt=int(R.nt), ne=int(R.spec.ne))
    assert diff <= allowed, (test, case, diff, noise, floor)
    return lo


# ---- 1. device against the numpy rule: fused and reduce forms ----------------------------------------------------------------------
@pytest.mark.parametrize("tables", [False, True], ids=["powerlaw3", "emis+time"])
@pytest.mark.parametrize("name", ["ip15", "ip16", "plane80", "plane30"])
def test_device_against_the_rule(krlib, name, tables):
    rays, R = ds.records(name), response_model(tables=tables)
    post, _ = ds.post_line_records(rays)
    mu, bad = ds.angles(rays)
    law = (1, 2.06)
    words, after = fused(R, law, rays)
    assert after.tobytes() == post.tobytes()
    lo = against_the_rule("test_device_against_the_rule", f"{name}-{'tables' if tables else 'powerlaw3'}-fused-laor", R, words, post, law, mu, bad)
    assert lo["used"] > 30 and lo["outside"] == 0
    words, after = reduced(R, post)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_device_against_the_rule", f"{name}-{'tables' if tables else 'powerlaw3'}-reduce", R, words, post)
    host = api.reduce_response(R, post)                                                    # the host-record form: the same kernel
    assert (host["on_disc"], host["used"], host["bad_angle"], host["outside"]) == tuple(int(w) for w in words[-4:])
    assert np.array_equal(host["resp"] == 0, words[:-4].reshape(R.nt, -1) == 0) and sr.rel_diff(host["resp"].ravel(), words[:-4]) <= 1e-12
    assert np.array_equal(host["time"], (np.arange(R.nt) + 0.5) * R.dt) and np.allclose(host["energy"], sr.energies(R.spec), rtol=4e-16, atol=0)


def test_table_time_without_table_emis_and_a_non_finite_delay(krlib):
    """table_time alone takes ir for the delay and powerlaw3 for the emissivity; a record in a bin whose delay is NaN or inf is not used."""
    rays = ds.records("plane80")
    post, _ = ds.post_line_records(rays)
    time = TIME40.copy()
    time[[3, 17]] = np.nan, np.inf
    spec = ds.table_model(table_r_min=ds.r_isco(), table_dr=(R_DISC / ds.r_isco()) ** (1.0 / 40))
    R = capi.response_model(spec, T0, 1.0, 200, table_time=time)
    assert not R.spec.table_emis and R.spec.table_nr == 40
    words, _ = reduced(R, post)
    lo = against_the_rule("test_table_time_without_table_emis", "plane80", R, words, post)
    assert 30 < lo["used"] < lo["on_disc"] and lo["outside"] == 0


# ---- 2. against two independent existing passes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", [False, True], ids=["powerlaw3", "emis+time"])
@pytest.mark.parametrize("name", ["ip16", "plane80", "plane30"])
def test_rows_sum_to_the_spectrum_pass(krlib, name, tables):
    rays, R = ds.records(name), response_model(dt=0.5, nt=400, tables=tables)
    words, _ = fused(R, "laor", rays)
    got = api.response_from_words(R, words)
    spec_words, _ = ds.fused(R.spec, "laor", rays)
    want = api.spectrum_from_words(R.spec, spec_words)
    assert got["outside"] == 0 and (got["on_disc"], got["used"], got["bad_angle"]) == (want["on_disc"], want["used"], want["bad_angle"]) and got["used"] > 30
    worst = sr.rel_diff(got["resp"].sum(axis=0), want["flux"])
    print(f"{name}: rows summed against kr_post_spectrum_dev_f64: {worst:.2e}")
    assert worst <= parity.BIN_RTOL


@pytest.mark.parametrize("tables", [False, True], ids=["powerlaw3", "emis+time"])
@pytest.mark.parametrize("name", ["ip16", "plane80", "plane30"])
def test_flat_table_equals_the_line_pass_per_time_row(krlib, name, tables):
    """S = 1 and one energy: resp[:, 0] is the line pass's flux plane (g_index = 3) summed over its energies, row by row."""
    rays = ds.records(name)
    L = api.lib()
    dt, nt = 1.5, 40                                                                # 9950 ... 10010: the latest rays fall outside
    b = capi.line_bins(line_energy=1.0, e_min=1e-3, de=1.2, ne=80, log_e=True, t0=T0, dt=dt, nt=nt, r_isco=ds.r_isco(), r_disc=R_DISC, q1=3.0, rb1=4.0, q2=2.5, rb2=10.0,
                       q3=3.0, g_index=3.0)
    kw = {}
    if tables:
        b.with_table(ds.r_isco(), (R_DISC / ds.r_isco()) ** (1.0 / 40), EMIS40, TIME40)
        kw = dict(table_emis=EMIS40, table_r_min=ds.r_isco(), table_dr=(R_DISC / ds.r_isco()) ** (1.0 / 40))
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(api.line_words(b) * 8)
        capi.check(L, L.kr_post_line_dev_f64(-SPIN, *POST, 0, -PI, PI, C.byref(b), d, len(rays), h, None), "kr_post_line")
        post, line = dev.fetch(d, len(rays), rays.dtype), api.line_from_words(b, dev.fetch(h, api.line_words(b)))
    spec = capi.spectrum_model("table", 1.0, 0.5, 1, r_isco=ds.r_isco(), r_disc=R_DISC, q1=3.0, rb1=4.0, q2=2.5, rb2=10.0, q3=3.0, s=np.ones(64), s_e_min=1e-3, s_de=1.3, **kw)
    R = capi.response_model(spec, T0, dt, nt, table_time=TIME40 if tables else None)
    g = post["redshift"][sr.disc_filter(spec, post)]
    E = sr.energies(spec)[0]
    assert g.min() * E >= 1e-3 and g.max() * E <= sr.last_node(spec) and g.min() > 1e-3 and g.max() < 1e-3 * 1.2 ** 80      # every ray inside both energy ranges
    words, after = fused(R, "isotropic", rays)
    assert after.tobytes() == post.tobytes()
    got = api.response_from_words(R, words)
    assert got["on_disc"] == line["on_disc"] == got["used"] > 30 and got["outside"] > 0
    assert line["binned"] == got["used"] - got["outside"]
    want = line["flux"].sum(axis=1)
    assert np.array_equal(want == 0, got["resp"][:, 0] == 0) and np.array_equal(line["count"].sum(axis=1) > 0, got["resp"][:, 0] != 0)
    worst = sr.rel_diff(got["resp"][:, 0], want)
    print(f"{name}: flat table against the line pass's flux plane per time row: {worst:.2e}")
    assert worst <= parity.BIN_RTOL


# ---- 3. shapes where the kernel can go wrong --------------------------------------------------------------------------------------
def shape_response(ne, nt=3, dt=40.0, nz=1, s_ne=600, tables=False):
    """ds.shape_model's smooth table (log_e for odd ne), three wide rows by default."""
    s_de, S = ds.smooth_table(nz, s_ne)
    extra = dict(table_emis=EMIS40, table_r_min=ds.r_isco(), table_dr=(R_DISC / ds.r_isco()) ** (1.0 / 40)) if tables else {}
    spec = capi.spectrum_model("table", 0.05, (40.0 / 0.05) ** (1.0 / ne) if ne % 2 else 39.95 / ne, ne, log_e=ne % 2 == 1, r_isco=ds.r_isco(), r_disc=R_DISC, s=S, s_e_min=0.01,
                               s_de=s_de, **extra)
    return capi.response_model(spec, T0, dt, nt, table_time=TIME40 if tables else None)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3 * 256 + 1])
def test_every_record_count(krlib, n):
    src = ds.records("plane80")
    post_all, _ = ds.post_line_records(src)
    first = int(np.flatnonzero(sr.disc_filter(ds.thermal_model(), post_all))[0])                 # begin at a record on the disc
    rays, post = np.ascontiguousarray(src[first:first + n]), np.ascontiguousarray(post_all[first:first + n])
    assert len(rays) == n
    R = shape_response(65, nt=90, dt=1.0)
    if n == 0:
        L = api.lib()
        with DeviceScope(L) as dev:
            h = dev.upload(np.full(api.response_words(R), 7.0))
            law = capi.limb_law("laor")
            capi.check(L, L.kr_post_response_dev_f64(-SPIN, *POST, 0, -PI, PI, C.byref(R), C.byref(law), None, 0, h, None), "kr_post_response")
            capi.check(L, L.kr_reduce_response_dev_f64(C.byref(R), None, 0, h, None), "kr_reduce_response")
            assert (dev.fetch(h, api.response_words(R)) == 7.0).all()                        # n == 0 adds nothing
        host = api.reduce_response(R, post)
        assert not host["resp"].any() and (host["on_disc"], host["used"], host["bad_angle"], host["outside"]) == (0, 0, 0, 0)
        return
    mu, bad = ds.angles(rays)
    words, after = fused(R, "laor", rays)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_every_record_count", f"n{n}-fused", R, words, post, (1, 2.06), mu, bad)
    words, after = reduced(R, post)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_every_record_count", f"n{n}-reduce", R, words, post)


@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257, 1025, 4096])
def test_every_energy_count(krlib, ne):
    rays = ds.records("ip16")
    post, _ = ds.post_line_records(rays)
    R = shape_response(ne, nt=3, dt=40.0, tables=ne in (65, 1025))
    mu, bad = ds.angles(rays)
    words, after = fused(R, "laor", rays)
    assert after.tobytes() == post.tobytes()
    lo = against_the_rule("test_every_energy_count", f"ne{ne}", R, words, post, (1, 2.06), mu, bad)
    assert len(set(lo["row"])) >= 2 and lo["outside"] == 0


@pytest.mark.parametrize("nt,dt", [(1, 200.0), (2, 60.0), (257, 0.375)])
def test_every_row_count(krlib, nt, dt):
    rays = ds.records("ip15")
    post, _ = ds.post_line_records(rays)
    R = shape_response(130, nt=nt, dt=dt)
    mu, bad = ds.angles(rays)
    words, _ = fused(R, "laor", rays)
    lo = against_the_rule("test_every_row_count", f"nt{nt}", R, words, post, (1, 2.06), mu, bad)
    rows = set(lo["row"])
    assert lo["outside"] == 0 and (len(rows) == nt if nt <= 2 else max(rows) >= 250 and len(rows) > 20)      # nt = 257: rows up to the last few are lit


def test_tiles_without_rays_and_with_only_the_last_lane(krlib):
    """Three tiles of 256 records: in the first no ray passes the filter, in the second only the last lane's does, the third is as traced."""
    src = ds.records("plane80")
    post_all, _ = ds.post_line_records(src)
    on = sr.disc_filter(ds.thermal_model(), post_all)
    last = next(j for j in np.flatnonzero(on) if j >= 511 and j + 257 <= len(src) and on[j + 1:j + 257].sum() > 10)      # the record of lane 255 of the second tile
    rays = np.ascontiguousarray(src[last - 511:last + 257])
    dead = np.ones(768, dtype=bool)
    dead[511:] = False
    rays["steps"][dead] = -1 * np.abs(rays["steps"][dead])                                      # steps <= 0: filtered
    assert rays["steps"][511] > 0
    post, _ = ds.post_line_records(rays)
    f = sr.disc_filter(ds.thermal_model(), post)
    assert not f[:256].any() and list(np.flatnonzero(f[256:512])) == [255] and f[512:].sum() > 10
    R = shape_response(300, nt=200, dt=1.0)
    mu, bad = ds.angles(rays)
    words, after = fused(R, "laor", rays)
    assert after.tobytes() == post.tobytes()
    against_the_rule("test_tiles", "fused", R, words, post, (1, 2.06), mu, bad)
    words, _ = fused(R, "laor", np.ascontiguousarray(rays[:512]))
    assert int(words[-4]) == 1 and int(words[-3]) == 1 and int(words[-1]) == 0 and (words[:-4] != 0).sum() == 300          # one record: one row, every energy
    words, _ = fused(R, "laor", np.ascontiguousarray(rays[:256]))
    assert not words.any()


@pytest.mark.parametrize("nz", [1, 3])
@pytest.mark.parametrize("where", ["lds", "global"])
def test_table_on_both_sides_of_the_lds_budget(krlib, nz, where):
    budget = ds.lds_limit()
    s_ne = budget // nz if where == "lds" else budget // nz + 1
    assert (nz * s_ne <= budget) == (where == "lds") and nz * (s_ne + 1) > budget
    rays = ds.records("ip16")
    post, _ = ds.post_line_records(rays)
    R = shape_response(130, nt=25, dt=4.0, nz=nz, s_ne=s_ne)
    mu, bad = ds.angles(rays)
    words, _ = fused(R, "laor", rays)
    against_the_rule("test_table_on_both_sides_of_the_lds_budget", f"nz{nz}-{where}-s_ne{s_ne}", R, words, post, (1, 2.06), mu, bad)
    assert len(set(sr.zone_of(R.spec, post["r"][sr.disc_filter(R.spec, post)]))) == nz


# ---- 4. runs: how long the items of a workgroup stay in one row ---------------------------------------------------------------------------
def on_disc_records(name="plane80"):
    """The records of a plane that pass the filter, after the redshift pass, in their traced order."""
    post, _ = ds.post_line_records(ds.records(name))
    return np.ascontiguousarray(post[sr.disc_filter(ds.thermal_model(), post)])


def test_one_row_for_the_whole_launch(krlib):
    post = on_disc_records()
    R = response_model(dt=500.0, nt=1)
    words, _ = reduced(R, post)
    lo = against_the_rule("test_runs", "one-row", R, words, post)
    assert set(lo["row"]) == {0} and lo["used"] == len(post) > 500


def test_a_new_row_with_nearly_every_item(krlib):
    post = on_disc_records()
    R = response_model(dt=0.25, nt=800)
    words, _ = reduced(R, post)
    lo = against_the_rule("test_runs", "dt0.25", R, words, post)
    changes = int((np.diff(lo["row"]) != 0).sum())
    print(f"dt = 0.25: {changes} row changes among {len(post)} consecutive items, {len(set(lo['row']))} rows")
    assert lo["outside"] == 0 and changes > 0.8 * (len(post) - 1)


def test_rows_that_decrease(krlib):
    post = np.ascontiguousarray(on_disc_records()[::-1])
    R = response_model(dt=1.0, nt=200, tables=True)
    words, _ = reduced(R, post)
    lo = against_the_rule("test_runs", "reversed", R, words, post)
    forward = rr.response(R, np.ascontiguousarray(post[::-1]))
    assert rr.tallies(forward) == rr.tallies(lo) and np.array_equal(forward["row"][::-1], lo["row"])
    assert (np.diff(lo["row"]) < 0).sum() > 50 and (np.diff(lo["row"]) > 0).sum() > 50          # the rows go up and down, in the order opposite to the traced one


def test_two_rows_alternating_item_by_item(krlib):
    post = on_disc_records().copy()
    post["t"] = np.where(np.arange(len(post)) % 2 == 0, 10003.3, 10017.7)
    R = response_model(dt=1.0, nt=200)
    words, _ = reduced(R, post)
    lo = against_the_rule("test_runs", "alternating", R, words, post)
    assert list(lo["row"][:4]) == [53, 67, 53, 67] and set(lo["row"]) == {53, 67}
    assert (words[:-4].reshape(200, -1).any(axis=1)).sum() == 2


def test_an_outside_record_between_two_of_the_same_row(krlib):
    """Every third record leaves the window (one early, the next one late, a NaN now and then); the others share two rows in runs of two."""
    post = on_disc_records().copy()
    k = np.arange(len(post))
    t = np.where((k // 3) % 2 == 0, 10003.3, 10017.7)
    t = np.where(k % 3 == 1, np.where((k // 3) % 3 == 0, 9000.4, np.where((k // 3) % 3 == 1, 20000.6, np.nan)), t)
    post["t"] = t
    R = response_model(dt=1.0, nt=200)
    words, _ = reduced(R, post)
    lo = against_the_rule("test_runs", "outside-between", R, words, post)
    assert lo["outside"] == int((k % 3 == 1).sum()) and lo["used"] == len(post)
    inside = np.ascontiguousarray(post[k % 3 != 1])
    words_in, _ = reduced(R, inside)
    assert np.array_equal(words_in[-4:], [len(inside), len(inside), 0, 0])
    assert np.array_equal(words_in[:-4] == 0, words[:-4] == 0) and sr.rel_diff(words[:-4], words_in[:-4]) <= parity.BIN_RTOL      # the rows are intact


# ---- 5. additivity -------------------------------------------------------------------------------------------------------------
def test_two_shards_add_up_to_one_call(krlib):
    rays = ds.records("plane30")
    R = response_model(dt=1.0, nt=70, tables=True)                                           # 9950 ... 10020: some rays outside
    L = api.lib()
    law = capi.limb_law("laor")
    nw = api.response_words(R)
    whole, _ = fused(R, "laor", rays)
    assert whole[-1] > 0 and whole[-3] - whole[-1] > 30
    half = len(rays) // 2 + 7
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        for part in (rays[:half], rays[half:]):
            d = dev.upload(np.ascontiguousarray(part))
            capi.check(L, L.kr_post_response_dev_f64(-SPIN, *POST, 0, -PI, PI, C.byref(R), C.byref(law), d, len(part), h, None), "kr_post_response")
        capi.check(L, L.kr_synchronize(None), "sync")
        both = dev.fetch(h, nw)
    assert np.array_equal(both[-4:], whole[-4:]) and np.array_equal(both[:-4] == 0, whole[:-4] == 0)
    assert sr.rel_diff(both[:-4], whole[:-4]) <= parity.BIN_RTOL
    twice, _ = fused(R, "laor", rays, calls=2)
    assert np.array_equal(twice[-4:], 2 * whole[-4:]) and sr.rel_diff(twice[:-4], 2 * whole[:-4]) <= parity.BIN_RTOL


# ---- 6. api.disc_response end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("incl", [80.0, 30.0])
def test_api_disc_response_end_to_end(krlib, incl):
    R = response_model(dt=2.0, nt=60, tables=True)
    res = api.disc_response(ds.plane(incl), ds.image_params(), R, limb="laor", return_records=True)
    rec = res["records"]
    assert len(rec) == 65 * 65 and res["used"] > 500
    mu, bad = ds.angles(rec)
    words = np.concatenate([res["resp"].ravel(), [res["on_disc"], res["used"], res["bad_angle"], res["outside"]]])
    against_the_rule("test_api_disc_response_end_to_end", f"incl{incl:.0f}", R, words, rec, (1, 2.06), mu, bad)
    assert np.allclose(res["energy"], sr.energies(R.spec), rtol=4e-16, atol=0) and np.array_equal(res["time"], (np.arange(60) + 0.5) * 2.0)
    edges = R.spec.e_min * R.spec.de ** np.arange(R.spec.ne + 1)
    lag = api.lag_energy(res["resp"], R.dt, np.diff(edges), np.array([0.0005, 0.001, 0.002]), np.arange(0, 20), cont=res["energy"] ** -2.0, refl=0.5)
    lit = res["resp"].any(axis=0)
    assert lit.sum() > 50 and np.isfinite(lag["lag"][lit]).all() and np.abs(lag["lag"][lit]).max() > 0


# ---- 7. the program ------------------------------------------------------------------------------------------------------------
def program_rest_spectrum(energy, value, bins):
    """apps/rest_spectrum.h step by step in scalar libm arithmetic: (s_e_min, s_de, S).  api.resample_spectrum takes the same nodes through numpy's power
    and interp, which round differently in the last bit: invisible in the 8 digits of kr_disc_spectrum's text file, not in a FITS plane."""
    first, last = float(energy[0]), float(energy[-1])
    s_de = math.exp(math.log(last / first) / (bins - 1))
    S = []
    for k in range(bins):
        node = first * math.pow(s_de, k)
        if k == bins - 1 and node > last:
            node = last
        le = math.log(node)
        if le <= math.log(energy[0]):
            S.append(float(value[0]))
        elif le >= math.log(energy[-1]):
            S.append(float(value[-1]))
        else:
            j = 0
            while j + 2 < len(energy) and le >= math.log(energy[j + 1]):
                j += 1
            l0, l1 = math.log(energy[j]), math.log(energy[j + 1])
            S.append(float(value[j]) + (le - l0) / (l1 - l0) * (float(value[j + 1]) - float(value[j])))
    return first, s_de, np.array(S)


def test_program_equals_api(krlib, tmp_path):
    exe = os.path.join(ds.ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_reverb_response")
    assert os.path.exists(exe), "kr_reverb_response not built (__graft_entry__.build())"
    out = tmp_path / "response.fits"
    r = subprocess.run([exe, f"--parfile={os.path.join(ds.APPS, 'reverb_response.par')}", f"--outfile={out}"], capture_output=True, text=True, timeout=300, cwd=ds.APPS)
    assert r.returncode == 0, r.stdout + r.stderr
    hdus = fits_lite.read(str(out))
    assert [h["name"] for h in hdus] == ["PRIMARY", "ENERGY", "TIME"]
    e, c = np.loadtxt(os.path.join(ds.APPS, "powerlaw.spec"), unpack=True)
    s_e_min, s_de, S = program_rest_spectrum(e, c, 64)
    assert np.allclose(S, api.resample_spectrum(e, c, 64)[2], rtol=1e-14, atol=0)
    table = np.loadtxt(os.path.join(ds.APPS, "emissivity.dat"))
    radius, emis, delay = table[:, 0], table[:, 4], table[:, 6]
    dr = float(np.exp(np.log(radius[-1] / radius[0]) / (len(radius) - 1)))
    spec = capi.spectrum_model("table", 0.5, math.exp(math.log(200 / 0.5) / 24), 24, log_e=True, r_isco=ds.r_isco(), r_disc=R_DISC, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0,
                               s=np.array([S, S]), s_e_min=s_e_min, s_de=s_de, table_emis=emis, table_r_min=float(radius[0]), table_dr=dr)
    R = capi.response_model(spec, 10000.0, 2.5, 32, table_time=delay)
    res = api.disc_response(ds.plane(80.0, 15), ds.image_params(), R)                 # 16 x 16 = 256 records: one tile, so every cell is summed in one order
    assert res["used"] > 30 and res["resp"].any()
    assert hdus[0]["data"].shape == (32, 24) and hdus[0]["data"].tobytes() == res["resp"].tobytes()
    assert hdus[1]["data"].tobytes() == res["energy"].tobytes() and hdus[2]["data"].tobytes() == res["time"].tobytes()
    head = hdus[0]["header"]
    assert (int(head["ON_DISC"]), int(head["USED"]), int(head["BADANGLE"]), int(head["OUTSIDE"])) == (res["on_disc"], res["used"], res["bad_angle"], res["outside"])
    assert (int(head["NT"]), int(head["NEN"]), float(head["T0"]), float(head["DT"]), head["LOG_E"]) == (32, 24, 10000.0, 2.5, "T")
    assert abs(float(head["DE"]) / spec.de - 1) < 1e-14 and float(head["E_MIN"]) == 0.5
