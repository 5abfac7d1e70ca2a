"""GPU: the (r, phi) illumination map of the disc (kr_post_illum_dev_f64 / kr_reduce_illum_dev_f64 / kr_reduce_illum_f64, csrc/kr_illum.hip) against
the numpy restatement of tests/illum_rules.py applied to the records fetched from the device.

Source records, traced once per session: ONE off-axis kr_pointsource at pos = (0, 8, 1.0, 0.6), spin 0.9, V = 0.04 on a 99 x 125 grid (dcosalpha =
0.02, dbeta = 0.05: 12 503 slots), RK4 with the golden fixtures' trace parameters; and the on-axis fixture ps_h10.  Plus the chosen records of
tests/reducer_cases.py, which sit where traced rays almost never do (NaN and infinite phi and t, g = 0, every radial edge, 20 000 copies of one record).

  counts     every cell's count and both tallies equal the rule EXACTLY, no cell and no record left out.  The device's log is not correctly rounded,
             so each comparison first asserts that no binned record of the rule lies within 1e-9 of a cell edge (illum_rules.edge_margin); the
             azimuthal quotient is IEEE arithmetic on both sides.  phi_shift = 0.0137 keeps the sources' own symmetry planes off the edges.
  sums       within parity.BIN_RTOL of the per-cell sum of absolute terms (reducer_rules.check_reduction), non-finite cells alike
  shapes     nr x nphi = 12 x 16 (192 cells: the planes in LDS) and 64 x 512 (32 768 cells: global atomics, grouped by wave), 7 x 1 (nphi = 1: the
             emissivity histogram itself), and 32 x 32 / 33 x 32 either side of the 1024-cell crossover
  fused      rays[] after kr_post_illum_dev_f64 is byte for byte what kr_post_emissivity_dev_f64 leaves, and its map is the reduce form's on those
  adds       two calls into one buffer sum
  radial     summed over ip the map is the device's own emissivity histogram: counts exactly
  api        api.illumination_map for a PointSourceSpec, end to end, and api.illumination_table of its map
"""
import ctypes as C
import math

import numpy as np
import pytest

import golden_cases as gc
import illum_rules as il
import oracle_lib as ol
import parity
import reducer_cases as rc
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu
RTOL = parity.BIN_RTOL
EDGE = 1e-9
PHI_SHIFT = 0.0137
OFF_SPIN, OFF_V = 0.9, 0.04
R_DISC = 200.0
SHAPES = [(12, 16), (64, 512), (7, 1), (32, 32), (33, 32)]


def offaxis_source():
    return ol.pointsource_spec([0.0, 8.0, 1.0, 0.6], OFF_V, OFF_SPIN, 0.02, 0.05, cosalpha0=-0.995, cosalphamax=0.995, beta0=-np.pi, betamax=np.pi)


def offaxis_params():
    return gc._params(capi.RK4, spin=OFF_SPIN)


SOURCES = {"offaxis": (OFF_SPIN, OFF_V), "ps_h10": (gc.SPIN, 0.0)}


@pytest.fixture
def dev(krlib):
    with DeviceScope(krlib) as scope:
        yield scope


_TRACED = {}


def traced(name):
    """The records of one source after its constructor with the emitted energy and kr_trace_dev_f64 (RK4), fetched once and never modified."""
    if name not in _TRACED:
        L = api.lib()
        with DeviceScope(L) as scope:
            if name == "offaxis":
                spec = offaxis_source()
                n = api.pointsource_count(spec)[0]
                d = scope.alloc(n * capi.RAY_F64.itemsize)
                capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(spec), 0, 1, spec.V, 0, 0, d, n, None), "init_emit")
                p = offaxis_params()
            else:
                init = np.ascontiguousarray(np.load(gc.golden_path(name))["init"])          # the constructor's records after redshift_start(V = 0)
                n, d = len(init), scope.upload(init)
                p = gc.cases()[name]["runs"]["rk4"]
            capi.check(L, L.kr_trace_dev_f64(C.byref(p), d, n, None, None), "trace")
            rays = scope.fetch(d, n, capi.RAY_F64)
        assert name != "offaxis" or (12000 < (rays["steps"] != -1).sum() < 13500 and (rays["steps"] > 0).sum() > 10000)
        rays.setflags(write=False)
        _TRACED[name] = rays
    return _TRACED[name]


def finished(name):
    """The traced records after range_phi and redshift(V = -1) on the device: what the reduce forms read."""
    key = name + "/finished"
    if key not in _TRACED:
        rays = traced(name).copy()
        api.range_phi(rays)
        api.redshift(SOURCES[name][0], -1.0, 0, 0, rays)
        rays.setflags(write=False)
        _TRACED[key] = rays
    return _TRACED[key]


def bins_for(name, nr, nphi, phi_shift=PHI_SHIFT):
    spin = SOURCES[name][0] if name in SOURCES else 0.998
    b = capi.EmisBins()
    b.r_isco = api.lib().kr_kerr_isco(spin, 1)
    b.r_min, b.dr = b.r_isco, float(np.exp(np.log(R_DISC / b.r_isco) / nr))
    b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = 2.0, spin, 12503.0, nr, 1
    return capi.illum_bins(b, nphi, phi_shift)


def rule(m, rays, populated=True):
    """The rule's map of `rays`, with the precondition of every comparison asserted: no binned record within EDGE of a cell edge."""
    want = il.reduce_illum(m, rays)
    margin = il.edge_margin(want, m.rad.logbin)
    assert margin > EDGE, ("a record of the rule lies on a cell edge: choose other bins", margin)
    if populated:
        assert want["binned"] > 100 and want["disc_count"] >= want["binned"]
    return want


def map_on_device(dev, m, rays, d_out=None, fused=None):
    """(the map's words, the records afterwards, the buffer) of one pass over a device copy of `rays`; fused: (spin, V) of kr_post_illum_dev_f64"""
    L, nw, n = dev.lib, api.illum_words(m), len(rays)
    d_rays = dev.upload(np.ascontiguousarray(rays)) if n > 0 else C.c_void_p()
    d_out = d_out if d_out is not None else dev.zeros(nw * 8)
    if fused is not None:
        capi.check(L, L.kr_post_illum_dev_f64(fused[0], fused[1], 0, 0, 0, -math.pi, math.pi, C.byref(m), d_rays, n, d_out, None), "kr_post_illum")
    else:
        capi.check(L, L.kr_reduce_illum_dev_f64(C.byref(m), d_rays, n, d_out, None), "kr_reduce_illum")
    return dev.fetch(d_out, nw), dev.fetch(d_rays, n, capi.RAY_F64), d_out


def emissivity_on_device(dev, b, rays, fused=None):
    L, nw, n = dev.lib, api.emissivity_words(b), len(rays)
    d_rays, d_hist = dev.upload(np.ascontiguousarray(rays)), dev.zeros(nw * 8)
    if fused is not None:
        capi.check(L, L.kr_post_emissivity_dev_f64(fused[0], fused[1], 0, 0, 0, -math.pi, math.pi, C.byref(b), d_rays, n, d_hist, None), "kr_post_emissivity")
    else:
        capi.check(L, L.kr_reduce_emissivity_dev_f64(C.byref(b), d_rays, n, d_hist, None), "kr_reduce_emissivity")
    return api.emissivity_from_words(b, dev.fetch(d_hist, nw)), dev.fetch(d_rays, n, capi.RAY_F64)


@pytest.mark.parametrize("name", sorted(SOURCES))
@pytest.mark.parametrize("nr,nphi", SHAPES)
def test_map_of_traced_sources_equals_the_rule(dev, name, nr, nphi):
    rays = finished(name)
    m = bins_for(name, nr, nphi)
    want = rule(m, rays)
    got = api.illum_from_words(m, map_on_device(dev, m, rays)[0])
    worst = il.check_illum(got, want, RTOL, (name, nr, nphi, "reduce"))
    host = api.reduce_illum(m, np.ascontiguousarray(rays))
    worst = max(worst, il.check_illum(host, want, RTOL, (name, nr, nphi, "host form")))
    if name == "offaxis" and nphi > 1:
        # off the axis the map is NOT axisymmetric: the side under the source holds several times the rays of the far side
        ring = want["count"].sum(axis=0)
        assert ring.max() > 3 * max(ring.min(), 1)
    parity.record_margin("test_map_of_traced_sources_equals_the_rule", f"{name}-{nr}x{nphi}",
                         {"n_traced": int(want["binned"]), "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(worst)}, allowed=RTOL)


@pytest.mark.parametrize("name", sorted(SOURCES))
@pytest.mark.parametrize("nr,nphi", [(12, 16), (64, 512), (7, 1)])
def test_fused_pass_equals_the_emissivity_pass_and_the_reduce_form(dev, name, nr, nphi):
    rays = traced(name)
    spin = SOURCES[name][0]
    m = bins_for(name, nr, nphi)
    fused_words, fused_rays, _ = map_on_device(dev, m, rays, fused=(spin, -1.0))
    emis_hist, emis_rays = emissivity_on_device(dev, m.rad, rays, fused=(spin, -1.0))
    assert fused_rays.tobytes() == emis_rays.tobytes()                               # byte for byte what kr_post_emissivity_dev_f64 leaves
    assert fused_rays.tobytes() == finished(name).tobytes()                          # ... which is range_phi + redshift
    assert not np.array_equal(fused_rays["redshift"], rays["redshift"])              # the fused pass did compute g
    want = rule(m, fused_rays)
    got = api.illum_from_words(m, fused_words)
    il.check_illum(got, want, RTOL, (name, nr, nphi, "fused"))
    sep_words = map_on_device(dev, m, fused_rays)[0]
    ncell = nr * nphi
    np.testing.assert_array_equal(fused_words[:ncell], sep_words[:ncell])
    np.testing.assert_array_equal(fused_words[-2:], sep_words[-2:])
    assert np.array_equal(fused_words != 0, sep_words != 0) and np.allclose(fused_words, sep_words, rtol=RTOL, atol=0)
    # summed over ip: the device's own emissivity histogram of the same records (every record of these sources has a finite phi)
    assert got["binned"] == emis_hist["count"].sum() and got["disc_count"] == emis_hist["disc_count"]
    radial = il.summed_over_phi(got)
    np.testing.assert_array_equal(radial["count"], emis_hist["count"])
    for k in il.SUMS:
        assert np.allclose(radial[k], emis_hist[k], rtol=RTOL, atol=0), k          # (nphi == 1: the map IS the histogram)


@pytest.mark.parametrize("nr,nphi", [(12, 16), (64, 512)])
def test_two_calls_into_one_buffer_sum(dev, nr, nphi):
    a, b = finished("offaxis"), finished("offaxis")[::-1][:5000]
    m = bins_for("offaxis", nr, nphi)
    wa, wb = map_on_device(dev, m, a)[0], map_on_device(dev, m, b)[0]
    _, _, d_out = map_on_device(dev, m, a)
    both = map_on_device(dev, m, b, d_out=d_out)[0]
    ncell = nr * nphi
    np.testing.assert_array_equal(both[:ncell], (wa + wb)[:ncell])
    np.testing.assert_array_equal(both[-2:], (wa + wb)[-2:])
    assert np.array_equal(both != 0, (wa + wb) != 0) and np.allclose(both, wa + wb, rtol=RTOL, atol=0)
    assert wb[-1] > 100


@pytest.mark.parametrize("nr,nphi,logbin", [(12, 16, 1), (64, 512, 1), (7, 1, 1), (1025, 3, 0), (4, 8, 0)])
def test_chosen_records_land_where_the_rule_puts_them(dev, nr, nphi, logbin):
    """tests/reducer_cases.py: NaN and infinite phi (in no cell with nphi > 1, in theirs with nphi == 1), NaN and infinite t and g (their cell's sums
    are NaN or infinite, alike), every edge of the linear radial rule, steps <= 0, and 20 000 records in one cell; the large set wraps the grid-stride
    loop with a ragged tail."""
    m = capi.illum_bins(rc.emis_bins(nr, logbin), nphi, PHI_SHIFT)
    for rec in (rc.small(), rc.large()):
        rays = rec.rays
        want = rule(m, rays)
        assert want["count"].max() >= rc.N_CONTENTION or nr == 4
        words, after, _ = map_on_device(dev, m, rays)
        assert after.tobytes() == rays.tobytes()                                     # the reducing form never writes a record
        il.check_illum(api.illum_from_words(m, words), want, RTOL, (nr, nphi, logbin, len(rays)))
    # the fused form on records whose phi lies many turns out: range_phi brings |phi| <= 1000 home first, and the rule reads the stored value
    rays = rc.small().rays
    fused_words, fused_rays, _ = map_on_device(dev, m, rays, fused=(0.998, -1.0))
    il.check_illum(api.illum_from_words(m, fused_words), rule(m, fused_rays, populated=False), RTOL, (nr, nphi, logbin, "fused"))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_every_record_count(dev, n):
    full = finished("offaxis")
    start = int(np.flatnonzero(il.per_ray(bins_for("offaxis", 12, 16), full)["binned"])[3])      # a binned ray leads the slice
    rays = full[start:start + n]
    for nr, nphi in ((12, 16), (64, 512)):
        m = bins_for("offaxis", nr, nphi)
        want = rule(m, rays, populated=False)
        assert n == 0 or want["binned"] >= 1
        words, after, _ = map_on_device(dev, m, rays)
        il.check_illum(api.illum_from_words(m, words), want, RTOL, (n, nr, nphi))
        assert len(after) == n and after.tobytes() == rays.tobytes()


def test_phase_shift_rolls_the_map(dev):
    """phi_shift + 2 pi k / nphi is the same map k columns on: counts exactly, sums at the bar (under the precondition, on both shifts)."""
    rays = finished("offaxis")
    for nr, nphi, k in ((12, 16, 5), (64, 512, 131)):
        base, turned = bins_for("offaxis", nr, nphi), bins_for("offaxis", nr, nphi, PHI_SHIFT + 2 * math.pi * k / nphi)
        rule(base, rays), rule(turned, rays)
        a = api.illum_from_words(base, map_on_device(dev, base, rays)[0])
        b = api.illum_from_words(turned, map_on_device(dev, turned, rays)[0])
        np.testing.assert_array_equal(b["count"], np.roll(a["count"], k, axis=1))
        assert (a["disc_count"], a["binned"]) == (b["disc_count"], b["binned"])
        for key in il.SUMS:
            assert np.allclose(b[key], np.roll(a[key], k, axis=1), rtol=RTOL, atol=0), key


def test_api_illumination_map_end_to_end(krlib):
    src, p = offaxis_source(), offaxis_params()
    m = bins_for("offaxis", 12, 16)
    res = api.illumination_map(src, p, m, return_records=True)
    assert res["records"].tobytes() == finished("offaxis").tobytes()
    want = rule(m, res["records"])
    il.check_illum(res, want, RTOL, "api")
    assert res["stats"]["rays_traced"] > 10000 and res["count"].shape == (12, 16) and res["phi_shift"] == PHI_SHIFT
    # the table of the map: the annuli of the flat disc, the whole ring (dphi = 2 pi)
    edges = m.rad.r_min * m.rad.dr ** np.arange(13)
    areas = api.surface_area(edges, m.rad.r_isco, 0.0, 0.0, OFF_SPIN, dphi=2 * math.pi)
    tab = api.illumination_table(res, areas)
    e, t = il.table_from_map(res, areas)
    np.testing.assert_array_equal(tab["emis"], e)
    np.testing.assert_array_equal(tab["time"], t)
    lit = res["count"] > 0
    assert lit.sum() > 100 and np.isnan(tab["time"][~lit]).all() and np.isfinite(tab["time"][lit]).all() and (tab["emis"][lit] > 0).all()
    # the side under the source (phi_s = 0.6) is lit earlier than the far side of the same ring
    ring = 6
    near, far = np.argmin(np.abs(res["phi"] - 0.6)), np.argmin(np.abs(res["phi"] - (0.6 - math.pi)))
    assert tab["time"][ring, near] < tab["time"][ring, far]


# ---- the map as an (r, phi) table of the line and the response (kr_illum_table; the ILLUM flavour of kr_line.hip and kr_response.hip) -----------------
# Disc records, helpers and bars: those of tests/test_gpu_disc_spectrum.py, tests/test_gpu_reverb_response.py and tests/test_gpu_line_profile.py
# (ip15, ip16 and the 65 x 65 planes at 80 and 30 degrees, traced once per session).
#   rule       the reduce forms (device and host records) against illum_rules.line_from_rays / response: tallies, counts and the zero / non-zero pattern
#              exact; the line's flux within 1e-9 (the bar of test_gpu_line_profile.py against numpy), the response within max(16 x noise, floor)
#              (the bar of test_gpu_reverb_response.py).  The fused forms leave rays[] as kr_post_line_dev_f64 does and, under the isotropic law, give the
#              reduce forms' tallies and sums.
#   tables     12 x 16 and 40 x 64; emis smooth and positive, time growing outwards and varying with ip; the larger one with a block of NaN delays and
#              one zero-emis cell (its records count and add nothing: the cell pattern stays exact)
#   limit      a table whose columns are all equal is the flat twin with the radial table, for three phi_shift
#   phase      phi_shift + 2 pi k / nphi on a table is the table rolled by k columns
#   precondition, asserted in every comparison with the rule: no used record has fi, q_ph, fe / fz or ft within 1e-9 of an integer; no record and
#              no cell is left out of a comparison.
import line_rules as lr                      # noqa: E402
import response_rules as rsp                 # noqa: E402
import spectrum_rules as sr                  # noqa: E402
import test_gpu_disc_spectrum as ds          # noqa: E402
import test_gpu_reverb_response as rv        # noqa: E402

DISC = ["ip15", "ip16", "plane80", "plane30"]
T0 = rv.T0


def make_table(nr, nphi, holes=False, phi_shift=PHI_SHIFT, axisymmetric=False):
    """An il.Table over the disc of the records: emis smooth and positive, the delay growing outwards and (unless axisymmetric) varying with ip."""
    ir, ip = np.arange(nr)[:, None], np.arange(nphi)[None, :]
    swing = 0.0 if axisymmetric else 1.0
    emis = (2.0 - 1.9 * ir / nr) * (1.0 + 0.3 * swing * np.cos(2 * math.pi * (ip + 0.5) / nphi)) + 0.0 * ip
    time = 12.0 + 9.0 * np.sqrt(ir / nr) + 3.0 * swing * np.sin(2 * math.pi * (ip + 0.5) / nphi) + 0.0 * ip
    if holes:
        time[nr // 4:nr // 4 + 4, nphi // 2:nphi // 2 + 12] = np.nan
        time[nr // 2, 1] = np.inf
        emis[nr // 3, nphi // 4] = 0.0
    return il.Table(emis, ds.r_isco(), (ds.R_DISC / ds.r_isco()) ** (1.0 / nr), 1, time, phi_shift)


TABLES = {"12x16": lambda **kw: make_table(12, 16, **kw), "40x64-holes": lambda **kw: make_table(40, 64, holes=True, **kw)}


def line_bins_for(time_axis=True):
    return capi.line_bins(line_energy=6.4, e_min=0.5, de=0.0837, ne=110, t0=T0, dt=2.137 if time_axis else 0.0, nt=60 if time_axis else 1, r_isco=ds.r_isco(),
                          r_disc=ds.R_DISC, g_index=3.0)


def response_for(nt=200, dt=1.0137, **kw):
    return capi.response_model(ds.table_model(**kw), T0, dt, nt)


def run_words(nw, call, rays):
    """(words, records after) of one device pass call(L, d_rays, n, d_out) over a device copy of `rays`"""
    L = api.lib()
    with DeviceScope(L) as scope:
        h = scope.zeros(nw * 8)
        d = scope.upload(np.ascontiguousarray(rays))
        capi.check(L, call(L, d, len(rays), h), "illum pass")
        capi.check(L, L.kr_synchronize(None), "sync")
        return scope.fetch(h, nw), scope.fetch(d, len(rays), capi.RAY_F64)


def line_illum(b, T, rays, fused=False):
    t, law = T.struct(), capi.limb_law("isotropic")
    if fused:
        words, after = run_words(api.line_words(b) + 1, lambda L, d, n, h: L.kr_post_line_illum_dev_f64(-ds.SPIN, *ds.POST, 0, -math.pi, math.pi, C.byref(b), C.byref(law),
                                                                                                          C.byref(t), d, n, h, None), rays)
        return api.line_from_words(b, words[:-1]), after, int(round(words[-1]))
    words, after = run_words(api.line_words(b), lambda L, d, n, h: L.kr_reduce_line_illum_dev_f64(C.byref(b), C.byref(t), d, n, h, None), rays)
    return api.line_from_words(b, words), after, 0


def response_illum(R, T, rays, fused=False):
    t, law = T.struct(), capi.limb_law("isotropic")
    if fused:
        call = lambda L, d, n, h: L.kr_post_response_illum_dev_f64(-ds.SPIN, *ds.POST, 0, -math.pi, math.pi, C.byref(R), C.byref(law), C.byref(t), d, n, h, None)      # noqa: E731
    else:
        call = lambda L, d, n, h: L.kr_reduce_response_illum_dev_f64(C.byref(R), C.byref(t), d, n, h, None)      # noqa: E731
    return run_words(api.response_words(R), call, rays)


def line_against_the_rule(test, case, b, T, got, post):
    want = il.line_from_rays(b, T, post)
    for k in ("fi", "q_ph", "fe") + (("ft",) if lr.has_time_axis(b) else ()):          # (without a time axis there is no ft)
        assert rv.away_from_integers(want[k]), (test, case, "precondition", k)
    assert (got["on_disc"], got["binned"]) == (want["on_disc"], want["binned"]), (test, case)
    problems, m = lr.compare_line(got, want, rtol=1e-9, slack=0, max_excluded=0)
    assert problems == [] and np.array_equal(got["flux"] == 0, want["flux"] == 0), (test, case, problems)
    parity.record_margin(test, case, {"n_traced": int(want["on_disc"]), "n_bad": 0, "frac_bad": 0.0, "worst_ok": m["worst_flux_rel"]}, allowed=1e-9)
    return want


def response_against_the_rule(test, case, R, T, words, post):
    noise, lo, hi = il.response_noise(R, T, post)
    for k in ("fi", "q_ph", "fz", "ft"):
        assert rv.away_from_integers(lo[k]), (test, case, "precondition", k)
    got = api.response_from_words(R, words)
    assert (got["on_disc"], got["used"], got["bad_angle"], got["outside"]) == rsp.tallies(lo), (test, case)
    assert np.array_equal(got["resp"] == 0, lo["resp"] == 0), (test, case)
    floor = ds.shape_floor(R.spec, post)
    d = rsp.cell_diff(got["resp"], lo["resp"])
    diff, allowed = (float(d.max()) if d.size else 0.0), max(16 * noise, floor)
    print(f"{test} {case}: used {got['used']} outside {got['outside']}; noise {noise:.3e}, floor {floor:.3e}, device - rule {diff:.3e}")
    parity.record_margin(test, case, {"n_traced": int(len(post)), "n_bad": 0, "frac_bad": 0.0, "worst_ok": diff}, allowed=allowed, noise=noise, floor=floor)
    assert diff <= allowed, (test, case, diff, noise, floor)
    return lo


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", DISC)
def test_line_with_a_table_against_the_rule(krlib, name, table):
    rays, T = ds.records(name), TABLES[table]()
    post, _ = ds.post_line_records(rays)
    for time_axis in (True, False):
        b = line_bins_for(time_axis)
        got, after, _ = line_illum(b, T, post)
        assert after.tobytes() == post.tobytes()                                       # the reducing form never writes a record
        want = line_against_the_rule("test_line_with_a_table_against_the_rule", f"{name}-{table}-t{int(time_axis)}", b, T, got, post)
        assert want["binned"] > 30 and (table == "12x16" or name != "plane30" or want["used"] < want["on_disc"])      # (the holes do leave records out)
        t = T.struct()
        host = np.zeros(api.line_words(b))
        capi.check(krlib, krlib.kr_reduce_line_illum_f64(C.byref(b), C.byref(t), post.ctypes.data_as(C.c_void_p), len(post), host.ctypes.data_as(C.c_void_p)), "host form")
        line_against_the_rule("test_line_with_a_table_against_the_rule", f"{name}-{table}-t{int(time_axis)}-host", b, T, api.line_from_words(b, host), post)
        fused, fused_after, bad_angle = line_illum(b, T, rays, fused=True)
        assert fused_after.tobytes() == post.tobytes()                                 # rays[] as kr_post_line_dev_f64 leaves it
        np.testing.assert_array_equal(fused["count"], got["count"])
        assert (fused["on_disc"], fused["binned"]) == (got["on_disc"], got["binned"]) and bad_angle >= 0
        assert np.allclose(fused["flux"], got["flux"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", DISC)
def test_response_with_a_table_against_the_rule(krlib, name, table):
    rays, T, R = ds.records(name), TABLES[table](), response_for()
    post, _ = ds.post_line_records(rays)
    words, after = response_illum(R, T, post)
    assert after.tobytes() == post.tobytes()
    lo = response_against_the_rule("test_response_with_a_table_against_the_rule", f"{name}-{table}", R, T, words, post)
    assert lo["used"] > 30 and lo["outside"] < lo["used"] // 2 and (table == "12x16" or name != "plane30" or lo["used"] < lo["on_disc"])
    t = T.struct()
    host = np.zeros(api.response_words(R))
    capi.check(krlib, krlib.kr_reduce_response_illum_f64(C.byref(R), C.byref(t), post.ctypes.data_as(C.c_void_p), len(post), host.ctypes.data_as(C.c_void_p)), "host form")
    response_against_the_rule("test_response_with_a_table_against_the_rule", f"{name}-{table}-host", R, T, host, post)
    fused, fused_after = response_illum(R, T, rays, fused=True)
    assert fused_after.tobytes() == post.tobytes()
    assert fused[-4] == words[-4] and fused[-3] == words[-3] and fused[-1] == words[-1]      # on_disc, used, outside (bad_angle: the fused form alone sees angles)
    assert np.array_equal(fused[:-4] == 0, words[:-4] == 0) and sr.rel_diff(fused[:-4], words[:-4]) <= 1e-12


INSTANCES = [("2 slots", dict(ne=300)), ("4 slots", dict(ne=600)), ("8 slots", dict(ne=1100)), ("two launches", dict(ne=2100)),
             ("S in global memory", dict(ne=96, big_s=True)), ("S in global memory, 4 slots", dict(ne=600, big_s=True))]


@pytest.mark.parametrize("label,shape", INSTANCES, ids=[i[0] for i in INSTANCES])
def test_every_instance_of_the_table_response(krlib, label, shape):
    """The table flavour compiles 16 response instances: 1, 2, 4 or 8 energies per lane, S in LDS or (beyond the LDS budget) in global memory, fused or
    reducing.  The other tests stay at ne <= 256 and a small S: this one launches the rest, ne > 2048 (two launches over the same records) included."""
    rays, T = ds.records("ip16"), TABLES["40x64-holes"]()
    post, _ = ds.post_line_records(rays)
    kw = dict(ne=shape["ne"])
    if shape.get("big_s"):
        nz, s_ne = 4, ds.lds_limit() // 4 + 40
        kw.update(nz=nz, s_ne=s_ne, S=ds.cutoff_power_law(nz, s_ne)[1])
        assert nz * s_ne > ds.lds_limit()
    R = response_for(nt=64, dt=3.0137, **kw)
    words, after = response_illum(R, T, post)
    assert after.tobytes() == post.tobytes()
    lo = response_against_the_rule("test_every_instance_of_the_table_response", label, R, T, words, post)
    assert lo["used"] > 30 and lo["outside"] < lo["used"] // 2
    fused, fused_after = response_illum(R, T, rays, fused=True)
    assert fused_after.tobytes() == post.tobytes()
    assert fused[-4] == words[-4] and fused[-3] == words[-3] and fused[-1] == words[-1]
    assert np.array_equal(fused[:-4] == 0, words[:-4] == 0) and sr.rel_diff(fused[:-4], words[:-4]) <= 1e-12


@pytest.mark.parametrize("phi_shift", [0.0, PHI_SHIFT, -2.5])
@pytest.mark.parametrize("name", ["ip16", "plane80"])
def test_axisymmetric_table_is_the_flat_twin(krlib, name, phi_shift):
    """Equal columns: the (r, phi) table is the radial table, whatever the shift -- against kr_reduce_line_dev_f64 and kr_reduce_response_dev_f64."""
    rays = ds.records(name)
    post, _ = ds.post_line_records(rays)
    T = make_table(40, 64, phi_shift=phi_shift, axisymmetric=True)
    assert (T.emis == T.emis[:, :1]).all() and (T.time == T.time[:, :1]).all()
    b = line_bins_for()
    flat = line_bins_for().with_table(T.r_min, T.dr, T.emis[:, 0], T.time[:, 0], logbin=True)
    want, _ = run_words(api.line_words(flat), lambda L, d, n, h: L.kr_reduce_line_dev_f64(C.byref(flat), d, n, h, None), post)
    want = api.line_from_words(flat, want)
    got, _, _ = line_illum(b, T, post)
    line_against_the_rule("test_axisymmetric_table_is_the_flat_twin", f"{name}-{phi_shift}", b, T, got, post)
    np.testing.assert_array_equal(got["count"], want["count"])
    assert (got["on_disc"], got["binned"]) == (want["on_disc"], want["binned"]) and want["binned"] > 30
    assert np.array_equal(got["flux"] == 0, want["flux"] == 0) and np.allclose(got["flux"], want["flux"], rtol=1e-9, atol=0)
    R = response_for()
    Rflat = capi.response_model(ds.table_model(table_emis=T.emis[:, 0]), T0, R.dt, R.nt, table_time=T.time[:, 0])
    assert abs(Rflat.spec.table_dr / T.dr - 1) < 1e-15 and Rflat.spec.table_r_min == T.r_min
    T.dr = Rflat.spec.table_dr
    want_words, _ = rv.reduced(Rflat, post)
    words, _ = response_illum(R, T, post)
    lo = response_against_the_rule("test_axisymmetric_table_is_the_flat_twin", f"{name}-{phi_shift}", R, T, words, post)
    np.testing.assert_array_equal(words[-4:], want_words[-4:])
    allowed = max(16 * il.response_noise(R, T, post)[0], ds.shape_floor(R.spec, post))
    assert np.array_equal(words[:-4] == 0, want_words[:-4] == 0) and float(rsp.cell_diff(words[:-4], want_words[:-4]).max()) <= allowed and lo["used"] > 30


@pytest.mark.parametrize("nr,nphi,k", [(12, 16, 5), (40, 64, 23)])
def test_phase_is_a_roll_of_the_table(krlib, nr, nphi, k):
    """phi_shift + 2 pi k / nphi moves every record k cells on, so the table read with that shift is the table with its columns rolled back by k."""
    post, _ = ds.post_line_records(ds.records("plane80"))
    base = make_table(nr, nphi, holes=nr == 40)
    turned = il.Table(base.emis, base.r_min, base.dr, 1, base.time, PHI_SHIFT + 2 * math.pi * k / nphi)
    rolled = il.Table(np.roll(base.emis, -k, axis=1), base.r_min, base.dr, 1, np.roll(base.time, -k, axis=1), PHI_SHIFT)
    b, R = line_bins_for(), response_for()
    a_line, _, _ = line_illum(b, turned, post)
    b_line, _, _ = line_illum(b, rolled, post)
    line_against_the_rule("test_phase_is_a_roll_of_the_table", f"{nr}x{nphi}-turned", b, turned, a_line, post)
    line_against_the_rule("test_phase_is_a_roll_of_the_table", f"{nr}x{nphi}-rolled", b, rolled, b_line, post)
    np.testing.assert_array_equal(a_line["count"], b_line["count"])
    assert (a_line["on_disc"], a_line["binned"]) == (b_line["on_disc"], b_line["binned"]) and a_line["binned"] > 30
    assert np.allclose(a_line["flux"], b_line["flux"], rtol=1e-9, atol=0)
    assert not np.array_equal(a_line["count"], line_illum(b, base, post)[0]["count"])      # ... and the phase does change the line
    a_words, _ = response_illum(R, turned, post)
    b_words, _ = response_illum(R, rolled, post)
    response_against_the_rule("test_phase_is_a_roll_of_the_table", f"{nr}x{nphi}-turned", R, turned, a_words, post)
    response_against_the_rule("test_phase_is_a_roll_of_the_table", f"{nr}x{nphi}-rolled", R, rolled, b_words, post)
    np.testing.assert_array_equal(a_words[-4:], b_words[-4:])
    allowed = max(16 * il.response_noise(R, turned, post)[0], ds.shape_floor(R.spec, post))
    assert np.array_equal(a_words[:-4] == 0, b_words[:-4] == 0) and float(rsp.cell_diff(a_words[:-4], b_words[:-4]).max()) <= allowed


def test_api_line_profile_and_disc_response_with_a_table(krlib):
    """api.line_profile(..., illum=) and api.disc_response(..., illum=) on the 65 x 65 plane: the fused entry points, end to end, from a map's table."""
    T = make_table(12, 16)
    tab = {"emis": T.emis, "time": T.time, "r_min": T.r_min, "dr": T.dr, "logbin": 1, "phi_shift": T.phi_shift, "nr": 12, "nphi": 16}
    b, R = line_bins_for(), response_for()
    # the records of THIS plane's own trace, as the fused pass leaves them (the trace is deterministic; the session's cached planes are shared with
    # other modules and are not relied on to be a fresh trace)
    res = api.disc_response(ds.plane(80.0), ds.image_params(), R, illum=capi.illum_table(tab, phi_shift=T.phi_shift), return_records=True)
    post = res["records"]
    assert len(post) == 65 * 65 and post.tobytes() == ds.post_line_records(post)[0].tobytes()      # rays[] as kr_post_line_dev_f64 leaves it
    words, _ = response_illum(R, T, post)
    assert (res["on_disc"], res["used"], res["outside"]) == (int(words[-4]), int(words[-3]), int(words[-1])) and res["used"] > 500
    assert np.array_equal(res["resp"].ravel() == 0, words[:-4] == 0) and sr.rel_diff(res["resp"].ravel(), words[:-4]) <= 1e-12
    response_against_the_rule("test_api_line_profile_and_disc_response_with_a_table", "plane80-12x16", R, T, words, post)
    res = api.line_profile(ds.plane(80.0), ds.image_params(), b, illum=tab)
    want, _, _ = line_illum(b, T, post)
    line_against_the_rule("test_api_line_profile_and_disc_response_with_a_table", "plane80-12x16", b, T, want, post)
    np.testing.assert_array_equal(res["count"], want["count"])
    assert (res["on_disc"], res["binned"]) == (want["on_disc"], want["binned"]) and want["binned"] > 500
    assert np.allclose(res["flux"], want["flux"], rtol=1e-12, atol=0) and res["bad_angle"] >= 0
    for kw in (dict(surface=(1.3, 0.0, 0.05, 0.0)), dict(V=capi.V_PLUNGE)):
        with pytest.raises(capi.KrError, match="illum cannot be combined"):
            api.disc_response(ds.plane(80.0), ds.image_params(), R, illum=tab, **kw)
        with pytest.raises(capi.KrError, match="illum cannot be combined"):
            api.line_profile(ds.plane(80.0), ds.image_params(), b, illum=tab, **kw)


# ---- the program: kr_offaxis_reverb against the API, byte for byte ------------------------------------------------------------------------------------
def test_program_equals_api_and_phase_is_phi_shift(krlib, tmp_path):
    """tests/golden/apps/offaxis_reverb.par: 182 source rays (one workgroup of the map kernel), no map cell with more than two of them (asserted: a sum
    of two terms does not depend on their order) and 256 image-plane records (one tile of the response kernel), so every sum is taken in one order and
    the file's HDUs equal the API's arrays byte for byte; then the same with phase = 0.7, which is table.phi_shift = -0.7 and nothing else."""
    import os
    import subprocess

    import fits_lite
    exe = os.path.join(ds.ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_offaxis_reverb")
    assert os.path.exists(exe), "kr_offaxis_reverb not built (__graft_entry__.build())"
    src = ol.pointsource_spec([0.0, 8.0, 1.0, 0.6], 0.04, ds.SPIN, 0.2, 0.4, cosalpha0=-0.995, cosalphamax=0.995, beta0=-np.pi, betamax=np.pi)
    p_src = capi.copy_params(gc._params(capi.RK4, spin=ds.SPIN), flags=capi.FLAG_HYBRID)
    b = capi.EmisBins()
    b.r_min = b.r_isco = ds.r_isco()
    b.dr, b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = math.exp(math.log(ds.R_DISC / ds.r_isco()) / 16), 2.0, ds.SPIN, float(api.pointsource_count(src)[0]), 16, 1
    m = capi.illum_bins(b, 32, 0.0)
    illum = api.illumination_map(src, p_src, m)
    assert api.pointsource_count(src)[0] == 182 and illum["binned"] > 50 and illum["count"].max() <= 2
    rule(m, api.illumination_map(src, p_src, m, return_records=True)["records"], populated=False)       # (no source ray on a cell edge)
    e, c = np.loadtxt(os.path.join(ds.APPS, "powerlaw.spec"), unpack=True)
    s_e_min, s_de, S = rv.program_rest_spectrum(e, c, 64)
    spec = capi.spectrum_model("table", 0.5, math.exp(math.log(200 / 0.5) / 24), 24, log_e=True, r_isco=ds.r_isco(), r_disc=ds.R_DISC, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0,
                               q3=3.0, s=np.array([S, S]), s_e_min=s_e_min, s_de=s_de)
    R = capi.response_model(spec, 10000.0, 2.5, 32)
    results = {}
    for phase in (0.0, 0.7):
        out = tmp_path / f"offaxis_{phase}.fits"
        r = subprocess.run([exe, f"--parfile={os.path.join(ds.APPS, 'offaxis_reverb.par')}", f"--outfile={out}", f"--phase={phase}"], capture_output=True, text=True,
                           timeout=300, cwd=ds.APPS)
        assert r.returncode == 0, r.stdout + r.stderr
        hdus = fits_lite.read(str(out))
        assert [h["name"] for h in hdus] == ["RESPONSE", "ILLUM_EMIS", "ILLUM_TIME", "ILLUM_COUNT", "ILLUM_AREA"]
        data = {h["name"]: h["data"] for h in hdus}
        areas = data["ILLUM_AREA"].ravel()
        edges = b.r_min * b.dr ** np.arange(17)
        assert np.allclose(areas, api.surface_area(edges, b.r_isco, 0.0, 0.0, ds.SPIN, dphi=2 * math.pi), rtol=1e-12, atol=0)
        tab = api.illumination_table(illum, areas)
        assert data["ILLUM_COUNT"].shape == (16, 32) and data["ILLUM_COUNT"].tobytes() == illum["count"].astype(np.float64).tobytes()
        assert data["ILLUM_EMIS"].tobytes() == tab["emis"].tobytes()
        assert np.array_equal(np.isnan(data["ILLUM_TIME"]), np.isnan(tab["time"])) and np.isnan(tab["time"]).sum() == (illum["count"] == 0).sum() > 0
        lit = illum["count"] > 0
        assert data["ILLUM_TIME"][lit].tobytes() == tab["time"][lit].tobytes()
        res = api.disc_response(ds.plane(80.0, 15), ds.image_params(), R, limb=(1, 2.06), illum=capi.illum_table(tab, phi_shift=tab["phi_shift"] - phase))
        assert data["RESPONSE"].shape == (32, 24) and data["RESPONSE"].tobytes() == res["resp"].tobytes()
        head = hdus[0]["header"]
        assert (int(head["ON_DISC"]), int(head["USED"]), int(head["BADANGLE"]), int(head["OUTSIDE"])) == (res["on_disc"], res["used"], res["bad_angle"], res["outside"])
        assert (int(head["SRC_RAYS"]), int(head["SRC_DISC"]), int(head["SRC_BIN"])) == (182, illum["disc_count"], illum["binned"])
        assert float(head["PHASE"]) == phase and float(head["PHISHIFT"]) == -phase and (int(head["NR"]), int(head["NPHI"])) == (16, 32)
        assert 0 < res["used"] < res["on_disc"] and res["resp"].any()
        results[phase] = (res, data)
    # the phase turns the table against the disc and nothing else: the same map, another response
    assert results[0.0][1]["ILLUM_EMIS"].tobytes() == results[0.7][1]["ILLUM_EMIS"].tobytes()
    assert results[0.0][1]["RESPONSE"].tobytes() != results[0.7][1]["RESPONSE"].tobytes()
