"""GPU: where a source's rays end, by emission angle (kr_post_angdist_dev_f64 / kr_reduce_angdist_dev_f64, csrc/kr_angdist.hip) against the numpy
restatement of tests/source_vel_rules.py applied to the records fetched from the device.  Four emitters (a lamp-post at rest, the same flowing out, an
orbiting and outflowing blob, a plunging one), about 35 x 36 rays each at a = 0.998, traced with Euler and RK4 and default flags.

  counts     every tally, the two unweighted totals and -- with unit weights -- all twelve histograms equal the rule EXACTLY: the device's acos / sin /
             cos are correctly rounded, the rule's too (mpmath), so every ray lands in the rule's bin
  sums       weighted histograms and class sums within parity.BIN_RTOL of the per-bin sum of absolute terms, the summation-order bar of
             tests/test_gpu_reducers.py (the rule sums exactly; the device adds in whatever order the atomics arrive)
  adds       two calls into one buffer equal the sum of two buffers
  fused      kr_post_angdist_dev_f64 leaves phi and redshift as kr_range_phi_dev_f64 + kr_redshift_dev_f64 do and counts as kr_reduce_angdist_dev_f64
             counts those records, bit for bit
  Nangle     62 and 63 (histograms in LDS) and 4096 (global atomics)
  edge       cos(alpha) == 0, NaN and out-of-range angles: the tallies say so and no bin moves
  labels     both labellings of (alpha, beta): PointSourceVel's (labels = 1, what these records carry) and PointSource's (labels = 0)
  classes    for the Keplerian disc source at r = 3 the three class counts equal those of the landing map's classification (api.reduce_return_map,
             the pass api.return_radiation runs) of the same records
"""
import ctypes as C
import math

import numpy as np
import pytest

import parity
import source_vel_rules as sv
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu
RTOL = parity.BIN_RTOL
R_DISC, R_ESC = 500.0, 1000.0
INTEGRATORS = {"euler": capi.EULER, "rk4": capi.RK4}


def trace_params(integrator):
    p = capi.default_params(sv.SPIN)
    p.integrator, p.r_max, p.theta_max, p.stop_kind = integrator, 1.1 * R_ESC, math.pi / 2, capi.STOP_THETA      # disc_source_return_angdist.cpp:126
    return p


def spec_for(dangle=0.1, unit_weights=False, source_r=0.0, source_phi=0.0, **kw):
    kw.setdefault("labels", 1)                                                 # the records come from the PointSourceVel source
    if unit_weights:
        kw.update(plane_iso=0, limb=0, weight_norm=0)
    return api.angdist_spec(api.lib().kr_kerr_isco(sv.SPIN, 1), R_DISC, R_ESC, dangle, source_r, source_phi, **kw)


@pytest.fixture
def dev(krlib):
    with DeviceScope(krlib) as scope:
        yield scope


_TRACED = {}


def traced(name, integrator):
    """The records of one emitter after kr_pointsource_vel_init_emit_dev_f64 + kr_trace_dev_f64, fetched once per module and never modified."""
    key = (name, integrator)
    if key not in _TRACED:
        L = api.lib()
        spec = sv.spec_of(name)
        n = api.pointsource_vel_count(spec)[0]
        with DeviceScope(L) as scope:
            d = scope.alloc(n * capi.RAY_F64.itemsize)
            capi.check(L, L.kr_pointsource_vel_init_emit_dev_f64(C.byref(spec), d, n, None), "init_emit")
            capi.check(L, L.kr_trace_dev_f64(C.byref(trace_params(INTEGRATORS[integrator])), d, n, None, None), "trace")
            rays = scope.fetch(d, n, capi.RAY_F64)
        assert (rays["steps"] > 0).sum() == 1190
        rays.setflags(write=False)
        _TRACED[key] = rays
    return _TRACED[key]


def reduce_on_device(dev, sp, rays, d_out=None, fused=False):
    """(words, records afterwards) of one pass over a device copy of `rays`; d_out: a buffer to add into"""
    L, nw, n = dev.lib, api.angdist_words(sp), len(rays)
    d_rays = dev.upload(np.ascontiguousarray(rays))
    d_out = d_out if d_out is not None else dev.zeros(nw * 8)
    if fused:
        capi.check(L, L.kr_post_angdist_dev_f64(sv.SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(sp), d_rays, n, d_out, None), "kr_post_angdist")
    else:
        capi.check(L, L.kr_reduce_angdist_dev_f64(C.byref(sp), d_rays, n, d_out, None), "kr_reduce_angdist")
    return dev.fetch(d_out, nw), dev.fetch(d_rays, n, capi.RAY_F64), d_out


def exact_counts(got, want, label):
    """with unit weights every histogram is a count: equal to the rule's bin populations, word for word"""
    for k in sv.HIST_KEYS:
        np.testing.assert_array_equal(got[k], want[k + "_n"], err_msg=f"{label} {k}")
    for c in ("escape", "return", "lost"):
        assert got[c + "_sum"] == want[c + "_count"], (label, c)
    assert got["ray_count"] == want["ray_count"], label


@pytest.mark.parametrize("integrator", list(INTEGRATORS))
@pytest.mark.parametrize("name", sv.EMITTERS)
def test_reduction_of_traced_sources_equals_the_rule(dev, name, integrator):
    rays = traced(name, integrator)
    worst = 0.0
    for sp, unit in ((spec_for(unit_weights=True), True), (spec_for(plane_iso=1, limb=1, weight_norm=1), False), (spec_for(plane_iso=1, limb=0, weight_norm=0), False),
                     (spec_for(unit_weights=True, labels=0), True), (spec_for(plane_iso=1, limb=1, labels=0), False)):
        want = sv.angdist(sp, rays)
        got = api.angdist_from_words(sp, reduce_on_device(dev, sp, rays)[0])
        worst = max(worst, sv.check_angdist(got, want, RTOL, (name, integrator)))
        if unit:
            exact_counts(got, want, (name, integrator))
            assert want["escape_count"] + want["return_count"] + want["lost_count"] + want["other"] + want["out_of_range"] + want["skipped"] == 1190
            assert want["out_of_range"] <= 40 and want["return_count"] + want["escape_count"] + want["lost_count"] > 1000
        host = np.zeros(api.angdist_words(sp))
        capi.check(dev.lib, dev.lib.kr_reduce_angdist_f64(C.byref(sp), rays.ctypes.data_as(C.c_void_p), len(rays), host.ctypes.data_as(C.c_void_p)), "host form")
        sv.check_angdist(api.angdist_from_words(sp, host), want, RTOL, (name, integrator, "host form"))
    parity.record_margin("test_reduction_of_traced_sources_equals_the_rule", f"{name}-{integrator}",
                         {"n_traced": 1190, "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(worst)}, allowed=RTOL)


@pytest.mark.parametrize("name", ["lamp-post", "plunge"])
def test_two_calls_into_one_buffer_sum(dev, name):
    sp = spec_for(unit_weights=True)
    a, b = traced(name, "euler"), traced(name, "rk4")
    wa, wb = reduce_on_device(dev, sp, a)[0], reduce_on_device(dev, sp, b)[0]
    _, _, d_out = reduce_on_device(dev, sp, a)
    both = reduce_on_device(dev, sp, b, d_out=d_out)[0]
    np.testing.assert_array_equal(both, wa + wb)                               # unit weights: whole numbers, exact in any order
    sp = spec_for(plane_iso=1, limb=1)
    wa, wb = reduce_on_device(dev, sp, a)[0], reduce_on_device(dev, sp, b)[0]
    _, _, d_out = reduce_on_device(dev, sp, a)
    both = reduce_on_device(dev, sp, b, d_out=d_out)[0]
    assert np.array_equal(both != 0, (wa + wb) != 0) and np.allclose(both, wa + wb, rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", sv.EMITTERS)
def test_fused_pass_equals_separate_passes(dev, name):
    rays = traced(name, "rk4")
    sp = spec_for(unit_weights=True, source_r=sv.emitter(name)[0][1], source_phi=sv.emitter(name)[0][3])       # the self-zone reads the wrapped phi
    fused_words, fused_rays, _ = reduce_on_device(dev, sp, rays, fused=True)
    sep = rays.copy()
    api.range_phi(sep)
    api.redshift(sv.SPIN, -1.0, 0, 0, sep)
    assert sep.tobytes() == fused_rays.tobytes()
    sep_words = reduce_on_device(dev, sp, sep)[0]
    np.testing.assert_array_equal(fused_words, sep_words)
    want = sv.angdist(sp, sep)
    got = api.angdist_from_words(sp, fused_words)
    sv.check_angdist(got, want, RTOL, name)
    exact_counts(got, want, name)
    assert got["bad_g"] == want["bad_g"] < 1190                                # the fused pass computed g; the reducing form of the raw records sees g = 0
    through_api = api.angdist(trace_params(capi.RK4), rays, sp)                # the public call: the same fused pass on a copy
    for k in sv.HIST_KEYS + ("total_norm", "total_az"):
        np.testing.assert_array_equal(through_api[k], got[k])


@pytest.mark.parametrize("nangle", [62, 63, 4096])
def test_bin_counts_on_both_sides_of_the_lds_limit(dev, nangle):
    sp = spec_for(dangle=2 * math.pi / (nangle + 0.5), unit_weights=True)
    assert api.angdist_nangle(sp) == nangle == sv.nangle_of(sp)
    for name in ("blob", "plunge"):
        rays = traced(name, "euler")
        want = sv.angdist(sp, rays)
        got = api.angdist_from_words(sp, reduce_on_device(dev, sp, rays)[0])
        sv.check_angdist(got, want, RTOL, (name, nangle))
        exact_counts(got, want, (name, nangle))
        assert got["total_norm"].sum() == want["ray_count"] > 1000
    spw = spec_for(dangle=2 * math.pi / (nangle + 0.5), plane_iso=1, limb=1)
    sv.check_angdist(api.angdist_from_words(spw, reduce_on_device(dev, spw, rays)[0]), sv.angdist(spw, rays), RTOL, ("weighted", nangle))


def test_edge_records_move_tallies_and_no_bin(dev):
    sp = spec_for(unit_weights=True)
    nan, inf = float("nan"), float("inf")
    cases = [("skipped", 0.0, 0.3), ("skipped", -0.0, 0.3), ("out_of_range", nan, 0.3), ("out_of_range", 0.5, nan), ("out_of_range", 0.5, inf), ("out_of_range", 0.5, -inf),
             ("out_of_range", 0.5, 4.0), ("out_of_range", 0.5, -3.5), ("out_of_range", 2.0, 0.3), ("out_of_range", -1.0000000000000002, 0.3), ("out_of_range", inf, 0.3),
             ("dead", 0.5, 0.3)]
    rays = np.zeros(len(cases) * 70, dtype=capi.RAY_F64)                      # 840 records: more than one workgroup's wave, every lane mix
    for q, (kind, c, beta) in enumerate(cases):
        sel = slice(q, None, len(cases))
        rays["alpha"][sel], rays["beta"][sel] = c, beta
        rays["steps"][sel] = 0 if kind == "dead" else 7
    rays["r"], rays["theta"], rays["redshift"] = 10.0, math.pi / 2, 1.0
    whole = rays.copy()
    whole_nan = np.frombuffer(np.full(rays.nbytes // 8, nan).tobytes(), dtype=capi.RAY_F64).copy()       # every double NaN, the integers NaN's bits
    whole_nan["steps"] = 3
    for recs, skipped, oor in ((whole, 140, 630), (whole_nan, 0, len(whole_nan))):
        for fused in (False, True):
            words = reduce_on_device(dev, sp, recs, fused=fused)[0]
            got = api.angdist_from_words(sp, words)
            assert not words[:-8].any(), (fused, np.flatnonzero(words[:-8])[:8])
            assert (got["skipped"], got["out_of_range"], got["other"], got["ray_count"]) == (skipped, oor, 0, 0.0), (fused, got)
            want = sv.angdist(sp, recs, wrap=(-math.pi, math.pi)) if not fused else None
            if want:
                assert (want["skipped"], want["out_of_range"], want["other"]) == (skipped, oor, 0)
    # a live record with good angles and a NaN radius is in the totals and in no class
    odd = np.zeros(3, dtype=capi.RAY_F64)
    odd["alpha"], odd["beta"], odd["steps"], odd["r"], odd["theta"], odd["redshift"] = 0.5, 0.3, 7, [nan, 700.0, 10.0], [1.0, 1.0, 1.0], [1.0, nan, -1.0]
    got = api.angdist_from_words(sp, reduce_on_device(dev, sp, odd)[0])
    assert (got["other"], got["ray_count"], got["bad_g"], got["total_norm"].sum(), got["total_az"].sum()) == (3, 3.0, 2, 3, 3)
    assert not any(got[k].any() for k in sv.HIST_KEYS)


def test_disc_source_classes_equal_the_landing_maps(dev, krlib):
    """The Keplerian disc source at r = 3 of disc_source_return_angdist.cpp, as a PointSourceVel with u = (1, 0, 0, V), over its whole sky: the half
    that starts into the disc lands in the source's own zone at once and is in no class on either side.  With dangle = 0.1 the 62 bins end at
    -pi + 6.2 = 3.058 and six rays of this grid, whose azimuth lies beyond, are out of range (where the reference's array index is): such rays are in
    none of the angular sums and would be in the landing map's.  So the bins here are 62 that cover the whole circle, and no ray is left out."""
    V = krlib.kr_disc_velocity(3.0, sv.SPIN, 1)
    pos = (0.0, 3.0, math.pi / 2 - 1e-6, 1.5707)
    vel = api.pointsource_vel_spec(pos, (1.0, 0.0, 0.0, V), sv.SPIN, 0.06, 0.18, beta0=-3.1, betamax=3.0)
    sp = spec_for(dangle=2 * math.pi / 62.000001, unit_weights=True, source_r=3.0, source_phi=1.5707)
    assert api.angdist_nangle(sp) == 62
    res = api.source_angdist(vel, trace_params(capi.EULER), sp, return_records=True)
    rays = res["records"]
    assert res["skipped"] == 0 and res["out_of_range"] == 0 and res["stats"]["rays_traced"] == (rays["steps"] > 0).sum() > 1000
    m = api.return_map_struct(sp.cls.r_isco, R_DISC, R_ESC, 3.0, 1.5707, 1.0, 5.0, 100, False, plane_iso=0, limb=0, weight_norm=0)
    landing = api.reduce_return_map(m, rays)
    for k in ("escape", "return", "lost"):
        assert res[k + "_sum"] == landing[k], (k, res[k + "_sum"], landing[k])
    assert res["ray_count"] == landing["ray_count"] and res["return_sum"] > 50 and res["escape_sum"] > 50
    for k in ("escape", "return", "lost"):
        assert res[k + "_frac"] == landing[k] / landing["ray_count"]
    # and the rule on the final records, which the fused pass wrapped and shifted
    want = sv.angdist(sp, rays)
    sv.check_angdist(res, want, RTOL, "disc source")
    exact_counts(res, want, "disc source")
