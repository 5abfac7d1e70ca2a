"""GPU: the HEALPix point source and the fate map of its sky (csrc/kr_healpix.hip) against the numpy restatement of their rules
(tests/healpix_rules.py), the reference's own pixel vectors (tests/golden/healpix_vectors.npz) and the CPU oracle's trace.

The four sources: the lamp-post (0, 5, 1e-3, 1.5707), a = 0.998, at rest; the jet, the same source moving outward at dr/dt = 0.3; an orbiting source
(0, 6, 1.2, 1.5707), a = 0.9, V = 0.06411, basis 1; and a source on the disc (0, 6, pi/2 - 1e-6, 1.5707), a = 0.9, in Keplerian motion, basis 1,
whose own neighbourhood on the disc is the self-zone.  Everything runs at orders 0 and 3 (12 and 768 pixels); one call at order 12 takes the
large-index integer path without allocating the sphere.  Traces stop at theta = pi/2 or r = 1000; the map takes r_esc = 999 (the Euler trace ends
a ray AT r_max) and r_disc = 2000 > r_max, so that theta_tol decides the class of rays that leave just above the plane."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import healpix_rules as hr
import oracle_lib as ol
import parity
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
GEOMETRY_ATOL = 4.5e-16                  # tests/test_healpix_rules.py: 1 ulp of sin / cos, one more rounding, operands <= 1
EMIS_RTOL = parity.BIN_RTOL              # the bound tests/test_gpu_reducers.py gives the image reducer's flux plane (powerlaw3(r) / g^3 there as here)
SOURCES = ("lamp-post", "jet", "orbiting", "on-disc")


def source(name, order=3, rays_per_pixel=1, E=1.0, unit_center=0):
    if name == "lamp-post":
        return api.healpix_spec((0.0, 5.0, 1e-3, 1.5707), 0.0, 0.998, order, 0, 0, rays_per_pixel, unit_center, E)
    if name == "jet":
        return api.healpix_spec((0.0, 5.0, 1e-3, 1.5707), 0.3, 0.998, order, 1, 0, rays_per_pixel, unit_center, E)
    if name == "orbiting":
        return api.healpix_spec((0.0, 6.0, 1.2, 1.5707), 0.06411, 0.9, order, 0, 1, rays_per_pixel, unit_center, E)
    return api.healpix_spec((0.0, 6.0, math.pi / 2 - 1e-6, 1.5707), api.lib().kr_disc_velocity(6.0, 0.9, 1), 0.9, order, 0, 1, rays_per_pixel, unit_center, E)


def trace_params(spin, integrator):
    p = capi.default_params(spin)
    p.integrator, p.r_max, p.theta_max, p.stop_kind = integrator, 1000.0, math.pi / 2, capi.STOP_THETA
    return p


def fate_map(spec, theta_tol=0.0, self_zone=0, rays_per_pixel=None):
    rpp = spec.rays_per_pixel if rays_per_pixel is None else rays_per_pixel
    return api.healpix_map_struct(hr.npix_of(spec.order), api.lib().kr_kerr_isco(spec.spin, 1), 2000.0, 999.0, theta_tol, spec.pos[1], spec.pos[3], self_zone, rpp,
                                  q1=7.0, rb1=4.0, q2=0.0, rb2=10.0, q3=3.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture
def dev(krlib):
    """Device buffers of one test, freed at its end."""
    with DeviceScope(api.lib()) as scope:
        yield scope


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "healpix_vectors.npz"))
    return z["order"], z["pix"], z["bits"].view(np.float64)


@pytest.fixture(scope="module")
def sphere3(krlib):
    """The device's own vectors of order 0 and order 3, computed once."""
    return {o: api.healpix_vectors(o) for o in (0, 3)}


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------
def test_vectors_match_reference_fixture(dev, fixture):
    order, pix, want = fixture
    got = np.zeros_like(want)
    for o in np.unique(order):
        idx = np.flatnonzero(order == o)
        d = dev.alloc(max(len(idx) * 120, 8))
        if o <= 3:
            capi.check(dev.lib, dev.lib.kr_healpix_vectors_dev_f64(int(o), 0, 0, 1, len(idx), d, None), "kr_healpix_vectors")
        else:
            for q, p in enumerate(pix[idx]):
                capi.check(dev.lib, dev.lib.kr_healpix_vectors_dev_f64(int(o), 0, int(p), 1, 1, vp(d.value + 120 * q), None), "kr_healpix_vectors")
        got[idx] = dev.fetch(d, len(idx) * 15).reshape(-1, 15)
    worst = float(np.abs(got - want).max())
    differ = int((bits(got) != bits(want)).sum())
    print(f"device vectors against the reference's: worst |difference| {worst:.3e}, {differ} of {want.size} components not bit-identical")
    parity.record_margin("test_vectors_match_reference_fixture", "orders 0-3, 8, 12", {"n_traced": int(want.size), "n_bad": differ, "frac_bad": differ / want.size,
                         "worst_ok": worst}, allowed=GEOMETRY_ATOL, bar="|component - reference's| <= 4.5e-16; n_bad counts components that are not bit-identical")
    assert worst <= GEOMETRY_ATOL


def test_strided_vectors_and_unit_centre(sphere3):
    whole = sphere3[3]
    assert same_bits(api.healpix_vectors(3, first_pix=5, stride=7), whole[5::7])
    unit = api.healpix_vectors(3, unit_center=1)
    assert same_bits(unit[:, :12], whole[:, :12])
    c = unit[:, 12:]
    assert np.abs(np.sqrt((c * c).sum(axis=1)) - 1).max() <= 2.3e-16
    assert same_bits(c, hr.centre_of(unit[:, :12].reshape(-1, 4, 3), unit_center=True))          # the rule on the device's own corners
    assert same_bits(whole[:, 12:], hr.centre_of(whole[:, :12].reshape(-1, 4, 3)))
    plain = np.sqrt((whole[:, 12:] ** 2).sum(axis=1))
    assert 0.99455 < plain.min() and plain.max() < 0.99605              # not normalised: 0.9946 ... 0.9960 to four digits


# ---- constants ---------------------------------------------------------------------------------------------------------------------------------
def check_records(spec, rays, vec15, label):
    v = hr.source_vectors(spec, vec15)
    want = hr.records(spec, v, beta=rays["beta"])
    bad = ol.rays_equal_bitwise(rays, want)
    assert not bad, f"{label}: {bad}"
    assert np.abs(rays["beta"] - np.arctan2(v[:, 1], v[:, 0])).max() <= 4.5e-16, label      # atan2: correctly rounded against numpy's, <= 1 ulp of pi


@pytest.mark.parametrize("name", SOURCES)
def test_records_equal_rule_on_device_vectors(name, sphere3):
    for order in (0, 3):
        five = api.healpix_init(source(name, order, 5), emit=False)
        one = api.healpix_init(source(name, order, 1), emit=False)
        assert len(five) == 5 * hr.npix_of(order) and len(one) == hr.npix_of(order)
        check_records(source(name, order, 5), five, sphere3[order], f"{name} order {order}, 5 rays per pixel")
        check_records(source(name, order, 1), one, sphere3[order], f"{name} order {order}, centres")
        assert not ol.rays_equal_bitwise(one, five[4::5])
        for rpp, whole in ((5, five), (1, one)):
            s = source(name, order, rpp)
            shards = [api.healpix_init(s, emit=False, first=f, stride=2) for f in (0, 1)]
            w = whole.reshape(-1, rpp)
            assert not ol.rays_equal_bitwise(shards[0], np.ascontiguousarray(w[0::2]).ravel()) and not ol.rays_equal_bitwise(shards[1], np.ascontiguousarray(w[1::2]).ravel())


def test_unit_centre_changes_only_the_centre_rays(sphere3):
    plain = api.healpix_init(source("jet", 3, 5), emit=False)
    unit = api.healpix_init(source("jet", 3, 5, unit_center=1), emit=False)
    assert not ol.rays_equal_bitwise(plain.reshape(-1, 5)[:, :4].ravel(), unit.reshape(-1, 5)[:, :4].ravel())
    check_records(source("jet", 3, 5, unit_center=1), unit, api.healpix_vectors(3, unit_center=1), "unit centre")
    assert (plain["k"][4::5] != unit["k"][4::5]).any()


def test_order_12_shard_takes_the_large_pixel_path(fixture):
    order, pix, want = fixture
    nside = 1 << 12
    first = 12 * nside * nside - 2 * nside * (nside - 1)                 # npix - ncap: a fixture pixel, 151 million pixels into the sphere
    row = np.flatnonzero((order == 12) & (pix == first))
    assert len(row) == 1
    vec = api.healpix_vectors(12, first_pix=first, stride=1, count=64)
    assert np.abs(vec[0] - want[row[0]]).max() <= GEOMETRY_ATOL
    assert np.abs(vec - hr.pixel_vectors(12, first + np.arange(64))).max() <= GEOMETRY_ATOL
    for name in ("jet", "orbiting"):
        s = source(name, 12, 1)
        rays = api.healpix_init(s, emit=False, first=first, stride=1, count=64)
        check_records(s, rays, vec, f"{name} order 12")
    s5 = source("jet", 12, 5)
    rays5 = api.healpix_init(s5, emit=False, first=first, stride=3, count=5 * 8)
    check_records(s5, rays5, api.healpix_vectors(12, first_pix=first, stride=3, count=8), "jet order 12, strided, 5 rays per pixel")
    last = api.healpix_vectors(13, first_pix=12 * 4 ** 13 - 1, count=1)                  # the last pixel of the largest sphere
    assert np.abs(last - hr.pixel_vectors(13, np.array([12 * 4 ** 13 - 1]))).max() <= GEOMETRY_ATOL


# ---- emit --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("lamp-post", "orbiting", "on-disc"))
def test_fused_emit_equals_redshift_start(name):
    for reverse in (0, 1):
        s = source(name, 3, 5)
        fused = api.healpix_init(s, emit=True, reverse=reverse)
        separate = api.redshift_start(s.spin, s.V, reverse, 0, api.healpix_init(s, emit=False))
        assert not ol.rays_equal_bitwise(fused, separate), (name, reverse)


def emit_deviation(name, rays_per_pixel, unit_center=0):
    rays = api.healpix_init(source(name, 3, rays_per_pixel, unit_center=unit_center), emit=True, reverse=0)
    return np.abs(rays["emit"] / 1.0 - 1)


@pytest.mark.parametrize("name", SOURCES)
def test_emitted_energy_is_E_in_the_source_frame(name):
    """|emit / E - 1| <= 1e-12 on every ray, both motions, reverse = 0: p . u = E in the frame the photon was launched in (the orbital frame on the jet
    would give 0.587 ... 1.704).  The radially moving source takes the product with the momentum its tetrad launched the photon with: rebuilt from
    k, h, Q through the null condition, p^r of the reference's un-normalised centre vectors (|v| = 0.9946 ... 0.9960) put the jet's centre rays 4.3e-2
    off (profiles/healpix_parity.json)."""
    for rpp in (5, 1):
        dev = emit_deviation(name, rpp)
        print(f"{name}, {rpp} ray(s) per pixel: worst |emit / E - 1| = {dev.max():.3e}" + (f" (corners alone {dev.reshape(-1, 5)[:, :4].max():.3e})" if rpp == 5 else ""))
        assert dev.max() <= 1e-12


def test_jet_emits_E_on_unit_centres_and_reversed():
    for rpp in (5, 1):
        dev = emit_deviation("jet", rpp, unit_center=1)
        print(f"jet, unit centres, {rpp} ray(s) per pixel: worst |emit / E - 1| = {dev.max():.3e}")
        assert dev.max() <= 1e-12
    # reverse = 1 negates the spatial momentum and the spin of the metric: on the axis (sin theta = 1e-3) the frame-dragging term is negligible, so
    # g_tt u^t p^t stays and the radial term changes sign -- the photon launched along +r is the one launched along -r seen running backwards
    fwd = api.healpix_init(source("jet", 0, 5), emit=True, reverse=0)
    back = api.healpix_init(source("jet", 0, 5), emit=True, reverse=1)
    assert not ol.rays_equal_bitwise(fwd, back, fields=[f for f in fwd.dtype.names if f != "emit"])
    assert np.isfinite(back["emit"]).all() and (back["emit"] > 0).all() and (back["emit"] != fwd["emit"]).any()


@pytest.mark.parametrize("name", SOURCES)
def test_energy_scales_the_record(name):
    """E = 2.5 scales k, h and emit by 2.5 and Q by 6.25 to within 4 ulp of the value: the record is the unit-energy record scaled, so each is one
    rounding away (calc_consts_from_vector's own rule, E carried through its sums, leaves h and Q up to 589 and 53 ulp off where their terms cancel).  The
    scaled record is the numpy rule's bit for bit as well."""
    one = api.healpix_init(source(name, 3, 5), emit=True)
    big = api.healpix_init(source(name, 3, 5, E=2.5), emit=True)
    assert np.array_equal(big["rdot_sign"], one["rdot_sign"]) and np.array_equal(big["thetadot_sign"], one["thetadot_sign"])
    worst = {f: float(np.abs(big[f] / (scale * one[f]) - 1).max() / 2.0 ** -52) for f, scale in (("k", 2.5), ("h", 2.5), ("emit", 2.5), ("Q", 6.25))}
    print(f"{name}: E = 2.5 against E = 1, worst relative difference in ulp: {worst}")
    assert max(worst.values()) <= 4
    check_records(source(name, 3, 5, E=2.5), api.healpix_init(source(name, 3, 5, E=2.5), emit=False), api.healpix_vectors(3), f"{name} E = 2.5")


# ---- fate pass ---------------------------------------------------------------------------------------------------------------------------------
_traced = {}


def traced(name, integrator, rays_per_pixel=1):
    """The order-3 rays of a source after the device trace, before any pass; computed once and never modified."""
    key = (name, integrator, rays_per_pixel)
    if key not in _traced:
        s = source(name, 3, rays_per_pixel)
        out, _ = api.trace(trace_params(s.spin, integrator), api.healpix_init(s, emit=True))
        out.setflags(write=False)
        _traced[key] = out
    return _traced[key]


def post_on_device(dev, spec, m, rays, first=0, stride=1, d_out=None):
    d_rays = dev.upload(np.ascontiguousarray(rays))
    d_out = d_out or dev.zeros(8 * api.healpix_map_words(m))
    capi.check(dev.lib, dev.lib.kr_post_healpix_map_dev_f64(spec.spin, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(m), d_rays, len(rays), first, stride, d_out, None), "kr_post_healpix_map")
    words = dev.fetch(d_out, api.healpix_map_words(m))
    return api.healpix_map_from_words(m, words), dev.fetch(d_rays, len(rays), capi.RAY_F64), d_out


def separate_passes(spec, rays):
    out = rays.copy()
    api.range_phi(out)
    return api.redshift(spec.spin, -1.0, 0, 0, out, motion=0)


def check_map(got, m, centres, label):
    cls = hr.classify(m, centres)
    assert np.array_equal(got["class"], cls), label
    for plane, field in (("r", "r"), ("theta", "theta"), ("phi", "phi"), ("g", "redshift"), ("t", "t")):
        assert same_bits(got[plane], centres[field]), (label, plane)
    t = hr.tallies(cls)
    assert [got[k] for k in api.HEALPIX_TALLIES] == [int(x) for x in t[:5]], label
    with np.errstate(invalid="ignore", divide="ignore"):
        emis = np.where(cls == 1, hr.powerlaw3(centres["r"], m.q1, m.rb1, m.q2, m.rb2, m.q3) / centres["redshift"] ** 3.0, 0.0)
    assert (got["emis"][cls != 1] == 0).all(), label
    np.testing.assert_allclose(got["emis"][cls == 1], emis[cls == 1], rtol=EMIS_RTOL, atol=0, err_msg=label)
    return cls


@pytest.mark.parametrize("name", SOURCES)
def test_fate_pass_equals_separate_passes_and_rule(name, dev):
    for integrator in (capi.EULER, capi.RK4):
        for rpp in (1, 5):
            if rpp == 5 and integrator == capi.RK4:
                continue
            spec = source(name, 3, rpp)
            rays = traced(name, integrator, rpp)
            want = separate_passes(spec, rays)
            for theta_tol, self_zone in ((0.0, 0), (1e-2, 1)):
                m = fate_map(spec, theta_tol, self_zone)
                got, after, _ = post_on_device(dev, spec, m, rays)
                label = f"{name} integrator {integrator} rpp {rpp} tol {theta_tol} self {self_zone}"
                if rpp == 1:
                    assert not ol.rays_equal_bitwise(after, want), label
                else:                                                       # the pass touches the centre records only
                    assert not ol.rays_equal_bitwise(after[4::5], want[4::5]) and not ol.rays_equal_bitwise(after.reshape(-1, 5)[:, :4].ravel(), rays.reshape(-1, 5)[:, :4].ravel()), label
                centres = want if rpp == 1 else want[4::5]
                check_map(got, m, centres, label)
                if rpp == 1:                                                # the reducing form's host entry on the finished records
                    check_same_map(api.reduce_healpix_map(m, want), got, label + " (kr_reduce_healpix_map_f64)")


def check_same_map(a, b, label):
    """Two fate maps: every plane bit for bit, every tally equal."""
    for k in api.HEALPIX_PLANES:
        assert np.array_equal(a[k], b[k]) if k == "class" else same_bits(a[k], b[k]), (label, k)
    assert [a[k] for k in api.HEALPIX_TALLIES] == [b[k] for k in api.HEALPIX_TALLIES], label


def reduce_on_device(dev, m, rays, first=0, stride=1, d_out=None):
    d_rays = dev.upload(np.ascontiguousarray(rays))
    d_out = d_out or dev.zeros(8 * api.healpix_map_words(m))
    capi.check(dev.lib, dev.lib.kr_reduce_healpix_map_dev_f64(C.byref(m), d_rays, len(rays), first, stride, d_out, None), "kr_reduce_healpix_map_dev")
    after = dev.fetch(d_rays, len(rays), capi.RAY_F64)
    assert not ol.rays_equal_bitwise(after, rays)                          # the reducing form reads
    return api.healpix_map_from_words(m, dev.fetch(d_out, api.healpix_map_words(m))), d_out


@pytest.mark.parametrize("rpp", (1, 5))
def test_reducing_form_on_device_equals_fused_pass(dev, rpp):
    """kr_reduce_healpix_map_dev_f64 on records that range_phi and redshift have finished: the planes and tallies of kr_post_healpix_map_dev_f64 on
    the traced ones, whole and as two interleaved shards into one buffer."""
    spec = source("on-disc", 3, rpp)
    rays = traced("on-disc", capi.EULER, rpp)
    m = fate_map(spec, 1e-2, 1)
    fused, finished, _ = post_on_device(dev, spec, m, rays)
    whole, _ = reduce_on_device(dev, m, finished)
    check_same_map(whole, fused, f"whole, {rpp} per pixel")
    w = finished.reshape(-1, rpp)
    _, d_out = reduce_on_device(dev, m, np.ascontiguousarray(w[0::2]).ravel(), first=0, stride=2)
    both, _ = reduce_on_device(dev, m, np.ascontiguousarray(w[1::2]).ravel(), first=1, stride=2, d_out=d_out)
    check_same_map(both, fused, f"two shards, {rpp} per pixel")


def test_dead_records_are_class_0_in_both_forms(dev):
    """Unused slots (steps = -1) and rays that hit the step limit (steps < -1) among live ones: class 0, out of every tally, their record's values
    still in the planes, phi not wrapped; the fused pass stores their redshift as kr_redshift_dev_f64 does."""
    spec = source("orbiting", 3, 1)
    rays = traced("orbiting", capi.EULER, 1).copy()
    dead = np.arange(0, 768, 7)
    rays["steps"][dead[0::2]] = -1
    rays["steps"][dead[1::2]] = -500
    rays["phi"][dead[:4]] += 20.0                                         # outside [-pi, pi): a live record would be wrapped
    m = fate_map(spec, 1e-2, 0)
    want = separate_passes(spec, rays)
    got, after, _ = post_on_device(dev, spec, m, rays)
    assert not ol.rays_equal_bitwise(after, want)
    cls = check_map(got, m, want, "dead records, fused")
    assert (cls[dead] == 0).all() and got["live"] == 768 - len(dead) and same_bits(got["phi"][dead[:4]], rays["phi"][dead[:4]])
    check_same_map(reduce_on_device(dev, m, want)[0], got, "dead records, reducing form")


def test_disc_source_kills_the_rays_that_start_into_the_disc(sphere3):
    """disc_source = 1 (the reference's set_disc_source()): steps = -1 where thetadot_sign > 0, every other field as without it; about half the
    sphere of a source on the disc; the trace passes over those slots and the fate map has them as class 0."""
    plain = api.healpix_init(source("on-disc", 3, 5), emit=True)
    spec = api.healpix_spec((0.0, 6.0, math.pi / 2 - 1e-6, 1.5707), api.lib().kr_disc_velocity(6.0, 0.9, 1), 0.9, 3, 0, 1, 5, disc_source=1)
    up = api.healpix_init(spec, emit=True)
    assert np.array_equal(up["steps"], np.where(plain["thetadot_sign"] > 0, -1, 0))
    assert not ol.rays_equal_bitwise(up, plain, fields=[f for f in up.dtype.names if f != "steps"])
    check_records(spec, api.healpix_init(spec, emit=False), sphere3[3], "disc source")
    centres = up[4::5]
    assert 0.45 * 768 <= (centres["steps"] == 0).sum() <= 0.55 * 768
    one = api.healpix_spec((0.0, 6.0, math.pi / 2 - 1e-6, 1.5707), spec.V, 0.9, 3, 0, 1, 1, disc_source=1)
    res = api.healpix_map(one, trace_params(0.9, capi.EULER), fate_map(one, 0.0, 1), return_records=True)
    assert res["live"] == int((centres["steps"] == 0).sum()) and np.array_equal(res["class"] == 0, centres["steps"] == -1)
    assert not ol.rays_equal_bitwise(res["records"][centres["steps"] == -1], api.redshift(0.9, -1.0, 0, 0, centres[centres["steps"] == -1].copy()))
    assert res["live"] == res["disc"] + res["escape"] + res["lost"] + res["self"] and res["escape"] > 200


def test_fate_pass_shards_write_disjoint_pixels_and_sum_tallies(dev):
    spec = source("orbiting", 3, 5)
    rays = traced("orbiting", capi.EULER, 5)
    m = fate_map(spec, 1e-2, 1)
    whole, _, _ = post_on_device(dev, spec, m, rays)
    w = rays.reshape(-1, 5)
    first_half, _, d_out = post_on_device(dev, spec, m, np.ascontiguousarray(w[0::2]).ravel(), first=0, stride=2)
    assert (first_half["class"][1::2] == 0).all() and (first_half["r"][1::2] == 0).all()          # the other shard's pixels are untouched
    both, _, _ = post_on_device(dev, spec, m, np.ascontiguousarray(w[1::2]).ravel(), first=1, stride=2, d_out=d_out)
    for k in api.HEALPIX_PLANES:
        assert same_bits(both[k], whole[k]) if k != "class" else np.array_equal(both[k], whole[k]), k
    assert [both[k] for k in api.HEALPIX_TALLIES] == [whole[k] for k in api.HEALPIX_TALLIES]
    assert first_half["live"] == 384


def test_theta_tol_and_self_zone_each_decide_a_class(dev):
    spec = source("on-disc", 3, 1)
    rays = traced("on-disc", capi.EULER, 1)
    maps = {(tol, sz): post_on_device(dev, spec, fate_map(spec, tol, sz), rays)[0]["class"] for tol in (0.0, 1e-2) for sz in (0, 1)}
    by_tol = maps[(0.0, 0)] != maps[(1e-2, 0)]
    assert by_tol.any() and set(maps[(0.0, 0)][by_tol]) == {2} and set(maps[(1e-2, 0)][by_tol]) == {1}
    by_zone = maps[(0.0, 0)] != maps[(0.0, 1)]
    assert by_zone.any() and set(maps[(0.0, 0)][by_zone]) == {1} and set(maps[(0.0, 1)][by_zone]) == {4}
    print(f"theta_tol moves {int(by_tol.sum())} pixels from escape to disc, self_zone {int(by_zone.sum())} from disc to self-zone")


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
_oracle_classes = {}


def end_to_end(name):
    spec = source(name, 3, 1)
    m = fate_map(spec, 0.0, 1 if name == "on-disc" else 0)
    p = trace_params(spec.spin, capi.EULER)
    got = api.healpix_map(spec, p, m)
    start = api.healpix_init(spec, emit=True)
    ref, _ = ol.oracle_trace(p, start)
    ol.oracle().kro_range_phi_f64(-math.pi, math.pi, ol.ptr(ref), len(ref))
    ol.oracle().kro_redshift_f64(spec.spin, -1.0, 0, 0, 0, ol.ptr(ref), len(ref))
    cls = hr.classify(m, ref)
    _oracle_classes[name] = cls
    return got, cls


@pytest.mark.parametrize("name", SOURCES)
def test_healpix_map_against_oracle_trace(name):
    got, cls = end_to_end(name)
    t = hr.tallies(cls).astype(int)
    differ = int((got["class"] != cls).sum())
    print(f"{name}: oracle live / disc / escape / lost / self = {t[:5].tolist()}; device classes differ at {differ} of 768 pixels")
    parity.record_margin("test_healpix_map_against_oracle_trace", name, {"n_traced": 768, "n_bad": differ, "frac_bad": differ / 768, "worst_ok": 0.0}, allowed=7 / 768,
                         bar="pixels whose class differs from the oracle-traced rays' <= 1 %")
    assert differ <= 7
    assert got["live"] == 768 and got["disc"] + got["escape"] + got["lost"] + got["self"] == 768
    assert abs(got["disc_frac"] + got["escape_frac"] + got["lost_frac"] + got["self_frac"] - 1) < 1e-12
    if name != "on-disc":
        want = {"lamp-post": (488, 240, 40), "jet": (342, 412, 14), "orbiting": (453, 272, 43)}[name]
        assert tuple(t[1:4]) == want                                     # the inputs are the ones the bounds below were chosen for
        assert t[1] >= 300 and t[2] >= 200 and t[3] >= 10


def test_outflow_beams_away_from_the_disc():
    for name in ("lamp-post", "jet"):
        if name not in _oracle_classes:
            end_to_end(name)
    disc = {name: int((_oracle_classes[name] == 1).sum()) for name in ("lamp-post", "jet")}
    assert disc["jet"] < disc["lamp-post"] - 100
    spec = source("jet", 3, 1)
    got = api.healpix_map(spec, trace_params(spec.spin, capi.EULER), fate_map(spec))
    rest = source("lamp-post", 3, 1)
    got_rest = api.healpix_map(rest, trace_params(rest.spin, capi.EULER), fate_map(rest))
    assert got["disc"] < got_rest["disc"] - 100
