"""GPU: the source-to-observer link (kr_post_observer_dev_f64 / kr_reduce_observer_dev_f64, csrc/kr_observer.hip) against the numpy restatement of
tests/observer_rules.py applied to the records fetched from the device.  The sources -- the lamp posts ps_h5 and ps_h10 of the golden cases (1260 rays
each, Euler and RK4), an orbiting and outflowing blob with its own four-velocity, a HEALPix source at order 2 (centres only) -- are traced once per
module to r_max = 700, so that the reference sphere at dist = 1000 is a real way off.

  counts     every tally and every count equals the rule EXACTLY.  The device's log and pow are not correctly rounded and the rule's momentum takes
             numpy's sin / cos, so each fixture first asserts that no record of the rule lies within 1e-9 (relative) of an inclination-bin or time-row edge
  sums       weighted sums within parity.BIN_RTOL of the per-bin sum of absolute terms (the device adds in whatever order the atomics arrive)
  adds       two calls into one buffer equal the sum of two buffers
  fused      kr_post_observer_dev_f64 leaves phi and redshift as kr_range_phi_dev_f64 + kr_redshift_dev_f64 do and counts as kr_reduce_observer_dev_f64
             counts those records, bit for bit
  n          0, 1, 63, 64, 65, 255, 256, 257 records: a wave's and a workgroup's ragged end
  shapes     nmu = 1, 2, 33; nt = 0, 1, 64; 75 x 68 = 5100 words (planes in LDS) and 76 x 68 = 5168 (global adds, grouped by wave)
  weights    gamma = 0 and 2; dist = 0 and 1000
  edges      the constructed records of tests/test_observer_rules.py: on and beside every edge of both index rules, NaN t, pr = 0, shift = 0
  api        api.source_to_observer for the three source kinds, feeding api.direct_arrival -> capi.response_model(t0=...)
  program    kr_source_observer against the API
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import golden_cases as gc
import observer_rules as obr
import parity
import source_vel_rules as sv
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu
RTOL = parity.BIN_RTOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPIN = gc.SPIN
R_DISC, R_ESC, R_MAX = 400.0, 650.0, 700.0
EDGE = 1e-9
SOURCES = [("ps_h5", "euler"), ("ps_h5", "rk4"), ("ps_h10", "euler"), ("ps_h10", "rk4"), ("blob", "rk4"), ("healpix", "rk4")]
INTEGRATORS = {"euler": capi.EULER, "rk4": capi.RK4}


def trace_params(integrator, r_max=R_MAX):
    p = capi.default_params(SPIN)
    p.integrator, p.r_max, p.theta_max, p.stop_kind = integrator, r_max, math.pi / 2, capi.STOP_THETA
    return p


def healpix_source():
    return api.healpix_spec((0.0, 5.0, 1e-3, 1.5707), 0.0, SPIN, 2, 0, 0, 1)


@pytest.fixture
def dev(krlib):
    with DeviceScope(krlib) as scope:
        yield scope


_TRACED = {}


def traced(name, integrator):
    """The records of one source after its constructor with the emitted energy and kr_trace_dev_f64, fetched once per module and never modified."""
    key = (name, integrator)
    if key not in _TRACED:
        L = api.lib()
        with DeviceScope(L) as scope:
            if name.startswith("ps_"):
                init = np.ascontiguousarray(np.load(gc.golden_path(name))["init"])          # the constructor's records after redshift_start(V = 0)
                n, d = len(init), scope.upload(init)
            elif name == "blob":
                spec = sv.spec_of("blob")
                n = api.pointsource_vel_count(spec)[0]
                d = scope.alloc(n * capi.RAY_F64.itemsize)
                capi.check(L, L.kr_pointsource_vel_init_emit_dev_f64(C.byref(spec), d, n, None), "init_emit")
            else:
                spec = healpix_source()
                n = api.healpix_count(spec)[0]
                d = scope.alloc(n * capi.RAY_F64.itemsize)
                capi.check(L, L.kr_healpix_init_emit_dev_f64(C.byref(spec), 0, 1, 0, d, n, None), "healpix_init_emit")
            capi.check(L, L.kr_trace_dev_f64(C.byref(trace_params(INTEGRATORS[integrator])), d, n, None, None), "trace")
            rays = scope.fetch(d, n, capi.RAY_F64)
        used = int((rays["steps"] != -1).sum())                                    # (the grid's unused slots carry steps = -1)
        assert used == {"ps_h5": 1260, "ps_h10": 1260, "healpix": 192}.get(name, used) and (rays["steps"] > 0).sum() > 150
        rays.setflags(write=False)
        _TRACED[key] = rays
    return _TRACED[key]


def spec_for(rays, nmu=33, nt=64, gamma=2.0, dist=1000.0, wrap=None, **kw):
    """A spec whose bins suit the records: odd mu0 and dmu that cover most of the upper hemisphere, time rows over the middle of the arrival times
    (so that some rays fall outside on either side).  Asserts the edge condition on the rule's side and returns (spec, the rule's result)."""
    mu0, dmu = 0.0137, 0.9431 / nmu
    probe = obr.per_ray(api.observer_spec(SPIN, gc.r_isco(), R_DISC, R_ESC, nmu=nmu, mu0=mu0, dmu=dmu, gamma=gamma, dist=dist, **kw), rays, wrap)
    t = probe["t_ref"][probe["binned"]]
    t0, dt = 0.0, 0.0
    if nt > 0:
        lo, hi = t.min() + 0.2137 * (t.max() - t.min()), t.min() + 0.8291 * (t.max() - t.min())
        t0, dt = float(lo), float(hi - lo) / nt
    sp = api.observer_spec(SPIN, gc.r_isco(), R_DISC, R_ESC, nmu=nmu, mu0=mu0, dmu=dmu, gamma=gamma, dist=dist, t0=t0, dt=dt, nt=nt, **kw)
    want = obr.observer(sp, rays, wrap)
    assert obr.edge_margin(want) > EDGE, ("a record of the rule lies on a bin edge: choose other bins", obr.edge_margin(want))
    return sp, want


def reduce_on_device(dev, sp, rays, d_out=None, fused=False):
    """(words, records afterwards, the buffer) of one pass over a device copy of `rays`; d_out: a buffer to add into"""
    L, nw, n = dev.lib, api.observer_words(sp), len(rays)
    d_rays = dev.upload(np.ascontiguousarray(rays)) if n > 0 else C.c_void_p()
    d_out = d_out if d_out is not None else dev.zeros(nw * 8)
    if fused:
        capi.check(L, L.kr_post_observer_dev_f64(SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(sp), d_rays, n, d_out, None), "kr_post_observer")
    else:
        capi.check(L, L.kr_reduce_observer_dev_f64(C.byref(sp), d_rays, n, d_out, None), "kr_reduce_observer")
    return dev.fetch(d_out, nw), dev.fetch(d_rays, n, capi.RAY_F64), d_out


SHAPES = [dict(nmu=1, nt=0, gamma=0.0, dist=0.0), dict(nmu=2, nt=1, gamma=2.0, dist=1000.0), dict(nmu=33, nt=64, gamma=2.0, dist=1000.0),
          dict(nmu=33, nt=64, gamma=0.0, dist=0.0), dict(nmu=2, nt=64, gamma=2.0, dist=0.0), dict(nmu=33, nt=1, gamma=0.0, dist=1000.0),
          dict(nmu=75, nt=64, gamma=2.0, dist=1000.0), dict(nmu=76, nt=64, gamma=2.0, dist=1000.0), dict(nmu=76, nt=64, gamma=0.0, dist=0.0)]


@pytest.mark.parametrize("name,integrator", SOURCES)
def test_reduction_of_traced_sources_equals_the_rule(dev, name, integrator):
    rays = traced(name, integrator)
    worst = 0.0
    for shape in SHAPES:
        sp, want = spec_for(rays, **shape)
        assert want["binned"] + want["outside_mu"] + want["inbound"] + want["bad_g"] == want["escape"] > 30
        assert shape["nt"] == 0 or 0 < want["outside_time"] < want["binned"]
        got = api.observer_from_words(sp, reduce_on_device(dev, sp, rays)[0])
        worst = max(worst, obr.check_observer(got, want, RTOL, (name, integrator, shape)))
        if shape["gamma"] == 0:                                              # unit weights: whole numbers, exact in any order
            np.testing.assert_array_equal(got["sum_w"], want["count"])
            np.testing.assert_array_equal(got["hist"], want["hist_n"])
    sp, want = spec_for(rays)
    host = api.reduce_observer(sp, np.ascontiguousarray(rays))
    obr.check_observer(host, want, RTOL, (name, integrator, "host form"))
    parity.record_margin("test_reduction_of_traced_sources_equals_the_rule", f"{name}-{integrator}",
                         {"n_traced": int((rays["steps"] > 0).sum()), "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(worst)}, allowed=RTOL)


@pytest.mark.parametrize("nmu", [33, 76])
def test_two_calls_into_one_buffer_sum(dev, nmu):
    a, b = traced("ps_h10", "euler"), traced("ps_h5", "rk4")
    both_rays = np.concatenate([a, b])
    for gamma in (0.0, 2.0):
        sp, _ = spec_for(both_rays, nmu=nmu, gamma=gamma)
        wa, wb = reduce_on_device(dev, sp, a)[0], reduce_on_device(dev, sp, b)[0]
        _, _, d_out = reduce_on_device(dev, sp, a)
        both = reduce_on_device(dev, sp, b, d_out=d_out)[0]
        if gamma == 0:
            nw = 4 * nmu
            np.testing.assert_array_equal(np.delete(both, np.s_[2 * nmu:nw]), np.delete(wa + wb, np.s_[2 * nmu:nw]))      # (sum_ws, sum_wt: not whole numbers)
        assert np.array_equal(both != 0, (wa + wb) != 0) and np.allclose(both, wa + wb, rtol=RTOL, atol=0)
        np.testing.assert_array_equal(both[-10:], (wa + wb)[-10:])


@pytest.mark.parametrize("name,integrator", SOURCES[1:])
def test_fused_pass_equals_separate_passes(dev, name, integrator):
    rays = traced(name, integrator)
    wrap = (-math.pi, math.pi)
    for kw in (dict(nmu=33), dict(nmu=76), dict(nmu=33, source_r=20.0, source_phi=1.5707 - 2 * math.pi)):      # (the self-zone reads the wrapped phi)
        sp, want = spec_for(rays, wrap=wrap, **kw)
        fused_words, fused_rays, _ = reduce_on_device(dev, sp, rays, fused=True)
        sep = rays.copy()
        api.range_phi(sep)
        api.redshift(SPIN, -1.0, 0, 0, sep)
        assert sep.tobytes() == fused_rays.tobytes()
        sep_words = reduce_on_device(dev, sp, sep)[0]
        np.testing.assert_array_equal(fused_words[-10:], sep_words[-10:])
        np.testing.assert_array_equal(fused_words[:sp.nmu], sep_words[:sp.nmu])
        assert np.array_equal(fused_words != 0, sep_words != 0) and np.allclose(fused_words, sep_words, rtol=RTOL, atol=0)
        obr.check_observer(api.observer_from_words(sp, fused_words), want, RTOL, (name, kw))
    assert not np.array_equal(sep["redshift"], rays["redshift"])                   # the fused pass did compute g


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_every_record_count(dev, n):
    full = traced("ps_h10", "rk4")
    start = int(np.flatnonzero(obr.per_ray(api.observer_spec(SPIN, gc.r_isco(), R_DISC, R_ESC), full)["escape"])[3])      # an escaping ray leads the slice
    rays = full[start:start + n]
    for nmu in (33, 76):
        sp, _ = spec_for(full, nmu=nmu)
        want = obr.observer(sp, rays)
        assert n == 0 or want["escape"] >= 1
        for fused in (False, True):
            words, after, _ = reduce_on_device(dev, sp, rays, fused=fused)
            obr.check_observer(api.observer_from_words(sp, words), want, RTOL, (n, nmu, fused))
            assert words[-10] == (rays["steps"] > 0).sum() and len(after) == n
            if not fused:
                assert after.tobytes() == rays.tobytes()                             # the reducing form never writes a record


def test_edge_records_land_where_the_rule_puts_them(dev):
    one = obr.synthetic_records([3.0])
    many = np.repeat(one, 130)                                                       # more than two waves of the same record
    for mu0, binned, imu in obr.mu_edge_cases():
        sp = api.observer_spec(0.0, 6.0, 400.0, 900.0, nmu=4, mu0=mu0, dmu=0.25)
        for recs in (one, many):
            for fused in (False, True):
                words = reduce_on_device(dev, sp, recs, fused=fused)[0] if not fused else post_spin0(dev, sp, recs)
                got = api.observer_from_words(sp, words)
                assert (got["escape"], got["binned"], got["outside_mu"]) == (len(recs), len(recs) * binned, len(recs) * (not binned)), (mu0, fused)
                assert list(np.flatnonzero(got["count"])) == ([imu] if binned else []) and got["count"].sum() == len(recs) * binned
    t = np.array([8.0, np.nextafter(8.0, 0.0), np.nextafter(10.0, 0.0), 10.0, np.nan, 9.25])
    odd = obr.synthetic_records(np.full(8, 9.0))
    odd["rdot_sign"][:2] = 0, -1
    odd["k"][2] = np.nan
    odd["emit"][3:6] = np.inf, -1.0, np.nan
    odd["steps"][6] = 0
    whole_nan = np.frombuffer(np.full(70 * capi.RAY_F64.itemsize // 8, np.nan).tobytes(), dtype=capi.RAY_F64).copy()       # every double NaN, the integers NaN's bits
    whole_nan["steps"] = 3
    sp = api.observer_spec(0.0, 6.0, 400.0, 900.0, nmu=2, mu0=0.0, dmu=0.5, gamma=2.0, t0=8.0, dt=0.5, nt=4)
    for recs in (obr.synthetic_records(t), np.tile(obr.synthetic_records(t), 50), odd, np.tile(odd, 40), whole_nan):
        want = obr.observer(sp, recs)
        for fused in (False, True):
            words = reduce_on_device(dev, sp, recs)[0] if not fused else post_spin0(dev, sp, recs)
            obr.check_observer(api.observer_from_words(sp, words), want, RTOL, ("edge", len(recs), fused))
    assert obr.observer(sp, whole_nan)["other"] == 70 and obr.observer(sp, obr.synthetic_records(t))["outside_time"] == 3


def post_spin0(dev, sp, recs):
    L, nw = dev.lib, api.observer_words(sp)
    d_rays, d_out = dev.upload(np.ascontiguousarray(recs)), dev.zeros(nw * 8)
    capi.check(L, L.kr_post_observer_dev_f64(0.0, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(sp), d_rays, len(recs), d_out, None), "kr_post_observer")
    return dev.fetch(d_out, nw)


def test_api_source_to_observer_end_to_end(krlib):
    p = trace_params(capi.RK4)
    src = gc.cases()["ps_h10"]["source"]
    blob, hp = sv.spec_of("blob"), healpix_source()
    for source, name in ((blob, "blob"), (hp, "healpix"), (src, "ps_h10")):
        probe = api.source_to_observer(source, p, api.observer_spec(SPIN, gc.r_isco(), R_DISC, R_ESC), return_records=True)
        sp, want = spec_for(probe["records"], nmu=10, nt=32)                         # (the final records: wrapped already, so no wrap for the rule)
        res = api.source_to_observer(source, p, sp, return_records=True)
        assert res["records"].tobytes() == probe["records"].tobytes()
        obr.check_observer(res, want, RTOL, name)
        assert res["stats"]["rays_traced"] > 0 and res["ray_count"] == (res["records"]["steps"] > 0).sum()
        assert res["records"]["redshift"].any()
        np.testing.assert_array_equal(api.reduce_observer(sp, res["records"])["count"], res["count"])
    # the lamp post (the last of the loop): R_f, the flux and the arrival of the direct continuum
    assert api.reflection_fraction(res) == res["return"] / res["escape"] and 1.0 < api.reflection_fraction(res) < 2.0
    flux = api.observer_flux(res)
    assert flux.shape == (10,) and np.all(np.isfinite(flux)) and flux[res["count"] > 0].min() > 0
    d = api.direct_arrival(res, 30.0)
    i = d["bin"]
    assert i == int((math.cos(math.radians(30.0)) - sp.mu0) / sp.dmu) and res["count"][i] > 0
    m = want["rays"]["imu"] == i
    t_rule = float((want["rays"]["w"][m] * want["rays"]["t_ref"][m]).sum() / want["rays"]["w"][m].sum())
    assert abs(d["t0"] / t_rule - 1) < 1e-12 and 1000.0 < d["t0"] < 1005.0          # 1000 - h cos(30 deg) + the Shapiro delay 2 log(1000 / 10) from h = 10 out
    assert abs(d["shift"] / obr.static_shift(10.0, 1e-3, SPIN) - 1) < 1e-13 and d["flux"] == flux[i]
    np.testing.assert_array_equal(d["hist"], res["hist"][i])
    model = capi.response_model(capi.spectrum_model("table", 0.1, 0.1, 8, r_isco=gc.r_isco(), r_disc=R_DISC, s=np.ones((1, 4)), s_e_min=0.05, s_de=1.5), d["t0"], 1.0, 16)
    assert model.t0 == d["t0"]
    with pytest.raises(capi.KrError, match="outside"):
        api.direct_arrival(res, 170.0)


@pytest.fixture(scope="module")
def exe():
    apps = os.path.join(ROOT, "raytrace_cpu_amd", "apps")
    subprocess.run(["make", "-s", "-C", apps], check=True)
    return os.path.join(apps, "_build", "kr_source_observer")


def test_program_equals_api(exe, tmp_path, krlib):
    par = os.path.join(ROOT, "tests", "golden", "apps", "source_observer.par")
    out = tmp_path / "observer.dat"
    env = dict(os.environ, KRTRACE_ARITHMETIC="strict")                 # api.source_to_observer below traces with flags = 0
    r = subprocess.run([exe, f"--parfile={par}", f"--outfile={out}"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    src = capi.PointSourceSpec()
    src.pos[0], src.pos[1], src.pos[2], src.pos[3] = 0.0, 10.0, 1e-3, 1.5707
    src.V, src.spin, src.tol, src.E = 0.0, SPIN, 100.0, 1.0
    src.dcosalpha, src.dbeta, src.cosalpha0, src.cosalphamax, src.beta0, src.betamax = 0.05, 0.1, -0.995, 0.995, -math.pi, math.pi
    sp = api.observer_spec(SPIN, krlib.kr_kerr_isco(SPIN, 1), 400.0, 1000.0, nmu=7, mu0=0.013, dmu=0.1371, gamma=2.0, dist=1000.0, t0=1000.3, dt=0.73, nt=16)
    res = api.source_to_observer(src, trace_params(capi.RK4, r_max=1100.0), sp, return_records=True)
    want = obr.observer(sp, res["records"])
    assert obr.edge_margin(want) > EDGE
    obr.check_observer(res, want, RTOL, "program's source")
    text = out.read_text()
    rows = text.splitlines()
    assert len(rows) == 8 and rows[0] == "%20s" % "# R_f" + "%20.8e" % api.reflection_fraction(res) and all(len(row) == (5 + 16) * 20 for row in rows[1:])
    table = np.array([[float(x) for x in row.split()] for row in rows[1:]])
    np.testing.assert_array_equal(table[:, 1], res["count"])
    assert (res["count"] > 0).all() and res["outside_time"] > 0 and res["hist"].any()
    # the atomics add in any order, run to run: the numbers as the API formats them, to within the last printed digit of a sum of a few hundred terms
    mine = np.array([[float(x) for x in row.split()] for row in api.observer_text(res).splitlines()[1:]])
    assert mine.shape == table.shape == (7, 21)
    np.testing.assert_allclose(table, mine, rtol=3e-8, atol=0)
    n = api.pointsource_count(src)[0]
    domega = 0.05 * 0.1
    lines = {line.split(":")[0]: line for line in r.stdout.splitlines() if line.startswith(("Total sky:", "Disc:"))}
    assert set(lines) == {"Total sky", "Disc"}
    assert lines["Total sky"] == "%-11s%-10s (%spi)" % ("Total sky: ", "%g" % (n * domega), "%g" % (n * domega / math.pi))
    assert lines["Disc"] == "%-11s%-10s (%spi)" % ("Disc: ", "%g" % (res["return"] * domega), "%g" % (res["return"] * domega / math.pi))
    assert f"Return {res['return']}, escape {res['escape']}, lost {res['lost']}, other {res['other']} of {res['ray_count']} rays" in r.stdout
