"""CPU: the finite-thickness disc (KR_STOP_THICKDISC) away from the device -- what the C ABI refuses and accepts, the class mirror's
ThickDiscDestination against the probe points that the reference-side subclass answered (tests/golden/thick_disc/ref_thick_dump.cpp), and the numpy
restatement (tests/surface_rules.py) against the records the reference's own integrators left on such a surface.  The last group also pins the
conditions that make the GPU tests on those fixtures meaningful."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import parity
import surface_rules as sr
from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def _trace_rc(lib, p, n=4):
    rays = np.zeros(n, dtype=capi.RAY_F64)
    rc = lib.kr_trace_f64(C.byref(p), rays.ctypes.data_as(C.c_void_p), n, None)
    assert (rays["r"] == 0).all()
    return rc, lib.kr_last_error().decode()


def _thick(integrator=capi.RK4, **sp):
    p = capi.default_params(0.5)
    p.integrator = integrator
    v = dict(r_in=4.233, r_out=400.0, slope=0.05, scale=1.0)
    v.update(sp)
    return api.thick_disc_params(p, v["r_in"], v["r_out"], v["slope"], v["scale"])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
REFUSALS = [(dict(r_in=0.0), "r_in"), (dict(r_in=-1.0), "r_in"), (dict(r_in=NAN), "r_in"), (dict(r_in=INF), "r_in"), (dict(r_out=NAN), "r_out"),
            (dict(r_out=INF), "r_out"), (dict(slope=-0.1), "slope"), (dict(slope=NAN), "slope"), (dict(slope=INF), "slope"), (dict(scale=-1.0), "scale"),
            (dict(scale=NAN), "scale"), (dict(scale=INF), "scale")]


@pytest.mark.parametrize("bad,name", REFUSALS, ids=[f"{n}={list(b.values())[0]!r}" for b, n in REFUSALS])
def test_bad_surface_parameter_is_refused_with_its_name(lib, bad, name):
    for integrator in (capi.RK4, capi.RK45):
        rc, msg = _trace_rc(lib, _thick(integrator, **bad))
        assert rc == capi.KR_EINVAL and msg.startswith("kr_trace: KR_STOP_THICKDISC: ") and f" {name} " in msg, msg


def test_good_surface_reaches_the_device_check(lib):
    """On the parent every kind-4 call ended in "unknown stop_kind".  Without a GPU a valid one now gets as far as everything else: KR_ENODEVICE."""
    if lib.kr_device_count() > 0:
        pytest.skip("a GPU is visible: the call would trace")
    for integrator in (capi.RK4, capi.RK45):
        for sp in (dict(), dict(r_out=-1.0), dict(r_out=0.0), dict(slope=0.0, scale=0.0)):
            rc, msg = _trace_rc(lib, _thick(integrator, **sp))
            assert rc == capi.KR_ENODEVICE and "no HIP device" in msg, (sp, msg)


def test_good_surface_is_not_an_invalid_argument(lib):
    """The same on any machine, through the entry point that validates and returns before any device work when n = 0 rays are handed over."""
    rays = np.zeros(1, dtype=capi.RAY_F64)
    for p in (_thick(), _thick(capi.RK45, r_out=-1.0)):
        assert capi.STOP_THICKDISC == 4 and p.stop_kind == 4 and p.stop_params[0] == 4.233 and p.stop_params[2] == 0.05 and p.stop_params[3] == 1.0
        rc = lib.kr_trace_f64(C.byref(p), rays.ctypes.data_as(C.c_void_p), 0, None)
        assert rc != capi.KR_EINVAL, lib.kr_last_error()


def test_euler_and_unknown_kinds_stay_refused(lib):
    rc, msg = _trace_rc(lib, _thick(capi.EULER))
    assert rc == capi.KR_EINVAL and "Euler does not support RayDestination" in msg
    p = capi.copy_params(_thick(), stop_kind=9)
    rc, msg = _trace_rc(lib, p)
    assert rc == capi.KR_EINVAL and msg == "kr_trace: unknown stop_kind"
    rc, msg = _trace_rc(lib, capi.copy_params(_thick(), stop_kind=5))
    assert rc == capi.KR_EINVAL and msg == "kr_trace: unknown stop_kind"


def test_struct_sizes_unchanged_and_new_symbols_bound(lib):
    """The surface is one more value of stop_kind in the unused fourth slot of stop_params, the reducers four more entry points: no struct grows."""
    assert C.sizeof(capi.Params) == 128 and C.sizeof(capi.Stats) == 136 and C.sizeof(capi.EmisBins) == 56 and C.sizeof(capi.ImageBins) == 104
    assert capi.Params.stop_params.offset == 80 and capi.Params.stop_params.size == 32
    want = {"kr_reduce_emissivity_surface_dev_f64": 5, "kr_post_emissivity_surface_dev_f64": 9, "kr_reduce_image_surface_dev_f64": 5,
            "kr_post_image_surface_dev_f64": 9}
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    assert "#define KR_STOP_THICKDISC  4" in header
    for name, nargs in want.items():
        assert hasattr(lib, name) and len(capi.PROTOTYPES[name][1]) == nargs, name
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs, name


def test_surface_entry_points_refuse_bad_arguments_before_any_device_work(lib):
    fake = C.c_void_p(4096)
    e = capi.EmisBins(r_min=1.0, dr=1.1, r_isco=1.0, gamma=2.0, spin=0.5, num_primary_rays=1.0, nr=4, logbin=1)
    i = capi.ImageBins(x0=-1.0, y0=-1.0, img_dx=1.0, img_dy=1.0, r_isco=1.0, r_disc=10.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0, img_nx=2, img_ny=2)
    calls = {"kr_reduce_emissivity_surface": lambda b, d, out: lib.kr_reduce_emissivity_surface_dev_f64(b, d, 4, out, None),
             "kr_post_emissivity_surface": lambda b, d, out: lib.kr_post_emissivity_surface_dev_f64(0.5, 0, -math.pi, math.pi, b, d, 4, out, None),
             "kr_reduce_image_surface": lambda b, d, out: lib.kr_reduce_image_surface_dev_f64(b, d, 4, out, None),
             "kr_post_image_surface": lambda b, d, out: lib.kr_post_image_surface_dev_f64(-0.5, 1, -math.pi, math.pi, b, d, 4, out, None)}
    for name, call in calls.items():
        good = C.byref(e if "emissivity" in name else i)
        for args in ((None, fake, fake), (good, None, fake), (good, fake, None)):
            assert call(*args) == capi.KR_EINVAL and lib.kr_last_error().decode() == f"{name}: null argument", name
    if lib.kr_device_count() == 0:
        for name, call in calls.items():
            assert call(C.byref(e if "emissivity" in name else i), fake, fake) == capi.KR_ENODEVICE, name


# ---- the class mirror against the probe points ----------------------------------------------------------------------------------------------
PROBE_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "raytracer/ray_destination.h"
int main()
{
    char w[16][64];
    int lines = 0;
    while (scanf("%63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9],
                 w[10], w[11], w[12], w[13], w[14], w[15]) == 16) {
        double v[11];
        for (int i = 0; i < 11; i++) v[i] = strtod(w[i], nullptr);
        const ThickDiscDestination<double> d(v[0], v[1], v[2], v[3]);
        const RayDestination<double>& base = d;
        int kind = -1;
        double sp[4] = {-1, -1, -1, -1};
        bool dv = true;
        const bool ok = base.describe(kind, sp, dv);
        if (!ok || kind != KR_STOP_THICKDISC || kind != 4 || sp[0] != v[0] || sp[1] != v[1] || sp[2] != v[2] || sp[3] != v[3] || dv) { printf("describe\n"); return 1; }
        if (base.velocity(v[4], v[5], v[6]) != -1) { printf("velocity\n"); return 1; }
        const double rho = v[4] * sin(v[5]);
        printf("%d %d %a %a %a\n", (int) base.reached(v[4], v[5], v[6]), (int) base.reached(v[4], v[5], v[6], v[7]),
               base.step_limit(v[4], v[5], v[6], v[8], v[9], v[10]), d.height(rho), rho);
        lines++;
    }
    return lines > 0 ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def probe_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("thick_probe")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "raytrace_cpu_amd", "host"), "-o", str(exe), str(src)], check=True)
    return str(exe)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name", ["probes_s005_m1", "probes_s01_open"])
def test_host_class_reproduces_the_probe_points_bit_for_bit(probe_program, name):
    """ThickDiscDestination<double> (g++ -ffp-contract=off, through the base-class interface) on every probe point: reached() in both forms,
    step_limit() and height() are the fixture's bits; describe() names kind 4 with the four parameters.  So is the numpy restatement."""
    import gzip
    text = gzip.open(os.path.join(sr.GOLDEN, name + ".txt.gz"), "rt").read()
    r = subprocess.run([probe_program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-200:] + r.stderr[-200:]
    got = [line.split() for line in r.stdout.splitlines()]
    pr = sr.load_probes(name)
    assert len(got) == len(pr["r"]) >= 200
    assert np.array_equal(np.array([int(g[0]) for g in got]), pr["reached3"]) and np.array_equal(np.array([int(g[1]) for g in got]), pr["reached4"])
    for col, key in ((2, "step_limit"), (3, "H"), (4, "rho")):
        assert _same_bits([float.fromhex(g[col]) for g in got], pr[key]).all(), key
    # the fixture holds what the issue asks of it
    assert (pr["rho"] == pr["r_in"]).sum() >= 3 and np.isnan(pr["r"]).any() and np.isnan(pr["theta"]).any() and np.isnan(pr["prev"]).any()
    assert pr["reached3"].sum() >= 20 and (pr["reached3"] == 0).sum() >= 20 and (pr["reached4"] != pr["reached3"]).sum() >= 5
    assert ((pr["step_limit"] < sr.DBL_MAX) & (pr["step_limit"] > capi.MIN_STEP)).sum() >= 10
    # numpy rule == fixture (same C library for sin / cos / sqrt)
    s = [pr[k] for k in ("r_in", "r_out", "slope", "scale")]
    assert np.array_equal(sr.reached(pr["r"], pr["theta"], pr["theta"], *s), pr["reached3"] == 1)
    assert np.array_equal(sr.reached(pr["r"], pr["theta"], pr["prev"], *s), pr["reached4"] == 1)
    assert _same_bits(sr.step_limit(pr["r"], pr["theta"], pr["pr"], pr["ptheta"], *s), pr["step_limit"]).all()
    assert _same_bits(sr.height(pr["rho"], s[0], s[2], s[3]), pr["H"]).all()
    assert _same_bits(api.surface_height(pr["rho"], s[0], s[2], s[3]), pr["H"]).all()


def test_probe_points_sit_on_the_surface_to_the_ulp():
    """The pairs of neighbouring theta between which |z| <= H changes are in the file: same r, theta one ulp apart, opposite answers."""
    pr = sr.load_probes("probes_s005_m1")
    r, th, hit = pr["r"], pr["theta"], pr["reached3"]
    pairs = [(i, i + 1) for i in range(len(r) - 1) if r[i] == r[i + 1] and abs(th[i].view(np.int64) - th[i + 1].view(np.int64)) == 1]
    assert len(pairs) >= 20 and all(hit[i] != hit[j] for i, j in pairs)
    assert any(th[i] < sr.HALF_PI for i, _ in pairs) and any(th[i] > sr.HALF_PI for i, _ in pairs)


# ---- the reference's records on the surface ---------------------------------------------------------------------------------------------------
def test_fixture_rays_are_the_oracle_point_source():
    """The slots the reference traced are the ones the GPU tests start from: the oracle's PointSource + redshift_start, bit for bit."""
    spec = ol.pointsource_spec(sr.SOURCE["pos"], sr.SOURCE["V"], sr.SPIN, sr.SOURCE["dcosalpha"], sr.SOURCE["dbeta"], cosalpha0=sr.SOURCE["cosalpha0"],
                               cosalphamax=sr.SOURCE["cosalphamax"], beta0=sr.SOURCE["beta0"], betamax=sr.SOURCE["betamax"])
    rays = ol.oracle_pointsource(spec)
    ol.oracle().kro_redshift_start_f64(sr.SPIN, 0.0, 0, 0, ol.ptr(rays), len(rays))
    init = sr.load_init()
    assert len(init) == 5168 and (init["steps"] != -1).sum() == 5040
    for f in ("steps", "rdot_sign", "thetadot_sign", "k", "h", "Q", "emit", "alpha", "beta", "t", "r", "theta", "phi"):
        assert _same_bits(rays[f], init[f]).all() if init[f].dtype.kind == "f" else np.array_equal(rays[f], init[f]), f


@pytest.mark.parametrize("name", list(sr.RUNS))
def test_rule_agrees_with_where_the_reference_stopped(name):
    """reached() by the numpy rule is true at the final position of every DEST ray and false at that of every HORIZON and RLIM ray."""
    slope, scale, _ = sr.RUNS[name]
    rec = sr.load_records(name)
    live = rec["steps"] != -1
    s = (sr.r_in(), sr.R_OUT, slope, scale)
    assert s[0] == capi.load().kr_kerr_isco(sr.SPIN, 1)
    dest, other = live & ((rec["status"] & capi.STATUS_DEST) != 0), live & ((rec["status"] & (capi.STATUS_HORIZON | capi.STATUS_RLIM)) != 0)
    assert dest.sum() > 2000 and other.sum() > 1500 and not (dest & other).any()
    body = sr.in_body(rec["r"], rec["theta"], *s)
    if slope == 0 and scale == 0:
        # the thin annulus: |z| <= 0 holds for no ray (z = r cos(theta) is never exactly 0 here): every stop is the equator clause's, a crossing of
        # the plane inside the radial range, which the record shows as a count of crossings and a position within one step of the plane
        assert not body[dest].any() and (rec["equatorial_crossings"][dest] >= 1).all()
        assert sr.in_range(rec["r"][dest] * np.sin(rec["theta"][dest]), s[0], s[1]).all()
    else:
        crossing = dest & ~body
        assert body[dest].sum() >= dest.sum() - crossing.sum() and (rec["equatorial_crossings"][crossing] >= 1).all()
    assert not body[other].any()
    g = rec["redshift"][dest]
    assert np.isfinite(g).all() and (g > 0).all()


def test_fixture_meets_the_conditions_of_the_gpu_tests():
    rec = sr.load_records("rk4_s005_m1")
    dest = (rec["steps"] > 0) & ((rec["status"] & capi.STATUS_DEST) != 0)
    z = rec["r"] * np.cos(rec["theta"])
    assert dest.sum() >= 2000 and (z[dest] > 0).sum() >= 1900
    counts = {n: int(((sr.load_records(n)["status"] & capi.STATUS_DEST) != 0).sum()) for n in sr.RUNS}
    assert counts == {"rk4_s005_m1": 2336, "rk4_s01_m0": 2406, "rk4_thin": 2265, "rk45_s005_m1": 2343}, counts
