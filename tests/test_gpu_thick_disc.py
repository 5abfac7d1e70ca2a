"""GPU: the finite-thickness disc (KR_STOP_THICKDISC) in the trace kernels and the two reducers for rays that landed on a surface
(raytrace_cpu_amd/csrc/kr_surface.hip).

The trace is held to what the REFERENCE's own integrators give for the same surface handed to them as a user-defined RayDestination
(tests/golden/thick_disc/, tests/test_thick_disc_cpu.py ties those files to the numpy rules of tests/surface_rules.py and to the oracle's point
source); first-hit semantics are checked without any fixture, on the device's own per-step rows; the reducers against the numpy rules.
Bars are tests/parity.py's own; nothing here introduces a tolerance."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import parity
import reducer_rules as rr
import surface_rules as sr
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
RTOL = parity.BIN_RTOL
RK4_RUNS = [n for n, (_, _, m) in sr.RUNS.items() if m == capi.RK4]


def steps_total(rays):
    live = rays["steps"] != -1
    return int(np.abs(rays["steps"][live].astype(np.int64)).sum())


_traced = {}


def strict_trace(name):
    """api.trace of fixture run `name` with flags = 0, once per session (read-only), with its stats."""
    if name not in _traced:
        out, st = api.trace(sr.run_params(name, flags=0), sr.load_init())
        out.setflags(write=False)
        _traced[name] = (out, st)
    return _traced[name]


# ---- trace parity with the reference fixtures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RK4_RUNS)
def test_rk4_trace_reproduces_the_reference_on_every_ray(krlib, name):
    """Strict RK4 through api.trace: every ray's integer outcome and step count are the reference's; floats within parity.compare_rays under
    parity.allowed_bad_frac_strict (the bar of test_destination_run_reproduces_every_integer_outcome), redshift(V = -1, projradius = 1) included,
    which is what the reference's redshift(&disc) computed with the subclass's four_velocity."""
    want = sr.load_records(name)
    out, st = strict_trace(name)
    p = sr.run_params(name)
    got = api.redshift(sr.SPIN, -1.0, 0, 1, out.copy())
    res = parity.compare_rays(got, want, rtol=parity.rtol_for(p), steps_slack=parity.steps_slack_for(p), check_redshift=True)
    allowed = parity.allowed_bad_frac_strict(p, res["n_traced"])
    parity.record_margin("test_rk4_trace_reproduces_the_reference_on_every_ray", f"{name}-strict", res, allowed, steps_total=st["steps_total"],
                         dest=int(((got["status"] & capi.STATUS_DEST) != 0).sum()))
    print(f"thick disc {name}: bad {res['n_bad']} / {res['n_traced']} (allowed {allowed:.4f}), integer fields differ {res['n_int_fields_differ']}, steps differ "
          f"{res['n_steps_differ']}, bit-identical {res['frac_bit_identical']:.4f}, worst accepted {res['worst_ok']:.3e}, steps {st['steps_total']}")
    assert res["n_traced"] == 5040
    assert res["n_int_fields_differ"] == 0 and res["n_steps_differ"] == 0, res
    assert res["frac_bad"] <= allowed, res
    assert st["steps_total"] == steps_total(out) and st["rays_traced"] == 5040


def test_rk45_trace_reproduces_the_reference(krlib):
    """Strict RK45 on the surface (0.05, 1): the per-ray bar of the rk45 golden cases (rtol 1e-7, +-2 steps) with the chaotic-ray allowance alone --
    1 %, no noise envelope added: the oracle that measures one does not know this surface.  The kernel's counters agree with its records."""
    name = "rk45_s005_m1"
    want = sr.load_records(name)
    p = sr.run_params(name)
    out, st = api.trace(p, sr.load_init())
    got = api.redshift(sr.SPIN, -1.0, 0, 1, out.copy())
    res = parity.compare_rays(got, want, rtol=parity.rtol_for(p), steps_slack=parity.steps_slack_for(p), check_redshift=True)
    allowed = parity.allowed_bad_frac(p, None, parity.rtol_for(p), envelope=0.0)
    parity.record_margin("test_rk45_trace_reproduces_the_reference", f"{name}-strict", res, allowed, 0.0, steps_total=st["steps_total"],
                         rk45_stationary_steps=st["rk45_stationary_steps"], rk45_extrapolated_steps=st["rk45_extrapolated_steps"])
    print(f"thick disc {name}: bad {res['n_bad']} / {res['n_traced']} (allowed {allowed:.4f}), terminal status differs {res['frac_terminal_status_differs']:.5f}, "
          f"worst accepted {res['worst_ok']:.3e}, steps {st['steps_total']}, replayed {st['rk45_stationary_steps']}, extrapolated {st['rk45_extrapolated_steps']}")
    assert res["n_traced"] == 5040 and allowed == parity.CHAOTIC_FRAC
    assert res["frac_bad"] <= allowed, res
    assert st["steps_total"] == steps_total(out)
    # the shortcuts for captured rays stay on for this kind (they creep inside r_in, where reached() is false for every theta) and change no outcome
    slow, st_slow = api.trace(capi.copy_params(p, flags=capi.FLAG_RK45_ITERATE_ALL), sr.load_init())
    assert st["rk45_extrapolated_steps"] + st["rk45_stationary_steps"] > 0 and st_slow["rk45_extrapolated_steps"] == 0
    assert np.array_equal(out["steps"], slow["steps"]) and np.array_equal(out["status"], slow["status"])
    for f in ("r", "theta"):
        assert np.array_equal(out[f].view(np.uint64), slow[f].view(np.uint64)), f


MIRROR_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "raytracer/pointsource.h"
#include "raytracer/ray_destination.h"
int main(int argc, char** argv)
{
    const double slope = atof(argv[1]), scale = atof(argv[2]);
    const bool rk45 = atoi(argv[3]) == 2;
    double pos[4] = {0, 5, 1E-3, 0};
    PointSource<double> src(pos, 0, 0.5, TOL, 0.0285, 0.0873, -0.995, 0.995, -1 * M_PI, M_PI);
    src.redshift_start();
    ThickDiscDestination<double> disc(kerr_isco<double>(0.5, +1), 400, slope, scale);
    src.run_raytrace(&disc, rk45 ? Integrator::RK45 : Integrator::RK4, 1000, 0);
    src.redshift(&disc);
    FILE* f = fopen(argv[4], "w");
    for (int i = 0; i < src.get_count(); i++) {
        const Ray<double>& q = src.rays[i];
        fprintf(f, "%d %d %d %d %d %d %a %a %a %a %a %a %a %a %a\n", q.steps, q.status, q.rdot_sign, q.thetadot_sign, q.rdot_flips, q.equatorial_crossings,
                q.t, q.r, q.theta, q.phi, q.pt, q.pr, q.ptheta, q.pphi, q.redshift);
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def mirror_program(tmp_path_factory):
    host, csrc = os.path.join(ROOT, "raytrace_cpu_amd", "host"), os.path.join(ROOT, "raytrace_cpu_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", host])
    d = tmp_path_factory.mktemp("thick_mirror")
    src, exe = d / "mirror.cpp", d / "mirror"
    src.write_text(MIRROR_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-Wno-unused-parameter", "-I" + host, "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src),
                    "-L" + host, "-lkr_host", "-L" + csrc, "-lkrtrace", "-Wl,-rpath," + host, "-Wl,-rpath," + csrc], check=True)
    return str(exe), d


@pytest.mark.parametrize("name", RK4_RUNS)
def test_class_mirror_traces_the_surface(krlib, mirror_program, name):
    """PointSource<double>::run_raytrace(&ThickDiscDestination, RK4) + redshift(&disc) through the host mirror: the records api.trace leaves with
    flags = 0 (the mirror's arithmetic for a destination) and api.redshift(V = -1, projradius = 1), bit for bit -- so the reference's, to the same bar."""
    exe, d = mirror_program
    slope, scale, integrator = sr.RUNS[name]
    path = d / f"{name}.txt"
    r = subprocess.run([exe, repr(slope), repr(scale), str(integrator), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-300:] + r.stderr[-300:]
    cols = list(zip(*[line.split() for line in open(path)]))
    out, _ = strict_trace(name)
    want = api.redshift(sr.SPIN, -1.0, 0, 1, out.copy())
    assert len(cols[0]) == len(want) == 5168
    for f, col in zip(("steps", "status", "rdot_sign", "thetadot_sign", "rdot_flips", "equatorial_crossings"), cols[:6]):
        assert np.array_equal(np.array(col, dtype=np.int64), want[f]), f
    live = want["steps"] != -1
    for f, col in zip(("t", "r", "theta", "phi", "pt", "pr", "ptheta", "pphi", "redshift"), cols[6:]):
        g, w = np.array([float.fromhex(x) for x in col])[live], want[f][live]
        assert ((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))).all(), f


# ---- first-hit semantics, without fixtures ----------------------------------------------------------------------------------------------------
def test_no_recorded_step_before_the_last_is_on_the_surface(krlib):
    """The path recorder on 300 rays of the grid (RK4, write_step = 1): an iteration that ends on reached() writes no row, every other one that
    moved the ray does -- so by the numpy rule no row of any ray satisfies reached(r, theta, phi, previous theta), and the final position of every
    DEST ray does.  The recorded rays end with the records of the flags = 0 trace, bit for bit."""
    name = "rk4_s005_m1"
    slope, scale, _ = sr.RUNS[name]
    s = (sr.r_in(), sr.R_OUT, slope, scale)
    init = sr.load_init()
    live = np.flatnonzero(init["steps"] != -1)
    pick = live[np.linspace(0, len(live) - 1, 300).astype(np.int64)]
    rays = np.ascontiguousarray(init[pick])
    offsets, rows, traced, out, st = api.trace_paths(sr.run_params(name), rays, write_step=1)
    full, _ = strict_trace(name)
    assert traced.all() and parity.same_records(out, full[pick])
    dest = (out["status"] & capi.STATUS_DEST) != 0
    assert dest.sum() >= 100 and (~dest).sum() >= 100
    hits = 0
    for i in range(len(rays)):
        mine = rows[offsets[i]:offsets[i + 1]]
        prev = np.concatenate([[rays["theta"][i]], mine[:-1, 2]])
        hits += int(sr.reached(mine[:, 1], mine[:, 2], prev, *s).sum())
        if dest[i]:
            last_prev = mine[-1, 2] if len(mine) else rays["theta"][i]
            assert sr.reached(out["r"][i], out["theta"][i], last_prev, *s), i
    print(f"thick disc first hit: {int(offsets[-1])} rows of 300 rays, {int(dest.sum())} DEST rays, rows on the surface {hits}")
    assert hits == 0


# ---- hybrid / fast arithmetic -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,mode", [(capi.FLAG_HYBRID, "hybrid"), (capi.FLAG_FAST_MATH, "fastmath")])
def test_other_arithmetic_modes_stop_the_same_rays(krlib, flags, mode):
    """The 5040-ray grid on the surface (0.05, 1), RK4: the hybrid and the fast arithmetic end on the disc exactly the rays the strict one does,
    but for the column whose outcome is decided by rounding in the reference itself (parity.knife_edge_mask)."""
    name = "rk4_s005_m1"
    init = sr.load_init()
    strict, _ = strict_trace(name)
    got, st = api.trace(sr.run_params(name, flags=flags), init)
    keep = (init["steps"] != -1) & ~parity.knife_edge_mask(init, False)
    a, b = (got["status"] & capi.STATUS_DEST) != 0, (strict["status"] & capi.STATUS_DEST) != 0
    differ = keep & (a != b)
    res = parity.compare_rays(parity.drop_rays(got, ~keep), parity.drop_rays(strict, ~keep), rtol=parity.RAY_RTOL, steps_slack=parity.steps_slack_for(sr.run_params(name), flags))
    parity.record_margin("test_other_arithmetic_modes_stop_the_same_rays", f"{name}-{mode}", res, None, dest_differs=int(differ.sum()), rays_strict_side=st["rays_strict_side"])
    print(f"thick disc {mode}: DEST differs on {int(differ.sum())} of {int(keep.sum())} rays ({np.flatnonzero(differ)[:10].tolist()}), beyond 1e-9 of strict {res['n_bad']}")
    assert keep.sum() == 5040 - 70 and b[keep].sum() >= 2000
    assert differ.sum() == 0
    assert st["steps_total"] == steps_total(got)


# ---- the surface reducers ---------------------------------------------------------------------------------------------------------------------
R_ISCO, R_MIN, LIN_DR = 1.0, 1.25, 8.0            # nr = 7 linear bins reach 57.25; 1025 bins of 1 / 16 reach 65.3; the log bins 50


def emis_bins(nr, logbin):
    b = capi.EmisBins()
    b.r_min, b.r_isco, b.gamma, b.spin, b.num_primary_rays = R_MIN, R_ISCO, 1.7, 0.5, 1000.0
    b.dr = math.exp(math.log(50.0 / R_MIN) / nr) if logbin else (LIN_DR if nr == 7 else 2.0 ** -4)
    b.nr, b.logbin = nr, int(logbin)
    return b


def image_bins(nx, ny, flip):
    b = capi.ImageBins()
    b.x0 = b.y0 = -4.0
    b.img_dx = b.img_dy = 1.0
    b.r_isco, b.r_disc = R_ISCO, 40.0
    b.q1, b.rb1, b.q2, b.rb2, b.q3 = 3.0, 4.0, 2.5, 10.0, 3.5
    b.img_nx, b.img_ny, b.flip_image, b.pad = nx, ny, int(flip), 0
    return b


def hand_made():
    """353 records chosen, not traced: rho on every linear bin edge of the nr = 7 histogram and in the band -1 < q <= 0 (theta = pi/2: sin is
    exactly 1 on the device and in numpy, so rho = r and the decision is IEEE-exact), either side of r_isco and r_disc, NaN / zero / negative g,
    records inside the body without the DEST bit, dead slots, landing points above, below and next to the plane, image coordinates on and off
    the pixel grid, and a block of scattered ones.  353 is neither a multiple of 64 nor of 256; the first 37 are used as a set of their own."""
    rng = np.random.default_rng(20251019)
    rows = []
    good = dict(t=10.0, r=6.0, theta=sr.HALF_PI, phi=0.5, k=1.0, h=1.0, Q=5.0, emit=1.0, redshift=0.8, steps=5, status=capi.STATUS_DEST, rdot_sign=-1,
                thetadot_sign=1, alpha=0.5, beta=0.5)
    edges = [R_MIN + LIN_DR * k for k in range(8)]
    for e in edges:
        rows += [dict(r=float(np.nextafter(e, 0.0))), dict(r=e), dict(r=float(np.nextafter(e, np.inf)))]
    rows += [dict(r=v) for v in (1.0, float(np.nextafter(1.0, 0.0)), 1.01, 1.2, 0.5, 40.0, float(np.nextafter(40.0, 0.0)), 45.0)]       # the band, r_isco, r_disc
    rows += [dict(redshift=g) for g in (0.0, -0.0, float("nan"), -1.0, 1e-3, 7.0)]
    rows += [dict(status=0), dict(status=capi.STATUS_RLIM), dict(status=capi.STATUS_HORIZON), dict(status=capi.STATUS_DEST | capi.STATUS_ERGO), dict(steps=0), dict(steps=-1),
             dict(steps=-40)]
    rows += [dict(theta=sr.HALF_PI - d, r=r) for d in (0.3, 0.05, 1e-9, -1e-9, -0.05, -0.3) for r in (2.0, 6.0, 30.0)]                      # z > 0 and z < 0
    rows += [dict(alpha=a, beta=bb) for a in (-4.0, -4.5, -5.0, 3.999, 4.0, 9.0, float("nan")) for bb in (-4.0, 0.999, 1.0)]
    rows += [dict(r=float("nan")), dict(theta=float("nan")), dict(t=float("inf"), r=1.3)]
    out = np.zeros(353, dtype=capi.RAY_F64)
    for i in range(len(out)):
        row = dict(good, **rows[i]) if i < len(rows) else dict(good, r=float(np.exp(rng.uniform(math.log(0.6), math.log(60.0)))), theta=float(rng.uniform(1.0, 2.1)),
                                                             redshift=float(rng.uniform(-0.2, 2.0)), t=float(rng.uniform(-50, 200)), phi=float(rng.uniform(-40, 40)),
                                                             alpha=float(rng.uniform(-5, 10)), beta=float(rng.uniform(-5, 10)), status=int(rng.choice([1, 1, 1, 0, 4, 17])),
                                                             steps=int(rng.choice([-3, 0, 1, 900])), h=float(rng.uniform(-3, 3)), Q=float(rng.uniform(0, 20)))
        for f, v in row.items():
            out[f][i] = v
    assert len(rows) < 353
    out.setflags(write=False)
    return out


def guard(rays, bins):
    """What goes through sin, cos or log may differ in the last bit between device and numpy: no record's log-bin quotient may be within 1e-9 of an
    integer, nor -- where sin(theta) is not exactly 1 -- its linear one, and no rho within 1e-9 of r_isco / r_disc.  Counts are then compared with no slack."""
    with np.errstate(all="ignore"):
        rho = rays["r"] * np.sin(rays["theta"])
        exact = np.sin(rays["theta"]) == 1.0          # (theta within 1e-8 of pi/2: 1 - sin is far below half an ulp, the sine is 1 on either side)
    for b in bins:
        q = rr.emissivity_quotient(b, rho)
        keep = np.isfinite(q) & (~exact if not b.logbin else (rho != b.r_min))
        keep &= np.rint(q) != 0                              # (truncation toward zero: everything in (-1, 1) is index 0, whichever side of 0 it rounds to)
        gap = np.abs(q[keep] - np.rint(q[keep]))
        assert gap.size == 0 or gap.min() > 1e-9, (b.nr, b.logbin, float(gap.min()))
    for edge in (R_ISCO, 40.0):
        gap = np.abs(rho[~exact & np.isfinite(rho)] - edge)
        assert gap.min() > 1e-9


@pytest.fixture
def dev(krlib):
    with DeviceScope(krlib) as scope:
        yield scope


def fetch(dev, d, n, dtype=np.float64):
    capi.check(dev.lib, dev.lib.kr_synchronize(None), "sync")
    return dev.fetch(d, n, dtype)


def hist_dict(b, words):
    raw = api._emissivity_surface_layout(b, words)
    assert np.isfinite(raw["count"]).all() and np.array_equal(np.rint(raw["count"]), raw["count"])
    return api.emissivity_surface_from_words(b, words)


def check_surface_hist(got, want, label):
    for k in ("binned", "upper", "lower"):
        assert got[k] == want[k], (label, k, got[k], want[k])
    return rr.check_reduction(got, want, "count", sr.EMIS_SURFACE_SUMS, RTOL, label)


def margin(test, case, n, worst, **extra):
    parity.record_margin(test, case, {"n_traced": int(n), "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(worst)}, allowed=RTOL,
                         bar="counts and tallies exact; worst_ok = worst |sum - rules| / per-bin sum of absolute terms", **extra)


def record_sets():
    hm = hand_made()
    return {"traced": sr.load_records("rk4_s005_m1"), "hand-made": hm, "hand-made-37": hm[:37]}


EMIS_CASES = [(7, 0), (7, 1), (1025, 0), (1025, 1)]                    # either side of the LDS histogram's capacity (1024), both index rules


@pytest.mark.parametrize("nr,logbin", EMIS_CASES, ids=[f"{'log' if lb else 'lin'}-nr{nr}" for nr, lb in EMIS_CASES])
def test_surface_emissivity_reducer_matches_the_rules(dev, nr, logbin):
    """kr_reduce_emissivity_surface_dev_f64 -- the LDS instance (nr = 7) and the global-atomic one (nr = 1025) -- on the reference's traced records,
    on the hand-made set (353 records) and on its first 37: counts and the four tallies exact, every sum within parity.BIN_RTOL of its bin's sum of
    absolute terms.  The call adds into the caller's buffer: run twice, everything doubles."""
    b = emis_bins(nr, logbin)
    sets = record_sets()
    guard(sets["hand-made"], [b])
    words = api.emissivity_surface_words(b)
    for name, rays in sets.items():
        rays = np.ascontiguousarray(rays)
        want = sr.reduce_emissivity_surface(b, rays)
        d_rays, d_hist = dev.upload(rays), dev.zeros(words * 8)
        capi.check(dev.lib, dev.lib.kr_reduce_emissivity_surface_dev_f64(C.byref(b), d_rays, len(rays), d_hist, None), "kr_reduce_emissivity_surface")
        once = fetch(dev, d_hist, words)
        worst = check_surface_hist(hist_dict(b, once), want, (nr, logbin, name))
        capi.check(dev.lib, dev.lib.kr_reduce_emissivity_surface_dev_f64(C.byref(b), d_rays, len(rays), d_hist, None), "kr_reduce_emissivity_surface")
        twice = fetch(dev, d_hist, words)
        assert np.array_equal(twice[:nr], 2 * once[:nr]) and np.array_equal(twice[6 * nr:], 2 * once[6 * nr:])
        print(f"surface emissivity nr {nr} log {logbin} {name}: on the surface {want['disc_count']}, binned {want['binned']}, upper {want['upper']}, lower {want['lower']}, "
              f"worst sum error {worst:.3g}")
        margin("test_surface_emissivity_reducer_matches_the_rules", f"nr{nr}-log{logbin}-{name}", len(rays), worst, on_surface=want["disc_count"], binned=want["binned"])
        if name == "traced":
            assert want["disc_count"] >= 2000 and want["upper"] >= 1900 and want["binned"] >= 500
        if name == "hand-made":
            assert want["binned"] >= 50 and want["disc_count"] > want["binned"] and want["upper"] >= 10 and want["lower"] >= 10


IMAGE_CASES = [(8, 8, 1), (5, 13, 0)]


@pytest.mark.parametrize("nx,ny,flip", IMAGE_CASES, ids=[f"{nx}x{ny}-flip{f}" for nx, ny, f in IMAGE_CASES])
def test_surface_image_reducer_matches_the_rules(dev, nx, ny, flip):
    """kr_reduce_image_surface_dev_f64 on the hand-made set and its first 37 records (their alpha, beta are image coordinates on and off the grid):
    pixel counts and disc_count exact, every plane within parity.BIN_RTOL; the radius plane holds rho, the emissivity is taken at rho."""
    b = image_bins(nx, ny, flip)
    words = api.image_words(b)
    for name, rays in record_sets().items():
        if name == "traced":
            continue                                          # (a point source's alpha, beta are emission angles, not image coordinates)
        rays = np.ascontiguousarray(rays)
        want = sr.reduce_image_surface(b, rays)
        d_planes = dev.zeros(words * 8)
        capi.check(dev.lib, dev.lib.kr_reduce_image_surface_dev_f64(C.byref(b), dev.upload(rays), len(rays), d_planes, None), "kr_reduce_image_surface")
        got = api.image_planes_from_words(fetch(dev, d_planes, words), nx, ny)
        worst = rr.check_reduction(got, want, "nrays", rr.IMAGE_SUMS, RTOL, (nx, ny, flip, name))
        margin("test_surface_image_reducer_matches_the_rules", f"{nx}x{ny}-flip{flip}-{name}", len(rays), worst, counted=want["disc_count"])
        if name == "hand-made":
            assert want["disc_count"] >= 40 and (want["nrays"] > 0).sum() >= 10
            flat = rr.reduce_image(b, rays)
            assert not np.array_equal(flat["nrays"], want["nrays"])          # the flat reducer sees another set of records


@pytest.mark.parametrize("nr,logbin", [(7, 0), (1025, 1)], ids=["lin-nr7", "log-nr1025"])
def test_fused_surface_emissivity_pass_equals_the_separate_passes(krlib, dev, nr, logbin):
    """kr_post_emissivity_surface_dev_f64 == kr_range_phi_dev_f64 + kr_redshift_dev_f64(V = -1, projradius = 1) + kr_reduce_emissivity_surface_dev_f64:
    records bit for bit, counts and tallies exact, both histograms against the rules on those records."""
    lib = krlib
    b = emis_bins(nr, logbin)
    traced = sr.load_records("rk4_s005_m1").copy()
    traced["phi"] += 40.0                                      # range_phi has work to do
    traced["redshift"] = -7.0                                  # and the redshift is the pass's own
    rays = np.concatenate([traced, hand_made()])
    n, words = len(rays), api.emissivity_surface_words(b)
    d_sep, d_fused = dev.upload(rays), dev.upload(rays)
    h_sep, h_fused = dev.zeros(words * 8), dev.zeros(words * 8)
    capi.check(lib, lib.kr_range_phi_dev_f64(-np.pi, np.pi, d_sep, n, None), "range_phi")
    capi.check(lib, lib.kr_redshift_dev_f64(sr.SPIN, -1.0, 0, 1, 0, d_sep, n, None), "redshift")
    capi.check(lib, lib.kr_reduce_emissivity_surface_dev_f64(C.byref(b), d_sep, n, h_sep, None), "reduce")
    capi.check(lib, lib.kr_post_emissivity_surface_dev_f64(sr.SPIN, 0, -np.pi, np.pi, C.byref(b), d_fused, n, h_fused, None), "post")
    sep, fused = fetch(dev, d_sep, n, capi.RAY_F64), fetch(dev, d_fused, n, capi.RAY_F64)
    assert parity.same_records(sep, fused)
    assert (sep["phi"] != rays["phi"]).sum() > 1000 and (sep["redshift"] > 0).sum() > 2000
    want = sr.reduce_emissivity_surface(b, sep)
    worst = max(check_surface_hist(hist_dict(b, fetch(dev, h, words)), want, (nr, logbin, name)) for name, h in (("separate", h_sep), ("fused", h_fused)))
    assert want["disc_count"] >= 2000
    margin("test_fused_surface_emissivity_pass_equals_the_separate_passes", f"nr{nr}-log{logbin}", n, worst, on_surface=want["disc_count"])


@pytest.mark.parametrize("nx,ny,flip", IMAGE_CASES, ids=[f"{nx}x{ny}-flip{f}" for nx, ny, f in IMAGE_CASES])
def test_fused_surface_image_pass_equals_the_separate_passes(krlib, dev, nx, ny, flip):
    """kr_post_image_surface_dev_f64 == kr_redshift_dev_f64(V = -1, projradius = 1) + kr_range_phi_dev_f64 + kr_reduce_image_surface_dev_f64 on the traced
    point-source records (their angles scaled into image coordinates) and the hand-made set: records bit for bit, both sets of planes against the rules
    on those records.  (tests further down run the pass as an image plane calls it: the stored, negated spin and reverse = 1.)"""
    lib = krlib
    b = image_bins(nx, ny, flip)
    traced = sr.load_records("rk4_s005_m1").copy()
    traced["phi"] += 40.0
    traced["redshift"] = -7.0
    traced["alpha"], traced["beta"] = 8.0 * traced["alpha"], 2.0 * traced["beta"]          # emission angles spread over the pixel grid and beyond it
    rays = np.concatenate([traced, hand_made()])
    n, words = len(rays), api.image_words(b)
    d_sep, d_fused = dev.upload(rays), dev.upload(rays)
    p_sep, p_fused = dev.zeros(words * 8), dev.zeros(words * 8)
    capi.check(lib, lib.kr_redshift_dev_f64(sr.SPIN, -1.0, 0, 1, 0, d_sep, n, None), "redshift")
    capi.check(lib, lib.kr_range_phi_dev_f64(-np.pi, np.pi, d_sep, n, None), "range_phi")
    capi.check(lib, lib.kr_reduce_image_surface_dev_f64(C.byref(b), d_sep, n, p_sep, None), "reduce")
    capi.check(lib, lib.kr_post_image_surface_dev_f64(sr.SPIN, 0, -np.pi, np.pi, C.byref(b), d_fused, n, p_fused, None), "post")
    sep, fused = fetch(dev, d_sep, n, capi.RAY_F64), fetch(dev, d_fused, n, capi.RAY_F64)
    assert parity.same_records(sep, fused)
    assert (sep["phi"] != rays["phi"]).sum() > 1000
    want = sr.reduce_image_surface(b, sep)
    worst = max(rr.check_reduction(api.image_planes_from_words(fetch(dev, d, words), nx, ny), want, "nrays", rr.IMAGE_SUMS, RTOL, (nx, ny, flip, name))
                for name, d in (("separate", p_sep), ("fused", p_fused)))
    assert want["disc_count"] >= 200
    margin("test_fused_surface_image_pass_equals_the_separate_passes", f"{nx}x{ny}-flip{flip}", n, worst, counted=want["disc_count"])


# ---- the image of a thick disc ----------------------------------------------------------------------------------------------------------------
def test_surface_image_of_a_thick_disc(krlib):
    """A 65 x 65 image plane at 75 degrees over a cone of slope 0.2 between the ISCO and r_out = 25 (a = 0.5, RK4), through api.surface_image: the
    seven planes against the numpy rule on the device's own records (which the fused pass leaves as redshift(V = -1, reverse, projradius = 1) +
    range_phi leave them).  The geometry is checked on those records by the surface rule: rays land above the plane, and some end on the outer rim --
    within 0.5 of r_out and deeper than a fifth of the height below the face, where a ray that came through the face (it stops within one step of
    it, RK4's known landing limit) cannot be."""
    spin, r_out, slope = 0.5, 25.0, 0.2
    spec = capi.ImagePlaneSpec()
    spec.dist, spec.inc_deg, spec.x0, spec.xmax, spec.dx, spec.y0, spec.ymax, spec.dy, spec.spin, spec.phi0, spec.precision = 10000.0, 75.0, -30.0, 30.0, 60.0 / 64, -30.0, 30.0, 60.0 / 64, spin, 0.0, 100.0
    n, nx, ny = api.imageplane_count(spec)
    assert (n, nx, ny) == (65 * 65, 65, 65)
    r_in = krlib.kr_kerr_isco(spin, 1)
    p = capi.default_params(-spin)
    p.integrator, p.r_max = capi.RK4, 11000.0
    p = api.thick_disc_params(p, r_in, r_out, slope, 0.0)
    b = capi.ImageBins()
    b.x0, b.y0, b.img_dx, b.img_dy = spec.x0 - spec.dx / 2, spec.y0 - spec.dy / 2, 2 * spec.dx, 2 * spec.dy
    b.r_isco, b.r_disc = r_in, r_out + 1.0
    b.q1, b.rb1, b.q2, b.rb2, b.q3 = 3.0, 4.0, 3.0, 10.0, 3.0
    b.img_nx, b.img_ny, b.flip_image, b.pad = 33, 33, 1, 0
    res = api.surface_image(spec, p, b, return_records=True)
    rec = res["records"]
    want = sr.reduce_image_surface(b, rec)
    worst = rr.check_reduction(res, want, "nrays", rr.IMAGE_SUMS, RTOL, "thick disc image")
    dest = (rec["steps"] > 0) & ((rec["status"] & capi.STATUS_DEST) != 0)
    rho, z = rec["r"] * np.sin(rec["theta"]), rec["r"] * np.cos(rec["theta"])
    H = sr.height(rho, r_in, slope, 0.0)
    assert sr.in_body(rec["r"][dest], rec["theta"][dest], r_in, r_out, slope, 0.0).mean() > 0.99
    upper, rim = dest & (z > 0), dest & (rho > r_out - 0.5) & (np.abs(z) < 0.8 * H)
    print(f"thick disc image: {int(dest.sum())} of {n} rays on the disc, {int(upper.sum())} above the plane, {int(rim.sum())} on the outer rim, counted {want['disc_count']}, "
          f"worst sum error {worst:.3g}, steps {res['stats']['steps_total']}")
    margin("test_surface_image_of_a_thick_disc", "65x65-75deg-slope0.2", n, worst, on_disc=int(dest.sum()), upper=int(upper.sum()), rim=int(rim.sum()))
    assert want["disc_count"] >= 500 and upper.sum() >= 1 and rim.sum() >= 1
    assert (rec["redshift"][dest] > 0).all()


# ---- the programs -----------------------------------------------------------------------------------------------------------------------------
EMISSIVITY_PAR = """# the 5040-ray lamp post of tests/golden/thick_disc on a disc with a surface: 30 logarithmic bins from the ISCO to 400
outfile = unused.dat
source = 0 5 1E-3 0
V = 0
spin = 0.5
dcosalpha = 0.0285
dbeta = 0.0873
r_esc = 400
Nr = 30
logbin_r = 1
integrator = rk4
disc_slope = 0.05
disc_scale = 1
"""


def test_emissivity_program_on_a_thick_disc(krlib, tmp_path):
    """kr_emissivity with disc_slope = 0.05, disc_scale = 1 writes what api.surface_emissivity + api.surface_area give for the same source, trace
    and bins: radii and areas to the digits of the table, counts exactly, the four quotients within parity.BIN_RTOL (two runs add in another order),
    and an eighth column, the mean landing height.  (Without the two keys the same program is held to its golden file by
    tests/test_gpu_dropin_apps.py::test_native_emissivity_app_matches_cpu_output.)"""
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_emissivity")
    assert os.path.exists(exe), "raytrace_cpu_amd/apps is not built"
    par, out = tmp_path / "thick.par", tmp_path / "thick.dat"
    par.write_text(EMISSIVITY_PAR)
    r = subprocess.run([exe, f"--parfile={par}", f"--outfile={out}", "--arithmetic=strict", "--timing"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
    got = np.array([[float(x) for x in line.split()] for line in open(out) if line.strip()])
    assert got.shape == (30, 8)

    spin, nr, r_out = 0.5, 30, 400.0
    r_in = krlib.kr_kerr_isco(spin, 1)
    spec = capi.PointSourceSpec()
    for i, v in enumerate(sr.SOURCE["pos"]):
        spec.pos[i] = v
    spec.V, spec.spin, spec.tol, spec.E = 0.0, spin, 100.0, 1.0
    spec.cosalpha0, spec.cosalphamax, spec.dcosalpha, spec.beta0, spec.betamax, spec.dbeta = -0.995, 0.995, 0.0285, -math.pi, math.pi, 0.0873
    b = capi.EmisBins()
    b.r_min, b.dr, b.r_isco, b.gamma, b.spin, b.nr, b.logbin = r_in, math.exp(math.log(r_out / r_in) / nr), r_in, 2.0, spin, nr, 1
    b.num_primary_rays = float(int(((spec.cosalphamax - spec.cosalpha0) / spec.dcosalpha) * ((spec.betamax - spec.beta0) / spec.dbeta)))
    p = capi.default_params(spin)
    p.integrator, p.r_max, p.flags = capi.RK4, r_out, 0
    res = api.surface_emissivity(spec, api.thick_disc_params(p, r_in, r_out, 0.05, 1.0), b)
    edges = np.array([b.r_min * b.dr ** i for i in range(nr)] + [0.0])
    area = np.array([api.surface_area([edges[i], edges[i] * b.dr], r_in, 0.05, 1.0, spin)[0] for i in range(nr)])
    count = res["count"]
    assert res["disc_count"] >= 2000 and res["upper"] >= 1900 and count.sum() >= 2000
    np.testing.assert_allclose(got[:, 0], edges[:nr], rtol=1e-8)
    np.testing.assert_allclose(got[:, 1], area, rtol=1e-8)
    assert np.array_equal(got[:, 2], count)
    filled = count > 0
    assert filled.sum() >= 15 and (~filled).sum() >= 1 and np.isnan(got[~filled, 5:]).all()          # (5040 rays leave some of the outer bins empty)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = {3: res["flux"] / area, 4: res["emis"] / area, 5: res["sum_redshift"] / count, 6: res["sum_time"] / count, 7: res["sum_z"] / count}
    for col, w in want.items():
        np.testing.assert_allclose(got[filled, col], w[filled], rtol=RTOL, atol=1e-8 * (1 if col == 7 else 0), err_msg=f"column {col}")
    assert (got[filled, 7] > 0).sum() >= 15              # a lamp post on the axis lights the upper face


IMAGE_PAR = """# a 32 x 32 ray grid at 75 degrees over a cone of slope 0.2 out to r_disc = 25 (no pixel at exactly (0, 0))
outfile = unused.fits
dist = 10000
incl = 75
spin = 0.5
r_disc = 25
x0 = -30
xmax = 30
y0 = -30
ymax = 30
Nx = 31
img_Nx = 16
integrator = rk4
disc_slope = 0.2
"""


def test_image_program_on_a_thick_disc(krlib, tmp_path):
    """kr_imageplane_disc_image with disc_slope = 0.2 writes the per-pixel means of what api.surface_image accumulates for the same plane, trace and
    pixels: the six image HDUs (X along FITS axis 1) within parity.BIN_RTOL, NaN in the same pixels, and the same number of rays on the disc."""
    import fits_lite
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_imageplane_disc_image")
    assert os.path.exists(exe), "raytrace_cpu_amd/apps is not built"
    par, out = tmp_path / "thick.par", tmp_path / "thick.fits"
    par.write_text(IMAGE_PAR)
    r = subprocess.run([exe, f"--parfile={par}", f"--outfile={out}", "--arithmetic=strict"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
    hdus = {h["name"]: h["data"] for h in fits_lite.read(str(out))}

    spin, r_disc = 0.5, 25.0
    r_in = krlib.kr_kerr_isco(spin, 1)
    spec = capi.ImagePlaneSpec()
    spec.dist, spec.inc_deg, spec.x0, spec.xmax, spec.dx, spec.y0, spec.ymax, spec.dy, spec.spin, spec.phi0, spec.precision = 10000.0, 75.0, -30.0, 30.0, 60.0 / 31, -30.0, 30.0, 60.0 / 31, spin, 0.0, 100.0
    b = capi.ImageBins()
    b.x0, b.y0, b.img_dx, b.img_dy, b.r_isco, b.r_disc = -30.0, -30.0, 60.0 / 16, 60.0 / 16, r_in, r_disc
    b.q1, b.rb1, b.q2, b.rb2, b.q3, b.img_nx, b.img_ny, b.flip_image, b.pad = 3.0, 4.0, 3.0, 10.0, 3.0, 16, 16, 1, 0
    p = capi.default_params(-spin)
    p.precision, p.integrator, p.theta_max, p.r_max, p.flags = 100.0, capi.RK4, math.pi / 2, 1.1 * 10000.0, 0
    res = api.surface_image(spec, api.thick_disc_params(p, r_in, r_disc, 0.2, 0.0), b)
    assert res["disc_count"] >= 100 and f"{res['disc_count']} rays hit the disc" in r.stdout
    hits = res["nrays"].reshape(16, 16).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = {"FLUX": np.where(hits > 0, res["flux"].reshape(16, 16) / hits, res["flux"].reshape(16, 16))}
        want.update({name: res[k].reshape(16, 16) / hits for name, k in (("RADIUS", "r"), ("PHI", "phi"), ("ENSHIFT", "enshift"), ("TIME", "time"), ("EMIS", "emis"))})
    for name, w in want.items():
        g = hdus[name].T
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), name
        ok = ~np.isnan(w)
        np.testing.assert_allclose(g[ok], w[ok], rtol=RTOL, atol=1e-12, err_msg=name)
    lit = hits > 0
    assert lit.sum() >= 20 and (hdus["RADIUS"].T[lit] >= r_in).all() and (hdus["RADIUS"].T[lit] < r_disc).all()
