"""GPU: the device-resident caustic maps of the source sphere and of a flat source plane (raytrace_cpu_amd/csrc/kr_caustic.hip,
include/kr_trace.h kr_source_map, api.caustic_source_map, apps/kr_caustic_sourceplane and apps/kr_caustic_plane) against
  * tests/source_caustic_rules.py -- pinned to the compiled reference by tests/test_source_caustic_rules.py -- applied to hand-made records (the
    gather and the Jacobian at the smallest shapes at which they can go wrong) and to the very records the device traced,
  * the oracle's trace with theta_max = 0 (the theta-limit overload with the equatorial stop switched off),
  * the compiled reference's FITS files (the applications end to end, with the rules of test_gpu_dropin_apps.py::test_caustic_apps_match_cpu_output),
  * the reference's own programs on the host mirror (the path users have today), where they were built."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fits_lite
import oracle_lib as ol
import parity
import source_caustic_rules as sr
from caustic_testlib import COORD_ULPS, FIXTURES, OFF, SHAPES, bundle_identity_mask, same_bits, spec_of, synthetic
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope
from test_gpu_dropin_apps import COUNT_KEYS, NATIVE

pytestmark = pytest.mark.gpu

ROOT = ol.ROOT
INCL, PHI0 = math.radians(30.0), 0.25


@pytest.fixture
def dev(krlib):
    """Device buffers of one test, freed at its end."""
    with DeviceScope(krlib) as scope:
        yield scope


def run_maps(dev, sm, rays, n=None):
    """kr_post_caustic_source_dev_f64 on a host array of records: uploaded, d_maps prefilled with 0xFF (the call must WRITE every word), the records
    read back afterwards (the call must not touch them).  Returns the words."""
    L = dev.lib
    n = len(rays) if n is None else n
    d = dev.alloc(max(rays.nbytes, 144))
    capi.check(L, L.kr_memcpy_h2d(d, ol.ptr(rays), rays.nbytes), "h2d")
    nw = api.source_caustic_words(sm)
    d_maps = dev.alloc(nw * 8)
    capi.check(L, L.kr_memset(d_maps, 0xff, nw * 8), "kr_memset")
    capi.check(L, L.kr_post_caustic_source_dev_f64(C.byref(sm), d, n, d_maps, None), "kr_post_caustic_source")
    words = dev.fetch(d_maps, nw)
    after = dev.fetch(d, len(rays), capi.RAY_F64)
    assert after.tobytes() == rays.tobytes(), "the pass modified the records"
    return words


def judge(kind, bundles, sm, words, rays, c, incl=0.0, phi0=0.0):
    """The device's words against the rules on `rays`: integer planes, NaN / SENTINEL positions and the counts equal, THETA_S bit-equal, the other
    coordinates within c, DET_J within det_bound(c, min eps, G), SIGN_J wherever |det| >= that bound.  For the sphere a pixel one of whose raw phi
    differences lies within c of +-pi (the wrap may go either way) counts as ambiguous too.  Returns (got planes, want planes, facts)."""
    nx, ny = sm.nx, sm.ny
    assert not np.isnan(words[8 * nx * ny:]).any() and not (words.view(np.uint64) == 0xFFFFFFFFFFFFFFFF).any(), "a word was not written"
    m = api.source_caustic_from_words(sm, words)
    got = {k.upper(): m[k] for k in api.SOURCE_CAUSTIC_PLANES[kind]}
    near = None
    if bundles:
        want, counts, G = sr.bundle_maps(rays, nx, ny, sm.eps_x, sm.eps_y, incl, phi0)
    else:
        want, counts, G, near = sr.grid_maps(rays, nx, ny, kind, sm.eps_x, sm.eps_y, incl, phi0)
    got_counts = tuple(m[k] for k in api.SOURCE_CAUSTIC_COUNTS[kind])
    assert got_counts == (counts["hit"], counts["captured"], counts["steplim"]), (got_counts, counts)
    hit_key, (ku, kv) = sr.HIT[kind], sr.COORDS[kind]
    for k in (hit_key, "ORDER", "RDOT_FLIPS", "EQUAT_CROSS"):
        assert sr.bits_equal(got[k], want[k]).all(), (k, int((~sr.bits_equal(got[k], want[k])).sum()))
    worst = {}
    for k in (ku, kv):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        if k == "THETA_S":
            assert sr.bits_equal(got[k], want[k]).all(), k
        diff = np.nan_to_num(np.abs(got[k] - want[k]))
        worst[k] = float(diff.max())
        assert (diff <= c).all(), (k, worst[k], c)
    gd, wd = got["DET_J"], want["DET_J"]
    unsure = np.zeros((nx, ny), bool) if near is None else np.nan_to_num(near, nan=np.inf) <= c
    sure = ~unsure
    assert np.array_equal(np.isnan(gd), np.isnan(wd)) and np.array_equal(gd == sr.SENTINEL, wd == sr.SENTINEL)
    defined = ~np.isnan(wd) & (wd != sr.SENTINEL)
    bound = sr.det_bound(c, min(sm.eps_x, sm.eps_y), G)
    judged = defined & sure
    ratio = (np.abs(gd - wd)[judged] / bound[judged]) if judged.any() else np.zeros(1)
    assert (ratio <= 1).all(), float(ratio.max())
    ambiguous = unsure & defined | (defined & (np.abs(wd) < bound))
    assert np.array_equal(got["SIGN_J"][~ambiguous], want["SIGN_J"][~ambiguous])
    assert np.isin(got["SIGN_J"], (-1.0, 0.0, 1.0)).all()
    facts = {"hits": counts["hit"], "defined": int(defined.sum()), "sentinel": int((wd == sr.SENTINEL).sum()), "ambiguous": int(ambiguous.sum()),
             "worst": worst, "worst_ratio": float(ratio.max()), "bit_equal_det": int(sr.bits_equal(gd, wd)[defined].sum()),
             "smallest_abs_det": float(np.abs(wd[defined]).min()) if defined.any() else None, "largest_bound": float(bound[defined].max()) if defined.any() else None}
    return got, want, facts


# ---- 1. hand-made records -----------------------------------------------------------------------------------------------------------------------
def struct_for(kind, bundles, nx, ny):
    eps = (0.01 * 0.5, 0.01 * 0.25) if bundles else (0.5, 0.25)            # dx = 0.5, dy = 0.25
    return api.source_map_struct(kind, nx, ny, eps[0], eps[1], bundles, INCL, PHI0)


MODES = [("sphere", False), ("plane", False), ("plane", True)]
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind,bundles", MODES, ids=["sphere", "plane-grid", "plane-bundles"])
def test_gather_and_jacobian_on_hand_made_records(dev, kind, bundles, shape):
    nx, ny = shape
    sm = struct_for(kind, bundles, nx, ny)
    rays = synthetic(kind, bundles, nx, ny, seed=nx * 1000 + ny, trailing=37)
    words = run_maps(dev, sm, rays)
    scale = math.pi if kind == "sphere" else float(rays["r"].max())
    got, want, facts = judge(kind, bundles, sm, words, rays, COORD_ULPS * scale, INCL, PHI0)
    print(kind, bundles, shape, facts)
    assert facts["ambiguous"] == 0
    if not bundles and (nx < 3 or ny < 3):
        assert np.isnan(got["DET_J"]).all() and (got["SIGN_J"] == 0).all()
    if nx * ny >= 63 and (bundles or (nx >= 3 and ny >= 3)):
        assert facts["defined"] > 0 and 0 < facts["hits"] < nx * ny
    if nx * ny >= 129 and (bundles or min(nx, ny) >= 5):
        assert facts["sentinel"] > 0
    # trailing records are no pixels: the same words without them, and with n exactly the pixel records
    rpb = 5 if bundles else 1
    assert run_maps(dev, sm, rays[:rpb * nx * ny]).tobytes() == words.tobytes()
    assert run_maps(dev, sm, rays, n=rpb * nx * ny).tobytes() == words.tobytes()


def test_sphere_wrap_winding_and_status_bits(dev):
    """The named edge cases one by one on a 5 x 5 sphere grid whose centre pixel (2, 2) has four escaped neighbours of its ORDER."""
    def base():
        rays = synthetic("sphere", False, 5, 5, seed=0, sprinkle=False)
        rays["steps"], rays["status"], rays["rdot_flips"] = 50, capi.STATUS_RLIM, 1
        g = rays.reshape(5, 5)
        ix, iy = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
        g["phi"] = 0.3 + 0.02 * ix + 0.01 * iy
        return rays, g
    sm = struct_for("sphere", False, 5, 5)
    c = COORD_ULPS * math.pi

    def centre(rays):
        got, want, facts = judge("sphere", False, sm, run_maps(dev, sm, rays), rays, c)
        return got, want, facts

    # a phi_s pair straddling +-pi: east just below pi, west just above -pi (as accumulated angles: pi - 0.01 and pi + 0.01)
    rays, g = base()
    g["phi"][3, 2], g["phi"][1, 2] = math.pi - 0.01, math.pi + 0.01
    got, want, _ = centre(rays)
    assert got["PHI_S"][3, 2] > 3.1 and got["PHI_S"][1, 2] < -3.1 and np.isfinite(got["DET_J"][2, 2])
    dphi_dx = (got["PHI_S"][3, 2] - got["PHI_S"][1, 2] - 2 * math.pi) / (2 * sm.eps_x)
    assert abs(dphi_dx - (-0.02 / (2 * sm.eps_x))) < 1e-12          # wrapped: -0.02 over 2 dx, not (2 pi - 0.02)
    # |phi_acc| of 1e3 pi on every pixel: ORDER 999 or 1000 - 1, phi_s through the library's argument reduction
    rays, g = base()
    g["phi"] += 1000 * math.pi
    got, want, facts = centre(rays)
    assert got["ORDER"][2, 2] == 999 and facts["defined"] == 9
    rays, g = base()
    g["phi"] = -(g["phi"] + 1000 * math.pi)
    got, want, facts = centre(rays)
    assert got["ORDER"][2, 2] == 999 and facts["defined"] == 9
    # a neighbour of another order -> SENTINEL at (2, 2) and at the pixels that have it for a neighbour
    rays, g = base()
    g["phi"][2, 3] += 4 * math.pi
    got, _, _ = centre(rays)
    assert got["DET_J"][2, 2] == sr.SENTINEL and got["SIGN_J"][2, 2] == 0 and got["ORDER"][2, 3] == 3 and got["ORDER"][2, 2] == 0
    # steps <= 0, HORIZON, STEPLIM
    for steps, status, expect in ((0, capi.STATUS_RLIM, (24, 0, 1)), (-3, capi.STATUS_RLIM | capi.STATUS_HORIZON, (24, 1, 1)), (50, capi.STATUS_HORIZON, (24, 1, 0)),
                                  (50, capi.STATUS_RLIM | capi.STATUS_STEPLIM, (25, 0, 1)), (50, capi.STATUS_RLIM | capi.STATUS_HORIZON, (25, 0, 0)),
                                  (50, capi.STATUS_DEST, (24, 0, 0))):
        rays, g = base()
        g["steps"][2, 1], g["status"][2, 1] = steps, status
        words = run_maps(dev, sm, rays)
        m = api.source_caustic_from_words(sm, words)
        assert (m["escaped_count"], m["captured"], m["steplim"]) == expect, (steps, status)
        judge("sphere", False, sm, words, rays, c)
        if expect[0] == 24:
            assert np.isnan(m["theta_s"][2, 1]) and np.isnan(m["phi_s"][2, 1]) and m["order"][2, 1] == -1 and np.isnan(m["det_j"][2, 2]) and m["rdot_flips"][2, 1] == 1


def test_plane_bundle_satellite_rules(dev):
    """One 3 x 2 plane in bundle mode; pixel (1, 1)'s satellites are bent one at a time."""
    sm = struct_for("plane", True, 3, 2)

    def base():
        rays = synthetic("plane", True, 3, 2, seed=0, sprinkle=False)
        rays["steps"], rays["status"], rays["rdot_flips"] = 50, capi.STATUS_DEST, 3
        return rays, rays.reshape(3, 2, 5)
    c = COORD_ULPS * 820.0
    rays, B = base()
    got, _, facts = judge("plane", True, sm, run_maps(dev, sm, rays), rays, c, INCL, PHI0)
    assert facts["defined"] == 6 and (got["ORDER"] == 1).all()                      # rdot_flips / 2
    for member in (1, 2, 3, 4):
        for what, expect in (("flips", sr.SENTINEL), ("far", sr.SENTINEL), ("near", None), ("miss", math.nan), ("unstepped", math.nan)):
            rays, B = base()
            q = B[1, 1, member:member + 1]
            if what == "flips":
                q["rdot_flips"] = 4
            elif what == "far":
                q["phi"] += 1.6
            elif what == "near":
                q["phi"] += 1.5
            elif what == "miss":
                q["status"] = capi.STATUS_RLIM | capi.STATUS_HORIZON
            else:
                q["steps"] = 0
            got, _, facts = judge("plane", True, sm, run_maps(dev, sm, rays), rays, c, INCL, PHI0)
            d = got["DET_J"][1, 1]
            assert (np.isfinite(d) and d != sr.SENTINEL) if expect is None else (np.isnan(d) if expect != expect else d == expect), (member, what, d)
            assert facts["defined"] == (6 if expect is None else 5) and got["HIT_PLANE"].all()


# ---- 2. theta_max = 0 on the device ------------------------------------------------------------------------------------------------------------
def test_trace_with_the_equatorial_stop_switched_off_matches_the_oracle():
    """The theta-limit overload with theta_max = 0 (TraceConsts::theta_lo / theta_hi open): the 41 x 41 plane of caustic_sourceplane.par, 1681 rays
    to r_lim = 1000 or the horizon, strict RK4, against ol.oracle_trace at the bar of test_gpu_parity.py's strict fixed-step cases."""
    g = sr.plane_geometry(sr.read_par(sr.golden("caustic_sourceplane.par")), "sphere")
    spec = spec_of(g)
    init = ol.oracle_imageplane(spec)
    assert len(init) == 1681
    p, _ = api.caustic_trace_params_source(spec, "sphere", r_lim=g["r_lim"], integrator=capi.RK4, precision=g["precision"], flags=0, steplim=g["steplim"])
    assert p.stop_kind == capi.STOP_THETA and p.theta_max == 0.0
    want, _ = ol.oracle_trace(p, init)
    got, st = api.trace(p, init)
    res = parity.compare_rays(got, want, rtol=parity.RAY_RTOL, steps_slack=parity.steps_slack_for(p, 0))
    allowed = parity.allowed_bad_frac_strict(p, res["n_traced"])
    parity.record_margin("test_trace_with_the_equatorial_stop_switched_off_matches_the_oracle", "caustic_sourceplane-rk4-strict", res, allowed)
    print({k: v for k, v in res.items() if k != "bad_index"}, "allowed", allowed)
    assert (want["equatorial_crossings"] > 1).any() and ((want["status"] & capi.STATUS_RLIM) != 0).sum() > 1500      # rays did cross the plane and go on
    assert res["frac_bad"] <= allowed, res


# ---- 3. the map kernels against the restatement on the same records --------------------------------------------------------------------------------
GOLDEN = {case: sr.plane_geometry(sr.read_par(sr.golden(name + ".par")), kind) for case, (name, kind) in FIXTURES.items()}
KIND_OF = {case: kind for case, (_, kind) in FIXTURES.items()}
# off the fixtures the step limit is lowered as in tests/test_gpu_caustic.py (a ray that ends on the limit has steps < 0 and is no hit in either
# implementation); RK45 keeps the reference's own 1e5
OFF_STEPLIM = {capi.RK4: 1000000, capi.RK45: 0}


def geometry(plane, case, integrator):
    """the fixture's own plane, or the 65 x 49 plane caustic_testlib.OFF with the programs' defaults (r_lim = 1.5 dist, z_s = dist, r_max = 4 z_s)"""
    if plane == "golden":
        return dict(GOLDEN[case])
    g = dict(OFF, steplim=OFF_STEPLIM[integrator])
    del g["r_disc"]
    if KIND_OF[case] == "sphere":
        g.update(r_lim=1.5 * g["dist"], eps_frac=0.0)
    else:
        g.update(z_s=g["dist"], r_max=4.0 * g["dist"], incl_rad=g["incl"] * math.pi / 180.0, eps_frac=0.01 if case == "plane-bundles" else 0.0)
    return g


def device_records(dev, g, kind, integrator):
    """device-built, device-traced (strict) records of the plane g -> (d_rays, n, sm, scale)"""
    L, spec = dev.lib, spec_of(g)
    bundles = g["eps_frac"] > 0
    n, nx, ny = api.bundles_count(spec) if bundles else api.imageplane_count(spec)
    assert (nx, ny) == (g["nx"], g["ny"])
    d = dev.alloc(n * 144)
    if bundles:
        capi.check(L, L.kr_bundles_init_emit_dev_f64(C.byref(spec), g["eps_frac"], 0.0, 1, 0, d, n, None), "kr_bundles_init_emit")
    else:
        capi.check(L, L.kr_imageplane_init_dev_f64(C.byref(spec), d, n, None), "kr_imageplane_init")
    p, geo = api.caustic_trace_params_source(spec, kind, r_lim=g.get("r_lim"), z_s=g.get("z_s"), r_max=g.get("r_max"), integrator=integrator, rk45_tol=g["rk45_tol"],
                                             precision=g["precision"], flags=0, steplim=g["steplim"])
    capi.check(L, L.kr_trace_dev_f64(C.byref(p), d, n, None, C.byref(capi.Stats())), "kr_trace_dev")
    eps = (g["eps_frac"] * g["dx"], g["eps_frac"] * g["dy"]) if bundles else (g["dx"], g["dy"])
    sm = api.source_map_struct(kind, nx, ny, eps[0], eps[1], bundles, geo.get("incl_rad", 0.0), g["phi0"])
    return d, n, sm, (math.pi if kind == "sphere" else g["r_max"])


@pytest.mark.parametrize("case", list(FIXTURES))
@pytest.mark.parametrize("integrator", ["rk4", "rk45"])
@pytest.mark.parametrize("plane", ["golden", "off"])
def test_source_map_kernels_match_the_rules_on_the_same_records(dev, plane, integrator, case):
    """kr_post_caustic_source_dev_f64 on device-built, device-traced (strict) records against source_caustic_rules on those very records, with the bar
    of test_gpu_caustic.py::test_map_kernels_match_the_rules_on_the_same_records and c = 1e-12 scale (scale = pi / r_max): integers, NaN / SENTINEL
    positions, counts and THETA_S equal; coordinates within c; DET_J within det_bound; SIGN_J wherever |det| is not below that bound; ambiguous pixels
    (those, and for the sphere a raw phi difference within c of +-pi) at most 0.1 % of the hits, none on the golden RK4 plane."""
    L, kind = dev.lib, KIND_OF[case]
    method = capi.RK4 if integrator == "rk4" else capi.RK45
    g = geometry(plane, case, method)
    d, n, sm, scale = device_records(dev, g, kind, method)
    traced = dev.fetch(d, n, capi.RAY_F64)
    nw = api.source_caustic_words(sm)
    d_maps = dev.alloc(nw * 8)
    capi.check(L, L.kr_memset(d_maps, 0xff, nw * 8), "kr_memset")
    capi.check(L, L.kr_post_caustic_source_dev_f64(C.byref(sm), d, n, d_maps, None), "kr_post_caustic_source")
    words = dev.fetch(d_maps, nw)
    assert dev.fetch(d, n, capi.RAY_F64).tobytes() == traced.tobytes()
    c = 1e-12 * scale
    got, want, facts = judge(kind, bool(sm.bundles), sm, words, traced, c, g.get("incl_rad", 0.0), g["phi0"])
    print(plane, integrator, case, facts)
    hits = facts["hits"]
    assert hits > 0.3 * sm.nx * sm.ny and facts["defined"] > 0.2 * sm.nx * sm.ny
    parity.record_margin("test_source_map_kernels_match_the_rules_on_the_same_records", f"{plane}-{integrator}-{case}",
                         {"n_traced": facts["defined"], "n_bad": facts["ambiguous"], "frac_bad": facts["ambiguous"] / hits, "worst_ok": facts["worst_ratio"]},
                         worst_coordinate_difference=max(facts["worst"].values()), smallest_abs_det=facts["smallest_abs_det"], largest_bound=facts["largest_bound"])
    if plane == "golden" and integrator == "rk4":
        assert facts["ambiguous"] == 0
    assert facts["ambiguous"] <= 1e-3 * hits, (facts["ambiguous"], hits)


# ---- 4. the applications end to end against the reference's files ---------------------------------------------------------------------------------------
APP = {"sphere": "kr_caustic_sourceplane", "plane-bundles": "kr_caustic_plane", "plane-grid": "kr_caustic_plane"}
HIT_LINE = {"sphere": "rays escaped to source sphere", "plane": "rays hit source plane"}


def run_native(case, extra=()):
    exe = os.path.join(NATIVE, APP[case])
    assert os.path.exists(exe), f"{exe} not built (make -C raytrace_cpu_amd/apps)"
    par = sr.golden(FIXTURES[case][0] + ".par")
    with tempfile.TemporaryDirectory() as w:
        out = os.path.join(w, "out.fits")
        r = subprocess.run([exe, f"--parfile={par}", f"--outfile={out}", "--timing", *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "timing: rays" in r.stdout and HIT_LINE[KIND_OF[case]] in r.stdout and "rays captured by BH" in r.stdout
        return fits_lite.read(out), fits_lite.header_cards(out), r.stdout


@pytest.mark.parametrize("case", list(FIXTURES))
def test_native_source_caustic_apps_match_cpu_output(case):
    """kr_caustic_sourceplane / kr_caustic_plane against the compiled reference's FITS files with exactly the rules of test_caustic_apps_match_cpu_output:
    HDU list; header cards identical except count cards; classification planes equal on >= 99 % of the pixels; coordinates 1e-6 on >= 99 %; DET_J 1e-3
    on >= 97 %; a 2 pi wrap allowed on PHI_S.  api.caustic_source_map returns the planes of the app's file, bitwise."""
    name, kind = FIXTURES[case]
    golden = sr.golden(name + ".fits")
    hdus, got_cards, stdout = run_native(case)
    got = {h["name"]: h for h in hdus}
    want = {h["name"]: h for h in fits_lite.read(golden)}
    assert list(got) == list(want) == ["PRIMARY"] + list(sr.PLANES[kind])
    for gc_, wc_ in zip(got_cards, fits_lite.header_cards(golden)):
        diff = [(a, b) for a, b in zip(gc_, wc_) if a != b]
        assert len(gc_) == len(wc_) and all(a[:8] == b[:8] and a[:8].strip() in COUNT_KEYS for a, b in diff), diff[:3]
    for pname in list(want)[1:]:
        gq, w = got[pname]["data"], want[pname]["data"]
        nan_same = np.isnan(gq) == np.isnan(w)
        assert nan_same.mean() >= 0.99, (pname, nan_same.mean())
        ok = ~np.isnan(w) & ~np.isnan(gq)
        if pname in ("SIGN_J", "ORDER", "HIT_PLANE", "ESCAPED", "RDOT_FLIPS", "EQUAT_CROSS"):
            same = gq[ok] == w[ok]
            parity.record_margin("test_native_source_caustic_apps_match_cpu_output", f"{name}-{pname}",
                                 {"n_traced": int(ok.sum()), "n_bad": int((~same).sum()), "frac_bad": float((~same).mean()), "worst_ok": None}, 0.01)
            assert same.mean() >= 0.99, (pname, same.mean())
            continue
        rtol = 1e-3 if pname == "DET_J" else 1e-6
        close = np.isclose(gq[ok], w[ok], rtol=rtol, atol=1e-9)
        if pname == "PHI_S":
            close |= np.isclose(np.abs(gq[ok] - w[ok]), 2 * np.pi, rtol=0, atol=1e-5)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(gq[ok] == w[ok], 0.0, np.abs(gq[ok] - w[ok]) / np.maximum(np.abs(w[ok]), 1e-300))
        need_frac = 0.97 if pname == "DET_J" else 0.99
        parity.record_margin("test_native_source_caustic_apps_match_cpu_output", f"{name}-{pname}",
                             {"n_traced": int(ok.sum()), "n_bad": int((~close).sum()), "frac_bad": float((~close).mean()),
                              "worst_ok": float(rel[close].max()) if close.any() else None}, 1 - need_frac, frac_bit_identical_to_cpu=float((gq[ok] == w[ok]).mean()))
        assert close.mean() >= need_frac, (pname, close.mean())

    # the Python entry point: the same planes as the file
    g = GOLDEN[case]
    res = api.caustic_source_map(spec_of(g), kind, r_lim=g.get("r_lim"), z_s=g.get("z_s"), r_max=g.get("r_max"),
                                 integrator=capi.RK4 if g["integrator"] == "rk4" else capi.RK45, eps_frac=g["eps_frac"], rk45_tol=g["rk45_tol"],
                                 precision=g["precision"], steplim=g["steplim"])
    for k, pname in zip(api.SOURCE_CAUSTIC_PLANES[kind], sr.PLANES[kind]):
        assert res[k].shape == (g["nx"], g["ny"])
        assert sr.bits_equal(res[k], np.asarray(got[pname]["data"], dtype=np.float64).T).all(), pname
    hit_count = res[api.SOURCE_CAUSTIC_COUNTS[kind][0]]
    assert f"{hit_count} {HIT_LINE[kind]}" in stdout and f"{res['captured']} rays captured by BH" in stdout
    hdr = got["PRIMARY"]["header"]
    assert tuple(int(hdr[k]) for k in sr.COUNT_CARDS[kind]) == (hit_count, res["captured"], res["steplim"])


# ---- 5. the same answer as the reference's programs on the host mirror -----------------------------------------------------------------------------
def grid_identity_mask(dev, g, tmp_path):
    """[nx, ny]: True where the device-built ray of the pixel carries the bits of the host mirror's ImagePlane constructor in every field"""
    L, spec = dev.lib, spec_of(g)
    n, nx, ny = api.imageplane_count(spec)
    d = dev.alloc(n * 144)
    capi.check(L, L.kr_imageplane_init_dev_f64(C.byref(spec), d, n, None), "kr_imageplane_init")
    got = dev.fetch(d, n, capi.RAY_F64)
    exe = os.path.join(ROOT, "tests", "cpp", "host_ctor_dump")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), exe])
    out = tmp_path / "ip.bin"
    args = [g["dist"], g["incl"], g["x0"], g["xmax"], g["dx"], g["y0"], g["ymax"], g["dy"], g["spin"], g["phi0"]]
    subprocess.run([exe, "ip", str(out)] + [repr(float(a)) for a in args], check=True, timeout=300)
    raw = out.read_bytes()
    want = np.frombuffer(raw[4:], dtype=capi.RAY_F64, count=int(np.frombuffer(raw[:4], dtype=np.int32)[0]))
    assert len(want) == n == nx * ny and g["precision"] == 100
    same = np.ones(n, bool)
    for f in ("t", "r", "theta", "phi", "pt", "pr", "ptheta", "pphi", "k", "h", "Q", "alpha", "beta", "rdot_sign", "thetadot_sign", "status", "steps"):
        same &= same_bits(got[f], want[f])
    return same.reshape(nx, ny)


@pytest.mark.parametrize("case", list(FIXTURES))
def test_native_source_caustic_apps_match_the_dropin_programs(dev, case, tmp_path):
    """The reference's caustic_sourceplane / caustic_plane built on the host mirror (oracle/_ref/dropin; skipped where they were not built) and the
    native programs, both on the strict arithmetic: the same trace kernel on the same records, so on every pixel whose device-built rays carry the
    mirror's bits the integer planes and the NaN / SENTINEL positions are equal and the float planes within the bounds of the map-kernel test.  The
    other pixels are counted, not judged; they must stay <= 5 %."""
    name, kind = FIXTURES[case]
    exe = os.path.join(ROOT, "oracle", "_ref", "dropin", name.replace("_grid", ""))
    if not os.path.exists(exe):
        pytest.skip(f"{exe} not built (oracle/build_dropin_apps.sh needs the reference sources)")
    g = GOLDEN[case]
    judged = bundle_identity_mask(dev, g, tmp_path)[0] if g["eps_frac"] > 0 else grid_identity_mask(dev, g, tmp_path)
    par = sr.golden(name + ".par")
    with tempfile.TemporaryDirectory() as w:
        out = os.path.join(w, "dropin.fits")
        subprocess.run([exe, f"--parfile={par}", f"--outfile={out}"], check=True, stdout=subprocess.DEVNULL, env=dict(os.environ, KRTRACE_ARITHMETIC="strict"),
                       timeout=600)            # (this build links no cfitsio: the plain environment)
        want, _ = sr.fits_planes(out, kind)
    hdus, _, _ = run_native(case, ["--arithmetic=strict"])
    got = {h["name"]: np.asarray(h["data"], dtype=np.float64).T for h in hdus[1:]}
    print(case, "pixels judged", int(judged.sum()), "of", judged.size)
    assert (~judged).mean() <= 0.05
    hit_key, (ku, kv) = sr.HIT[kind], sr.COORDS[kind]
    if g["eps_frac"] == 0:                      # a grid pixel's DET_J reads its four neighbours: judge it only where they are judged too
        inner = judged.copy()
        inner[1:-1, 1:-1] &= judged[2:, 1:-1] & judged[:-2, 1:-1] & judged[1:-1, 2:] & judged[1:-1, :-2]
    else:
        inner = judged
    for k in (hit_key, "ORDER", "RDOT_FLIPS", "EQUAT_CROSS"):
        assert np.array_equal(got[k][judged], want[k][judged]), k
    c = 1e-12 * (math.pi if kind == "sphere" else g["r_max"])
    for k in (ku, kv):
        assert np.array_equal(np.isnan(got[k])[judged], np.isnan(want[k])[judged]), k
        if k == "THETA_S":
            assert sr.bits_equal(got[k], want[k])[judged].all()
        diff = np.nan_to_num(np.abs(got[k] - want[k]))
        assert (diff[judged] <= c).all(), (k, float(diff[judged].max()))
    gd, wd = got["DET_J"], want["DET_J"]
    assert np.array_equal(np.isnan(gd)[inner], np.isnan(wd)[inner]) and np.array_equal((gd == sr.SENTINEL)[inner], (wd == sr.SENTINEL)[inner])
    defined = inner & ~np.isnan(wd) & (wd != sr.SENTINEL)
    eps = min(g["dx"], g["dy"]) * (g["eps_frac"] if g["eps_frac"] > 0 else 1.0)
    # G of the rules is not in the file: |det| <= 2 G^2 gives G >= sqrt(|det| / 2), a SMALLER bound than the map-kernel test's
    bound = sr.det_bound(c, eps, np.sqrt(np.abs(wd) / 2))
    if kind == "sphere":                        # a raw phi difference within c of +-pi may wrap either way (as in the map-kernel test)
        P = want["PHI_S"]
        near = np.full(P.shape, np.inf)
        with np.errstate(invalid="ignore"):
            near[1:-1, 1:-1] = np.minimum(np.abs(np.abs(P[2:, 1:-1] - P[:-2, 1:-1]) - math.pi), np.abs(np.abs(P[1:-1, 2:] - P[1:-1, :-2]) - math.pi))
        defined &= ~(np.nan_to_num(near, nan=np.inf) <= c)
    ratio = np.abs(gd - wd)[defined] / np.maximum(bound[defined], 1e-300)
    assert (np.abs(gd - wd)[defined] <= bound[defined]).all(), float(ratio.max())
    sure = defined & (np.abs(wd) >= bound)
    assert np.array_equal(got["SIGN_J"][sure], want["SIGN_J"][sure])
    parity.record_margin("test_native_source_caustic_apps_match_the_dropin_programs", case,
                         {"n_traced": int(judged.size), "n_bad": int((~judged).sum()), "frac_bad": float((~judged).mean()),
                          "worst_ok": float(ratio.max()) if defined.any() else None})
