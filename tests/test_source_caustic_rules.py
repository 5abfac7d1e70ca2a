"""CPU: the caustic maps of the source sphere and of a flat source plane (include/kr_trace.h, kr_source_map; raytrace_cpu_amd/csrc/kr_caustic.hip)
without a GPU.
  * tests/source_caustic_rules.py, the numpy restatement of the reference's caustic_sourceplane.cpp and caustic_plane.cpp that
    tests/test_gpu_source_caustic.py judges the device kernels with, is pinned to the compiled reference's own output first: the oracle's ImagePlane
    rays (or the host mirror's ImagePlaneBundles rays), the oracle's trace with theta_max = 0 / to a FlatPlaneDestination, the rules, against
    tests/golden/apps/caustic_sourceplane.fits, caustic_plane.fits and caustic_plane_grid.fits;
  * the new entry point refuses bad arguments before it touches a device; struct size, ABI version;
  * kr_caustic_sourceplane and kr_caustic_plane fail loudly where there is no GPU.

The coordinate bound is derived, not tuned.  PHI_S = atan2(sin phi, cos phi), X_S and Y_S are sums of at most three terms, each term a product of at
most four factors, each factor (a C-library sin / cos / atan2 value, or an exactly rounded product) within 1 ulp of the exact one: a term is off by
at most ~4 ulp of its size, three terms and their additions by < 16 * 2^-52 * scale, with scale = pi for the angle and r_max for the plane (no term
is larger than r <= r_max).  The golden files were written by an optimised build whose sincos() may round differently from math.sin / math.cos."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import source_caustic_rules as sr
from caustic_testlib import COORD_ULPS, FIXTURES, build_bundle_dump, mirror_bundles, spec_of
from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def trace_params(g, kind):
    integrator = capi.RK4 if g["integrator"] == "rk4" else capi.RK45
    p, _ = api.caustic_trace_params_source(spec_of(g), kind, r_lim=g.get("r_lim"), z_s=g.get("z_s"), r_max=g.get("r_max"), integrator=integrator,
                                           rk45_tol=g["rk45_tol"], precision=g["precision"], flags=0, steplim=g["steplim"])
    return p


def reference_maps(case, tmp_path):
    """(g, kind, maps, counts, G, eps, scale) of one fixture: the constructor's rays, the oracle's trace, the rules."""
    name, kind = FIXTURES[case]
    g = sr.plane_geometry(sr.read_par(sr.golden(name + ".par")), kind)
    nx, ny = g["nx"], g["ny"]
    bundles = g["eps_frac"] > 0
    if bundles:
        rays = mirror_bundles(build_bundle_dump(tmp_path), tmp_path, g, g["eps_frac"])
        assert len(rays) == 5 * nx * ny
    else:
        rays = ol.oracle_imageplane(spec_of(g))
        assert len(rays) == nx * ny
    rays, _ = ol.oracle_trace(trace_params(g, kind), rays)
    if kind == "sphere":
        maps, counts, G, _ = sr.grid_maps(rays, nx, ny, "sphere", g["dx"], g["dy"])
        return g, kind, maps, counts, G, min(g["dx"], g["dy"]), math.pi
    if bundles:
        eps_x, eps_y = g["eps_frac"] * g["dx"], g["eps_frac"] * g["dy"]
        maps, counts, G = sr.bundle_maps(rays, nx, ny, eps_x, eps_y, g["incl_rad"], g["phi0"])
        return g, kind, maps, counts, G, min(eps_x, eps_y), g["r_max"]
    maps, counts, G, _ = sr.grid_maps(rays, nx, ny, "plane", g["dx"], g["dy"], g["incl_rad"], g["phi0"])
    return g, kind, maps, counts, G, min(g["dx"], g["dy"]), g["r_max"]


@pytest.mark.parametrize("case", list(FIXTURES))
def test_rules_reproduce_the_reference_maps(case, tmp_path):
    """Demanded: integer planes, NaN and SENTINEL positions and the three header counts equal; THETA_S bit-equal; PHI_S, X_S, Y_S within
    c = 16 * 2^-52 * scale (module docstring); DET_J within caustic_rules.det_bound(c, min eps, G).  Measured when this was written (math.sin / cos / atan2 per
    element): the sphere file bit for bit in all eight planes; both plane files with 1 X_S pixel and 2 Y_S pixels not bit-equal, worst 2.8e-14 of the
    7.1e-12 allowed, and DET_J at most 1e-3 of its bound (bundles: 1485 of 1503 defined pixels bit-equal; grid: 1291 of 1299)."""
    name, kind = FIXTURES[case]
    g, kind, maps, counts, G, eps, scale = reference_maps(case, tmp_path)
    want, hdr = sr.fits_planes(sr.golden(name + ".fits"), kind)
    hit_key, (ku, kv) = sr.HIT[kind], sr.COORDS[kind]
    cards = sr.COUNT_CARDS[kind]
    print(case, counts, {k: int(hdr[k]) for k in cards})
    assert (counts["hit"], counts["captured"], counts["steplim"]) == tuple(int(hdr[k]) for k in cards)
    assert counts["hit"] == int(want[hit_key].sum())
    for k in ("SIGN_J", "ORDER", hit_key, "RDOT_FLIPS", "EQUAT_CROSS"):
        assert sr.bits_equal(maps[k], want[k]).all(), (k, int((~sr.bits_equal(maps[k], want[k])).sum()))
    c = COORD_ULPS * scale
    for k in (ku, kv):
        assert np.array_equal(np.isnan(maps[k]), np.isnan(want[k])), k
        diff = np.nan_to_num(np.abs(maps[k] - want[k]))
        print(k, "pixels not bit-equal", int((~sr.bits_equal(maps[k], want[k])).sum()), "worst |diff|", float(diff.max()), "allowed", c)
        if k == "THETA_S":
            assert sr.bits_equal(maps[k], want[k]).all(), k
        assert (diff <= c).all(), (k, float(diff.max()), c)
    gd, wd = maps["DET_J"], want["DET_J"]
    assert np.array_equal(np.isnan(gd), np.isnan(wd)) and np.array_equal(gd == sr.SENTINEL, wd == sr.SENTINEL)
    defined = ~np.isnan(wd) & (wd != sr.SENTINEL)
    bound = sr.det_bound(c, eps, G)
    ratio = np.abs(gd - wd)[defined] / bound[defined]
    print("DET_J defined", int(defined.sum()), "bit-equal", int(sr.bits_equal(gd, wd)[defined].sum()), "worst |diff| / bound", float(ratio.max()),
          "negative", int((wd[defined] < 0).sum()), "SENTINEL", int((wd == sr.SENTINEL).sum()), "NaN", int(np.isnan(wd).sum()), "largest ORDER", int(want["ORDER"].max()))
    assert (ratio <= 1).all(), float(ratio.max())
    # non-vacuity: every DET_J class is present in the file.  The reference's own caustic_plane_grid.fits holds no SENTINEL pixel (on this plane no
    # pixel with four hit neighbours has a neighbour of another ORDER: every hit is ORDER 0), so that file cannot show the class; the SENTINEL branch
    # of the grid-neighbour rule is the one source_caustic_rules.grid_maps shares between the two kinds, and the sphere file pins it on 80 pixels.
    assert (wd[defined] > 0).any() and (wd[defined] < 0).any() and np.isnan(wd).any()
    if case == "plane-grid":
        assert not (wd == sr.SENTINEL).any() and int(want["ORDER"].max()) == 0
        assert (counts["hit"], int(defined.sum()), int((wd[defined] < 0).sum())) == (1534, 1299, 1208)
    else:
        assert (wd == sr.SENTINEL).any()
    if case == "sphere":
        assert (counts["hit"], counts["captured"]) == (1612, 68)
        assert (int(defined.sum()), int((wd == sr.SENTINEL).sum()), int((wd[defined] < 0).sum())) == (1342, 80, 83)
        assert (want["ORDER"] >= 2).any() and int(want["ORDER"].max()) == 2203
    if case == "plane-bundles":
        assert (counts["hit"], int(defined.sum()), int((wd == sr.SENTINEL).sum()), int((wd[defined] < 0).sum())) == (1534, 1503, 19, 712)


# ---- the entry point without a GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def source_map(kind=1, bundles=0, nx=4, ny=4, eps_x=0.01, eps_y=0.01, trig=(0.5, math.sqrt(0.75), 0.0, 1.0)):
    sm = capi.SourceMap()
    sm.kind, sm.bundles, sm.nx, sm.ny, sm.eps_x, sm.eps_y = kind, bundles, nx, ny, eps_x, eps_y
    sm.sin_incl, sm.cos_incl, sm.sin_phi0, sm.cos_phi0 = trig
    return sm


def test_source_map_struct_and_abi_version(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    assert "static_assert(sizeof(kr_source_map) == 64" in header
    assert C.sizeof(capi.SourceMap) == 64
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()
    assert "#define KR_ABI_VERSION 16" in header
    sm = api.source_map_struct("plane", 3, 5, 0.1, 0.2, True, math.radians(30), 0.25)
    assert (sm.kind, sm.bundles, sm.nx, sm.ny, sm.eps_x, sm.eps_y) == (1, 1, 3, 5, 0.1, 0.2)
    assert (sm.sin_incl, sm.cos_incl, sm.sin_phi0, sm.cos_phi0) == (math.sin(math.radians(30)), math.cos(math.radians(30)), math.sin(0.25), math.cos(0.25))
    assert api.source_caustic_words(sm) == 8 * 15 + 3
    words = np.arange(8 * 15 + 3, dtype=float)
    m = api.source_caustic_from_words(sm, words)
    assert m["x_s"].shape == (3, 5) and m["x_s"][1, 2] == 4 * 15 + 1 * 5 + 2 and (m["hit_count"], m["captured"], m["steplim"]) == (120, 121, 122)


def test_source_trace_params():
    spec = ol.imageplane_spec(500.0, 30.0, -20, 20, 1.0, -20, 20, 1.0, 0.998, phi0=0.25)
    p, geo = api.caustic_trace_params_source(spec, "sphere", integrator=capi.RK4)
    assert (p.stop_kind, p.theta_max, p.r_max, p.spin, p.integrator, geo["r_lim"]) == (capi.STOP_THETA, 0.0, 750.0, -0.998, capi.RK4, 750.0)
    p, geo = api.caustic_trace_params_source(spec, "plane", integrator=capi.RK45, rk45_tol=1e-6)
    assert (p.stop_kind, p.r_max, p.rk45_tol, geo["z_s"], geo["r_max"]) == (capi.STOP_FLATPLANE, 2000.0, 1e-6, 500.0, 2000.0)
    assert list(p.stop_params) == [30.0 * math.pi / 180.0, 0.25, 500.0, 0.0]
    with pytest.raises(capi.KrError):
        api.caustic_trace_params_source(spec, "disc")


def test_source_entry_point_validates_before_touching_a_device(lib):
    """Every KR_EINVAL case returns with a message, also here, where a device call would have said KR_ENODEVICE."""
    fake = C.c_void_p(4096)          # never dereferenced: every call below is refused first
    nan, inf = float("nan"), float("inf")

    def refused(sm, n, text, rays=fake, maps=fake):
        rc = lib.kr_post_caustic_source_dev_f64(C.byref(sm) if sm is not None else None, rays, n, maps, None)
        assert rc == capi.KR_EINVAL, rc
        msg = lib.kr_last_error().decode()
        assert msg.startswith("kr_post_caustic_source: ") and text in msg, msg

    refused(None, 100, "null map")
    for bad in (source_map(nx=0), source_map(ny=0), source_map(nx=-3)):
        refused(bad, 10 ** 6, "nx and ny must be >= 1")
    for bad in (source_map(eps_x=0.0), source_map(eps_y=-1.0), source_map(eps_x=nan), source_map(eps_y=inf)):
        refused(bad, 10 ** 6, "eps_x and eps_y must be positive and finite")
    for kind in (-1, 2, 7):
        refused(source_map(kind=kind), 10 ** 6, "unknown kind")
    refused(source_map(kind=0, bundles=1), 10 ** 6, "no bundle mode")
    for q in range(4):
        for v in (nan, inf):
            trig = [0.5, 0.5, 0.5, 0.5]
            trig[q] = v
            refused(source_map(trig=tuple(trig)), 10 ** 6, "non-finite sine or cosine")
    refused(source_map(bundles=1), 5 * 16 - 1, "n smaller than 5 nx ny")
    refused(source_map(bundles=0), 15, "n smaller than nx ny")
    refused(source_map(kind=0), 15, "n smaller than nx ny")
    refused(source_map(), 16, "null argument", rays=None)
    refused(source_map(), 16, "null argument", maps=None)


def test_valid_source_call_answers_no_device(lib):
    if lib.kr_device_count() > 0:
        pytest.skip("a GPU is visible: the call would run kernels on dummy pointers")
    fake = C.c_void_p(4096)
    for sm, n in ((source_map(kind=0), 16), (source_map(kind=1), 16), (source_map(kind=1, bundles=1), 80), (source_map(kind=0, trig=(float("nan"),) * 4), 99)):
        assert lib.kr_post_caustic_source_dev_f64(C.byref(sm), fake, n, fake, None) == capi.KR_ENODEVICE
        assert b"no HIP device" in lib.kr_last_error()


@pytest.mark.parametrize("app,par", [("kr_caustic_sourceplane", "caustic_sourceplane.par"), ("kr_caustic_plane", "caustic_plane.par"),
                                     ("kr_caustic_plane", "caustic_plane_grid.par")])
def test_source_caustic_programs_fail_loudly_without_gpu(app, par, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raytrace_cpu_amd", "apps")], check=True)
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", app)
    out = tmp_path / "out.fits"
    r = subprocess.run([exe, f"--parfile={sr.golden(par)}", f"--outfile={out}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and not out.exists()
    assert "no HIP device available" in r.stderr
