"""CPU: the critical-curve maps (include/kr_trace.h, kr_caustic_map; raytrace_cpu_amd/csrc/kr_caustic.hip) without a GPU.
  * tests/caustic_rules.py, the numpy restatement of the reference's caustic_discplane.cpp that tests/test_gpu_caustic.py judges the device kernels
    with, is pinned to the compiled reference's own output first: the host mirror's ImagePlaneBundles rays (or the oracle's ImagePlane rays), the
    oracle's redshift_start / trace / redshift(dest), the rules, against tests/golden/apps/caustic_discplane{,_rk45,_grid}.fits;
  * the new entry points refuse bad arguments before they touch a device; struct size, ray counts, ABI version;
  * kr_caustic_discplane fails loudly where there is no GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import caustic_rules as cr
import oracle_lib as ol
from caustic_testlib import build_bundle_dump, mirror_bundles
from raytrace_cpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_pipeline(g, rays):
    """redshift_start(0, reverse) -> run_raytrace(DiscWithISCODestination, 1.1 dist) -> redshift(dest, reverse) with the oracle
    (caustic_discplane.cpp:215-217).  Returns (rays, r_isco)."""
    lib = ol.oracle()
    spin = g["spin"]
    r_isco = lib.kro_kerr_isco(spin, 1)
    rays = rays.copy()
    lib.kro_redshift_start_f64(-spin, 0.0, 1, 0, ol.ptr(rays), len(rays))
    p = capi.default_params(-spin)
    p.precision = g["precision"]
    p.integrator = capi.RK4 if g["integrator"] == "rk4" else capi.RK45
    p.rk45_tol = g["rk45_tol"]
    p.r_max = 1.1 * g["dist"]
    p.stop_kind = capi.STOP_DISC_ISCO
    for i, v in enumerate((r_isco, g["r_disc"], math.pi / 2, 0.0)):
        p.stop_params[i] = v
    p.steplim = 0
    rays, _ = ol.oracle_trace(p, rays)
    lib.kro_redshift_dest_f64(-spin, 1, ol.ptr(rays), len(rays))
    return rays, r_isco


def within_ulps(g, w, ulps):
    return np.abs(g - w) <= ulps * np.spacing(np.abs(w))


@pytest.mark.parametrize("name,suppressed_on_record", [("caustic_discplane", 241), ("caustic_discplane_rk45", None)])
def test_rules_reproduce_the_reference_bundle_maps(name, suppressed_on_record, tmp_path):
    """Bundle mode, RK4 and RK45.  Measured when this was written (math.sin / cos / atan2 per element): every plane but DET_J bit-equal in all 1681
    pixels under RK4 (1585 hits, 241 suppressed), one Y_DISC pixel 1 ulp off under RK45; DET_J bit-equal in 1566 of 1575 (RK4) defined pixels, the
    rest within 2.4e-13 / 5.1e-14 relative -- the C library's sincos() of the optimised reference build against separate sin / cos, amplified by
    the central difference.  Demanded: integer planes, NaN / SENTINEL positions, RADIUS, REDSHIFT and the hit count equal; PHI, X_DISC, Y_DISC within
    1 ulp; DET_J within 4 (c1 / eps) G with c1 = 2^-52 r_disc (caustic_rules.det_bound)."""
    g = cr.plane_geometry(cr.read_par(cr.golden(name + ".par")))
    want, hdr = cr.fits_planes(cr.golden(name + ".fits"))
    rays = mirror_bundles(build_bundle_dump(tmp_path), tmp_path, g, g["eps_frac"])
    assert len(rays) == 5 * g["nx"] * g["ny"]
    rays, r_isco = oracle_pipeline(g, rays)
    eps_x, eps_y = g["eps_frac"] * g["dx"], g["eps_frac"] * g["dy"]
    maps, counts, G = cr.bundle_maps(rays, g["nx"], g["ny"], r_isco, g["r_disc"], eps_x, eps_y)
    suppressed = cr.suppress(maps)
    print(name, "hits", counts["disc_count"], "suppressed", suppressed, counts)
    assert counts["disc_count"] == int(hdr["DISC_N"]) == int(want["HIT"].sum())
    if suppressed_on_record is not None:
        assert suppressed == suppressed_on_record
    for k in ("SIGN_J", "ORDER", "HIT", "RADIUS", "REDSHIFT"):
        assert cr.bits_equal(maps[k], want[k]).all(), (k, int((~cr.bits_equal(maps[k], want[k])).sum()))
    for k in ("PHI", "X_DISC", "Y_DISC"):
        ok = within_ulps(maps[k], want[k], 1)
        print(k, "pixels not bit-equal", int((~cr.bits_equal(maps[k], want[k])).sum()))
        assert ok.all(), (k, int((~ok).sum()))
    gd, wd = maps["DET_J"], want["DET_J"]
    assert np.array_equal(np.isnan(gd), np.isnan(wd)) and np.array_equal(gd == cr.SENTINEL, wd == cr.SENTINEL)
    defined = ~np.isnan(wd) & (wd != cr.SENTINEL)
    bound = cr.det_bound(2.0 ** -52 * g["r_disc"], min(eps_x, eps_y), G)
    ratio = np.abs(gd - wd)[defined] / bound[defined]
    print("DET_J defined", int(defined.sum()), "bit-equal", int(cr.bits_equal(gd, wd)[defined].sum()), "worst |diff| / bound", float(ratio.max()),
          "smallest |det|", float(np.abs(wd[defined]).min()))
    assert (ratio <= 1).all(), float(ratio.max())
    assert not (np.abs(wd[defined]) < bound[defined]).any()         # so SIGN_J is unambiguous on every pixel of this fixture


def test_rules_reproduce_the_reference_grid_maps():
    """Grid-neighbour mode (bundle_eps_frac = 0, tests/golden/make_caustic_grid_golden.sh) over the oracle's ImagePlane rays: all nine planes bit
    for bit (1585 hits, 6 pixels suppressed).  The grid holds the pixel (0, 0), whose ray has NaN constants and is no hit."""
    g = cr.plane_geometry(cr.read_par(cr.golden("caustic_discplane_grid.par")))
    assert g["eps_frac"] == 0 and g["integrator"] == "rk4"
    want, hdr = cr.fits_planes(cr.golden("caustic_discplane_grid.fits"))
    spec = ol.imageplane_spec(g["dist"], g["incl"], g["x0"], g["xmax"], g["dx"], g["y0"], g["ymax"], g["dy"], g["spin"], phi0=g["phi0"], precision=g["precision"])
    rays = ol.oracle_imageplane(spec)
    assert len(rays) == g["nx"] * g["ny"]
    rays, r_isco = oracle_pipeline(g, rays)
    maps, counts, _ = cr.grid_maps(rays, g["nx"], g["ny"], r_isco, g["r_disc"], g["dx"], g["dy"])
    suppressed = cr.suppress(maps)
    assert counts["disc_count"] == int(hdr["DISC_N"]) == 1585 and suppressed == 6
    for k in cr.PLANES:
        assert cr.bits_equal(maps[k], want[k]).all(), (k, int((~cr.bits_equal(maps[k], want[k])).sum()))


# ---- the entry points without a GPU -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def caustic_map(nx=4, ny=4, eps_x=0.01, eps_y=0.01, bundles=1):
    cm = capi.CausticMap()
    cm.r_isco, cm.r_disc, cm.eps_x, cm.eps_y, cm.nx, cm.ny, cm.bundles = 1.24, 50.0, eps_x, eps_y, nx, ny, bundles
    return cm


def test_caustic_struct_and_abi_version(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    assert "static_assert(sizeof(kr_caustic_map) == 48" in header
    assert C.sizeof(capi.CausticMap) == 48
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()


def test_bundles_count_is_five_times_the_grid(lib):
    grids = [ol.imageplane_spec(500.0, 30.0, -20, 20, 1.0, -20, 20, 1.0, 0.998),
             ol.imageplane_spec(10000.0, 80.0, -30, 30, 60 / 16, -30, 30, 60 / 16, 0.998),
             ol.imageplane_spec(1000.0, 45.0, -10, 10, 0.3, -7, 7, 0.3, 0.9)]      # 67.67 x 47.67 -> 3225 > 67 x 47 = 3149
    exceeds = 0
    for s in grids:
        nx, ny, mx, my = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        n = lib.kr_imageplane_count(C.byref(s), C.byref(nx), C.byref(ny))
        assert lib.kr_bundles_count(C.byref(s), C.byref(mx), C.byref(my)) == 5 * n
        assert (mx.value, my.value) == (nx.value, ny.value)
        assert lib.kr_bundles_count(C.byref(s), None, None) == 5 * n
        exceeds += n > nx.value * ny.value
    assert exceeds >= 1


def test_caustic_entry_points_validate_before_touching_a_device(lib):
    """Every KR_EINVAL case returns with a message, also here, where a device call would have said KR_ENODEVICE."""
    spec = ol.imageplane_spec(500.0, 30.0, -20, 20, 1.0, -20, 20, 1.0, 0.998)
    n = lib.kr_bundles_count(C.byref(spec), None, None)
    fake = C.c_void_p(4096)          # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == capi.KR_EINVAL, rc
        msg = lib.kr_last_error().decode()
        assert text in msg, msg

    for eps in (0.0, -0.01, 0.5, 0.7, float("nan"), float("inf")):
        refused(lib.kr_bundles_init_emit_dev_f64(C.byref(spec), eps, 0.0, 1, 0, fake, n, None), "eps_frac")
    refused(lib.kr_bundles_init_emit_dev_f64(C.byref(spec), 0.01, 0.0, 1, 0, fake, n - 1, None), "n smaller than 5 nx ny")
    refused(lib.kr_bundles_init_emit_dev_f64(None, 0.01, 0.0, 1, 0, fake, n, None), "null spec")
    empty = ol.imageplane_spec(500.0, 30.0, 20, -20, 1.0, -20, 20, 1.0, 0.998)
    refused(lib.kr_bundles_init_emit_dev_f64(C.byref(empty), 0.01, 0.0, 1, 0, fake, n, None), "nx and ny")

    for bad in (caustic_map(nx=0), caustic_map(ny=0), caustic_map(nx=-3)):
        refused(lib.kr_post_caustic_disc_dev_f64(-0.998, 1, C.byref(bad), fake, 10 ** 6, fake, None), "nx and ny")
        refused(lib.kr_caustic_suppress_dev_f64(C.byref(bad), fake, None), "nx and ny")
    for bad in (caustic_map(eps_x=0.0), caustic_map(eps_y=-1.0), caustic_map(eps_x=float("nan")), caustic_map(eps_y=float("inf"))):
        refused(lib.kr_post_caustic_disc_dev_f64(-0.998, 1, C.byref(bad), fake, 10 ** 6, fake, None), "eps_x and eps_y")
        refused(lib.kr_caustic_suppress_dev_f64(C.byref(bad), fake, None), "eps_x and eps_y")
    refused(lib.kr_post_caustic_disc_dev_f64(-0.998, 1, C.byref(caustic_map(bundles=1)), fake, 5 * 16 - 1, fake, None), "n smaller than 5 nx ny")
    refused(lib.kr_post_caustic_disc_dev_f64(-0.998, 1, C.byref(caustic_map(bundles=0)), fake, 15, fake, None), "n smaller than nx ny")
    refused(lib.kr_post_caustic_disc_dev_f64(-0.998, 1, None, fake, 100, fake, None), "null map")
    refused(lib.kr_caustic_suppress_dev_f64(None, fake, None), "null map")


@pytest.mark.parametrize("par", ["caustic_discplane.par", "caustic_discplane_grid.par"])
def test_caustic_program_fails_loudly_without_gpu(par, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raytrace_cpu_amd", "apps")], check=True)
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_caustic_discplane")
    out = tmp_path / "out.fits"
    r = subprocess.run([exe, f"--parfile={cr.golden(par)}", f"--outfile={out}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and not out.exists()
    assert "no HIP device available" in r.stderr or "no ROCm-capable device" in r.stderr
