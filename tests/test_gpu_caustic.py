"""GPU: the device-resident critical-curve maps (raytrace_cpu_amd/csrc/kr_caustic.hip, include/kr_trace.h kr_caustic_map, api.caustic_map,
apps/kr_caustic_discplane) against
  * the host mirror's ImagePlaneBundles constructor and the oracle's redshift_start (the bundle constructor),
  * tests/caustic_rules.py -- pinned to the compiled reference by tests/test_caustic_rules.py -- applied to the very records the device kernels
    read (the map kernels in isolation),
  * the compiled reference's FITS files (the application end to end, with the rules of test_gpu_dropin_apps.py::test_caustic_apps_match_cpu_output),
  * the reference's own program on the host mirror (the path users have today), where it was built."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import caustic_rules as cr
import fits_lite
import oracle_lib as ol
import parity
from raytrace_cpu_amd import api, capi
from test_caustic_rules import build_bundle_dump, mirror_bundles
from test_gpu_dropin_apps import COUNT_KEYS, NATIVE

pytestmark = pytest.mark.gpu

FLOATS = ("t", "r", "theta", "phi", "pt", "pr", "ptheta", "pphi", "k", "h", "Q", "alpha", "beta")
INTS = ("rdot_sign", "thetadot_sign", "status")

# the 41 x 41 plane of tests/golden/apps/caustic_discplane.par, and one away from the fixtures that contains the point (0, 0): 65 x 49 grid points
# (64 x 48 steps of 0.5), inclination 45 degrees, a = 0.9
GOLDEN = cr.plane_geometry(cr.read_par(cr.golden("caustic_discplane.par")))
OFF = dict(dist=500.0, incl=45.0, spin=0.9, r_disc=20.0, x0=-16.0, xmax=16.0, y0=-12.0, ymax=12.0, phi0=0.0, Nx=64, Ny=48, dx=0.5, dy=0.5, nx=65, ny=49,
           eps_frac=0.01, precision=100.0, rk45_tol=1e-8)
PLANES = {"golden": GOLDEN, "off": OFF}
# a photon trapped inside the ISCO is not stopped by a DiscWithISCODestination and runs to the step limit (1e7: 16-38 s of
# one launch).  A ray that ends on the limit has steps < 0 and is no hit in either implementation.
STEPLIM = {"golden": 0, "off": 1000000}


def spec_of(g):
    return ol.imageplane_spec(g["dist"], g["incl"], g["x0"], g["xmax"], g["dx"], g["y0"], g["ymax"], g["dy"], g["spin"], phi0=g["phi0"], precision=g["precision"])


class Dev:
    """device buffers of one test, freed at the end"""

    def __init__(self, L):
        self.L, self.ptrs = L, []

    def alloc(self, nbytes):
        p = C.c_void_p()
        capi.check(self.L, self.L.kr_malloc(C.byref(p), nbytes), "kr_malloc")
        self.ptrs.append(p)
        return p

    def rays(self, d, n):
        out = np.zeros(n, dtype=capi.RAY_F64)
        capi.check(self.L, self.L.kr_memcpy_d2h(ol.ptr(out), d, out.nbytes), "d2h")
        return out

    def doubles(self, d, n):
        out = np.zeros(n)
        capi.check(self.L, self.L.kr_memcpy_d2h(ol.ptr(out), d, out.nbytes), "d2h")
        return out

    def close(self):
        for p in self.ptrs:
            self.L.kr_free(p)


@pytest.fixture
def dev(krlib):
    d = Dev(krlib)
    yield d
    d.close()


def device_bundles(dev, g):
    L, spec = dev.L, spec_of(g)
    n, nx, ny = api.bundles_count(spec)
    assert (nx, ny) == (g["nx"], g["ny"]) and n == 5 * nx * ny
    d = dev.alloc(n * 144)
    capi.check(L, L.kr_bundles_init_emit_dev_f64(C.byref(spec), g["eps_frac"], 0.0, 1, 0, d, n, None), "kr_bundles_init_emit")
    return d, n


def device_grid(dev, g):
    L, spec = dev.L, spec_of(g)
    n, nx, ny = api.imageplane_count(spec)
    assert (nx, ny) == (g["nx"], g["ny"]) and n == nx * ny
    d = dev.alloc(n * 144)
    capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(spec), 0, 1, 0.0, 1, 0, d, n, None), "kr_imageplane_init_emit")
    return d, n


def same_bits(a, b):
    if a.dtype.kind == "f":
        return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def bundle_identity_mask(dev, g, tmp_path):
    """[nx, ny]: True where all five device-built rays of the bundle carry the host mirror's bits in every field (emit against the oracle's
    redshift_start on the mirror's rays).  Also returns (device rays, mirror rays with emit)."""
    d, n = device_bundles(dev, g)
    got = dev.rays(d, n)
    want = mirror_bundles(build_bundle_dump(tmp_path), tmp_path, g, g["eps_frac"])
    assert len(want) == n
    ol.oracle().kro_redshift_start_f64(-g["spin"], 0.0, 1, 0, ol.ptr(want), n)
    same = np.ones(n, bool)
    for f in FLOATS + INTS + ("emit", "steps"):
        same &= same_bits(got[f], want[f])
    return same.reshape(g["nx"], g["ny"], 5).all(axis=2), got, want


# ---- 5. the constructor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", ["golden", "off"])
def test_device_bundle_constructor_carries_the_reference_bits(dev, plane, tmp_path):
    """kr_bundles_init_emit_dev_f64: member 0 of every bundle is the ImagePlane constructor's ray bit for bit (one device function) away from the
    point (0, 0); all members against the host mirror's ImagePlaneBundles with the bar of
    test_gpu_geometry_sweep.py::test_device_imageplane_constructor_carries_the_reference_bits (>= 99 % of the live rays bit-identical in every
    field, no field further off than 1e-13 of its scale); emit against the oracle's redshift_start on the mirror's rays, same bar."""
    g = PLANES[plane]
    mask, got, want = bundle_identity_mask(dev, g, tmp_path)
    n, nx, ny = len(got), g["nx"], g["ny"]
    # member 0 against the ImagePlane constructor
    d_grid, n_grid = device_grid(dev, g)
    grid = dev.rays(d_grid, n_grid)
    centre = got[0::5]
    assert len(centre) == n_grid
    away = ~((centre["alpha"] == 0) & (centre["beta"] == 0))
    assert (~away).sum() == 1                                        # both planes contain the point
    for f in grid.dtype.names:
        assert same_bits(centre[f][away], grid[f][away]).all(), f
    at0 = centre[~away][0]
    assert at0["steps"] == 0 and np.isfinite(at0["h"]) and np.isfinite(at0["Q"]) and at0["h"] == 0      # beta = 0 instead of asin(0 / 0)
    # every member against the mirror
    assert np.array_equal(got["steps"], want["steps"]) and (want["steps"] == 0).all()
    all_same = np.ones(n, bool)
    for f in FLOATS + ("emit",):
        gf, wf = got[f], want[f]
        same = same_bits(gf, wf)
        all_same &= same
        assert same.mean() >= 0.99, (f, same.mean())
        ok = ~np.isnan(wf)
        np.testing.assert_allclose(gf[ok], wf[ok], rtol=1e-13, atol=1e-13 * max(1.0, float(np.nanmax(np.abs(wf)))), err_msg=f)
    for f in INTS:
        assert np.array_equal(got[f], want[f]), f
    parity.record_margin("test_device_bundle_constructor_carries_the_reference_bits", plane,
                         {"n_traced": n, "n_bad": int((~all_same).sum()), "frac_bad": float((~all_same).mean()), "worst_ok": None},
                         frac_bit_identical_every_field=float(all_same.mean()), bundles_bit_identical=float(mask.mean()))
    assert all_same.mean() >= 0.99, all_same.mean()


# ---- 6. the map kernels against the restatement on the same records ----------------------------------------------------------------------------
def caustic_struct(g, r_isco, bundles):
    cm = capi.CausticMap()
    cm.r_isco, cm.r_disc, cm.nx, cm.ny, cm.bundles = r_isco, g["r_disc"], g["nx"], g["ny"], int(bundles)
    cm.eps_x, cm.eps_y = (g["eps_frac"] * g["dx"], g["eps_frac"] * g["dy"]) if bundles else (g["dx"], g["dy"])
    return cm


def planes_of(cm, words):
    m = api.caustic_from_words(cm, words)
    return {k.upper(): m[k] for k in api.CAUSTIC_PLANES}, {k: m[k] for k in api.CAUSTIC_COUNTS}


@pytest.mark.parametrize("mode", ["bundles", "grid"])
@pytest.mark.parametrize("integrator", ["rk4", "rk45"])
@pytest.mark.parametrize("plane", ["golden", "off"])
def test_map_kernels_match_the_rules_on_the_same_records(dev, plane, integrator, mode):
    """kr_post_caustic_disc_dev_f64 + kr_caustic_suppress_dev_f64 on device-built, device-traced (strict) records against caustic_rules on those very
    records with the device's redshift.  HIT, ORDER, NaN / SENTINEL positions and the counts equal; RADIUS, REDSHIFT bitwise; PHI, X_DISC, Y_DISC
    within c = 1e-12 r_disc (a correctly rounded device routine against a <= 1-ulp host one, three calls and a product deep, is below 1e-15 r_disc);
    DET_J within 4 (c / eps) G; SIGN_J wherever |det| is not below that bound -- no such pixel may exist on the golden RK4 plane, at most 0.1 % of the
    hits elsewhere.  The suppression pass is also held, bit for bit, to the rules applied to the device's own maps before it.  rays[].redshift after
    the fused call equals kr_redshift_dest_dev_f64 on a copy."""
    L, g, bundles = dev.L, PLANES[plane], mode == "bundles"
    d, n = device_bundles(dev, g) if bundles else device_grid(dev, g)
    p, r_isco = api.caustic_trace_params(spec_of(g), g["r_disc"], capi.RK4 if integrator == "rk4" else capi.RK45, g["rk45_tol"], g["precision"], 0,
                                         STEPLIM[plane])
    st = capi.Stats()
    capi.check(L, L.kr_trace_dev_f64(C.byref(p), d, n, None, C.byref(st)), "kr_trace_dev")
    traced = dev.rays(d, n)
    d_copy = dev.alloc(n * 144)
    capi.check(L, L.kr_memcpy_h2d(d_copy, ol.ptr(traced), traced.nbytes), "h2d")
    capi.check(L, L.kr_redshift_dest_dev_f64(-g["spin"], 1, d_copy, n, None), "kr_redshift_dest")
    separate = dev.rays(d_copy, n)

    cm = caustic_struct(g, r_isco, bundles)
    nw = api.caustic_words(cm)
    d_maps = dev.alloc(nw * 8)
    capi.check(L, L.kr_memset(d_maps, 0xff, nw * 8), "kr_memset")        # the post call must WRITE every word
    capi.check(L, L.kr_post_caustic_disc_dev_f64(-g["spin"], 1, C.byref(cm), d, n, d_maps, None), "kr_post_caustic_disc")
    before, counts_before = planes_of(cm, dev.doubles(d_maps, nw))
    capi.check(L, L.kr_caustic_suppress_dev_f64(C.byref(cm), d_maps, None), "kr_caustic_suppress")
    after, counts = planes_of(cm, dev.doubles(d_maps, nw))
    fused = dev.rays(d, n)
    for f in fused.dtype.names:                                          # the fused pass leaves the records as the separate one does
        assert same_bits(fused[f], separate[f]).all(), f

    nx, ny = g["nx"], g["ny"]
    if bundles:
        want, want_counts, G = cr.bundle_maps(fused, nx, ny, r_isco, g["r_disc"], cm.eps_x, cm.eps_y)
    else:
        want, want_counts, G = cr.grid_maps(fused, nx, ny, r_isco, g["r_disc"], cm.eps_x, cm.eps_y)
    assert counts_before["suppressed"] == 0
    for k, v in want_counts.items():
        assert counts_before[k] == v == counts[k], (k, counts_before[k], v)
    hits = want_counts["disc_count"]
    assert hits > 0.3 * nx * ny
    for k in ("HIT", "ORDER"):
        assert np.array_equal(before[k], want[k]), k
    for k in ("RADIUS", "REDSHIFT"):
        assert cr.bits_equal(before[k], want[k]).all(), k
    c = 1e-12 * g["r_disc"]
    worst = {}
    for k in ("PHI", "X_DISC", "Y_DISC"):
        diff = np.abs(before[k] - want[k])
        worst[k] = float(diff.max())
        assert (diff <= c).all(), (k, worst[k], c)
    gd, wd = before["DET_J"], want["DET_J"]
    assert np.array_equal(np.isnan(gd), np.isnan(wd)) and np.array_equal(gd == cr.SENTINEL, wd == cr.SENTINEL)
    defined = ~np.isnan(wd) & (wd != cr.SENTINEL)
    assert defined.sum() > 0.2 * nx * ny
    bound = cr.det_bound(c, min(cm.eps_x, cm.eps_y), G)
    ratio = np.abs(gd - wd)[defined] / bound[defined]
    print(plane, integrator, mode, "hits", hits, "defined", int(defined.sum()), "worst coordinate differences", worst, "worst |d det| / bound", float(ratio.max()),
          "DET_J bit-equal", int(cr.bits_equal(gd, wd)[defined].sum()))
    assert (ratio <= 1).all(), float(ratio.max())
    ambiguous = defined & (np.abs(wd) < bound)
    assert np.array_equal(before["SIGN_J"][~ambiguous], want["SIGN_J"][~ambiguous])
    parity.record_margin("test_map_kernels_match_the_rules_on_the_same_records", f"{plane}-{integrator}-{mode}",
                         {"n_traced": int(defined.sum()), "n_bad": int(ambiguous.sum()), "frac_bad": float(ambiguous.sum() / hits), "worst_ok": float(ratio.max())},
                         worst_coordinate_difference=max(worst.values()), smallest_abs_det=float(np.abs(wd[defined]).min()), largest_bound=float(bound[defined].max()))
    if plane == "golden" and integrator == "rk4":
        assert not ambiguous.any()
    assert ambiguous.sum() <= 1e-3 * hits, (int(ambiguous.sum()), hits)

    # the suppression pass on the device's own maps: no tolerance
    expect = {"DET_J": before["DET_J"].copy(), "SIGN_J": before["SIGN_J"].copy()}
    n_supp = cr.suppress(expect)
    assert counts["suppressed"] == n_supp
    assert cr.bits_equal(after["DET_J"], expect["DET_J"]).all() and np.array_equal(after["SIGN_J"], expect["SIGN_J"])
    for k in ("ORDER", "HIT", "RADIUS", "PHI", "X_DISC", "Y_DISC", "REDSHIFT"):
        assert cr.bits_equal(after[k], before[k]).all(), k
    # ... and the whole chain, where no sign is in doubt
    if not ambiguous.any():
        assert cr.suppress(want) == n_supp
        assert np.array_equal(after["SIGN_J"], want["SIGN_J"]) and np.array_equal(after["DET_J"] == cr.SENTINEL, want["DET_J"] == cr.SENTINEL)


# ---- 7. the application end to end against the reference's files ----------------------------------------------------------------------------------
def run_native(par_path, extra=()):
    exe = os.path.join(NATIVE, "kr_caustic_discplane")
    assert os.path.exists(exe), f"{exe} not built (make -C raytrace_cpu_amd/apps)"
    with tempfile.TemporaryDirectory() as w:
        out = os.path.join(w, "out.fits")
        r = subprocess.run([exe, f"--parfile={par_path}", f"--outfile={out}", "--timing", *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "timing: rays" in r.stdout and "rays hit the disc" in r.stdout and "alternating-sign pixels suppressed (branch boundary)" in r.stdout
        return fits_lite.read(out), fits_lite.header_cards(out), r.stdout


@pytest.mark.parametrize("par", ["caustic_discplane", "caustic_discplane_rk45", "caustic_discplane_grid"])
def test_native_caustic_app_matches_cpu_output(par):
    """kr_caustic_discplane against the compiled reference's FITS files with exactly the rules of test_caustic_apps_match_cpu_output: HDU list; header
    cards identical except count cards; classification planes equal on >= 99 % of the pixels; coordinates 1e-6 on >= 99 %; DET_J 1e-3 on >= 97 %; a
    2 pi wrap allowed on PHI.  api.caustic_map returns the planes of the app's file, bitwise."""
    golden = cr.golden(par + ".fits")
    hdus, got_cards, stdout = run_native(cr.golden(par + ".par"))
    got = {h["name"]: h for h in hdus}
    want = {h["name"]: h for h in fits_lite.read(golden)}
    assert list(got) == list(want) == ["PRIMARY"] + list(cr.PLANES)
    for gc_, wc_ in zip(got_cards, fits_lite.header_cards(golden)):
        diff = [(a, b) for a, b in zip(gc_, wc_) if a != b]
        assert len(gc_) == len(wc_) and all(a[:8] == b[:8] and a[:8].strip() in COUNT_KEYS for a, b in diff), diff[:3]
    for name in list(want)[1:]:
        g, w = got[name]["data"], want[name]["data"]
        nan_same = np.isnan(g) == np.isnan(w)
        assert nan_same.mean() >= 0.99, (name, nan_same.mean())
        ok = ~np.isnan(w) & ~np.isnan(g)
        if name in ("SIGN_J", "ORDER", "HIT"):
            same = g[ok] == w[ok]
            parity.record_margin("test_native_caustic_app_matches_cpu_output", f"{par}-{name}",
                                 {"n_traced": int(ok.sum()), "n_bad": int((~same).sum()), "frac_bad": float((~same).mean()), "worst_ok": None}, 0.01)
            assert same.mean() >= 0.99, (name, same.mean())
            continue
        rtol = 1e-3 if name == "DET_J" else 1e-6
        close = np.isclose(g[ok], w[ok], rtol=rtol, atol=1e-9)
        if name == "PHI":
            close |= np.isclose(np.abs(g[ok] - w[ok]), 2 * np.pi, rtol=0, atol=1e-5)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(g[ok] == w[ok], 0.0, np.abs(g[ok] - w[ok]) / np.maximum(np.abs(w[ok]), 1e-300))
        need_frac = 0.97 if name == "DET_J" else 0.99
        parity.record_margin("test_native_caustic_app_matches_cpu_output", f"{par}-{name}",
                             {"n_traced": int(ok.sum()), "n_bad": int((~close).sum()), "frac_bad": float((~close).mean()),
                              "worst_ok": float(rel[close].max()) if close.any() else None}, 1 - need_frac, frac_bit_identical_to_cpu=float((g[ok] == w[ok]).mean()))
        assert close.mean() >= need_frac, (name, close.mean())

    # the Python entry point: the same planes as the file
    geo = cr.plane_geometry(cr.read_par(cr.golden(par + ".par")))
    res = api.caustic_map(spec_of(geo), geo["r_disc"], integrator=capi.RK4 if geo["integrator"] == "rk4" else capi.RK45, eps_frac=geo["eps_frac"],
                          rk45_tol=geo["rk45_tol"], precision=geo["precision"])
    for k, name in zip(api.CAUSTIC_PLANES, cr.PLANES):
        assert res[k].shape == (geo["nx"], geo["ny"])
        assert cr.bits_equal(res[k], np.asarray(got[name]["data"], dtype=np.float64).T).all(), name
    assert f"{res['disc_count']} rays hit the disc" in stdout and f"{res['suppressed']} alternating-sign pixels suppressed" in stdout
    assert int(got["PRIMARY"]["header"]["DISC_N"]) == res["disc_count"]


# ---- 8. the same answer as the reference's program on the host mirror ---------------------------------------------------------------------------
@pytest.mark.parametrize("par", ["caustic_discplane", "caustic_discplane_rk45"])
def test_native_caustic_app_matches_the_dropin_program(dev, par, tmp_path):
    """The reference's caustic_discplane built on the host mirror (oracle/_ref/dropin; skipped where it was not built) and kr_caustic_discplane, both on
    the strict arithmetic: the same trace kernel on the same records, so on every pixel whose five device-built rays carry the mirror's bits the
    classification planes are equal and the float planes within the bounds of the map-kernel test.  The other pixels are counted, not judged."""
    exe = os.path.join(ol.ROOT, "oracle", "_ref", "dropin", "caustic_discplane")
    if not os.path.exists(exe):
        pytest.skip(f"{exe} not built (oracle/build_dropin_apps.sh needs the reference sources)")
    g = cr.plane_geometry(cr.read_par(cr.golden(par + ".par")))
    mask, _, _ = bundle_identity_mask(dev, g, tmp_path)
    with tempfile.TemporaryDirectory() as w:
        out = os.path.join(w, "dropin.fits")
        subprocess.run([exe, f"--parfile={cr.golden(par + '.par')}", f"--outfile={out}"], check=True, stdout=subprocess.DEVNULL,
                       env=dict(os.environ, KRTRACE_ARITHMETIC="strict"), timeout=600)      # (this build links no cfitsio: the plain environment)
        want, _ = cr.fits_planes(out)
    hdus, _, _ = run_native(cr.golden(par + ".par"), ["--arithmetic=strict"])
    got = {h["name"]: np.asarray(h["data"], dtype=np.float64).T for h in hdus[1:]}
    judged = mask
    print(par, "bundles bit-identical (judged)", int(mask.sum()), "of", mask.size)
    assert judged.mean() >= 0.95            # the constructor's bar, >= 99 % of the rays, leaves >= 95 % of the 5-ray bundles
    for k in ("HIT", "ORDER"):
        assert np.array_equal(got[k][judged], want[k][judged]), k
    for k in ("RADIUS", "REDSHIFT"):
        assert cr.bits_equal(got[k], want[k])[judged].all(), k
    c = 1e-12 * g["r_disc"]
    for k in ("PHI", "X_DISC", "Y_DISC"):
        assert (np.abs(got[k] - want[k])[judged] <= c).all(), (k, float(np.abs(got[k] - want[k])[judged].max()))
    gd, wd = got["DET_J"], want["DET_J"]
    assert np.array_equal(np.isnan(gd)[judged], np.isnan(wd)[judged]) and np.array_equal((gd == cr.SENTINEL)[judged], (wd == cr.SENTINEL)[judged])
    defined = judged & ~np.isnan(wd) & (wd != cr.SENTINEL)
    eps = g["eps_frac"] * min(g["dx"], g["dy"])
    # G of the rules is not in the file: |det| <= 2 G^2 gives G >= sqrt(|det| / 2), a SMALLER bound than the map-kernel test's
    bound = cr.det_bound(c, eps, np.sqrt(np.abs(wd) / 2))
    assert (np.abs(gd - wd)[defined] <= bound[defined]).all(), float((np.abs(gd - wd)[defined] / bound[defined]).max())
    assert np.array_equal(got["SIGN_J"][judged], want["SIGN_J"][judged])
    parity.record_margin("test_native_caustic_app_matches_the_dropin_program", par,
                         {"n_traced": int(mask.size), "n_bad": int((~judged).sum()), "frac_bad": float((~judged).mean()),
                          "worst_ok": float((np.abs(gd - wd)[defined] / bound[defined]).max())})
