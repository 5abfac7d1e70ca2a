"""GPU: the device-resident critical-curve maps (raytrace_cpu_amd/csrc/kr_caustic.hip, include/kr_trace.h kr_caustic_map, api.caustic_map,
apps/kr_caustic_discplane) against
  * the host mirror's ImagePlaneBundles constructor and the oracle's redshift_start (the bundle constructor),
  * tests/caustic_rules.py -- pinned to the compiled reference by tests/test_caustic_rules.py -- applied to the very records the device kernels
    read (the map kernels in isolation), and to hand-made records at the smallest shapes at which the gather can go wrong,
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
from caustic_testlib import FLOATS, INTS, OFF, SHAPES, bundle_identity_mask, device_bundles, same_bits, spec_of, synthetic
import fits_lite
import oracle_lib as ol
import parity
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope
from test_gpu_dropin_apps import COUNT_KEYS, NATIVE

pytestmark = pytest.mark.gpu

# the 41 x 41 plane of tests/golden/apps/caustic_discplane.par, and one away from the fixtures that contains the point (0, 0): 65 x 49 grid points
# (64 x 48 steps of 0.5), inclination 45 degrees, a = 0.9
GOLDEN = cr.plane_geometry(cr.read_par(cr.golden("caustic_discplane.par")))
PLANES = {"golden": GOLDEN, "off": OFF}
# a photon trapped inside the ISCO is not stopped by a DiscWithISCODestination and runs to the step limit (1e7: 16-38 s of
# one launch).  A ray that ends on the limit has steps < 0 and is no hit in either implementation.
STEPLIM = {"golden": 0, "off": 1000000}


@pytest.fixture
def dev(krlib):
    """Device buffers of one test, freed at its end."""
    with DeviceScope(krlib) as scope:
        yield scope


def device_grid(dev, g):
    L, spec = dev.lib, spec_of(g)
    n, nx, ny = api.imageplane_count(spec)
    assert (nx, ny) == (g["nx"], g["ny"]) and n == nx * ny
    d = dev.alloc(n * 144)
    capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(spec), 0, 1, 0.0, 1, 0, d, n, None), "kr_imageplane_init_emit")
    return d, n


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
    grid = dev.fetch(d_grid, n_grid, capi.RAY_F64)
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
    L, g, bundles = dev.lib, PLANES[plane], mode == "bundles"
    d, n = device_bundles(dev, g) if bundles else device_grid(dev, g)
    p, r_isco = api.caustic_trace_params(spec_of(g), g["r_disc"], capi.RK4 if integrator == "rk4" else capi.RK45, g["rk45_tol"], g["precision"], 0,
                                         STEPLIM[plane])
    st = capi.Stats()
    capi.check(L, L.kr_trace_dev_f64(C.byref(p), d, n, None, C.byref(st)), "kr_trace_dev")
    traced = dev.fetch(d, n, capi.RAY_F64)
    d_copy = dev.upload(traced)
    capi.check(L, L.kr_redshift_dest_dev_f64(-g["spin"], 1, d_copy, n, None), "kr_redshift_dest")
    separate = dev.fetch(d_copy, n, capi.RAY_F64)

    cm = caustic_struct(g, r_isco, bundles)
    nw = api.caustic_words(cm)
    d_maps = dev.alloc(nw * 8)
    capi.check(L, L.kr_memset(d_maps, 0xff, nw * 8), "kr_memset")        # the post call must WRITE every word
    capi.check(L, L.kr_post_caustic_disc_dev_f64(-g["spin"], 1, C.byref(cm), d, n, d_maps, None), "kr_post_caustic_disc")
    before, counts_before = planes_of(cm, dev.fetch(d_maps, nw))
    capi.check(L, L.kr_caustic_suppress_dev_f64(C.byref(cm), d_maps, None), "kr_caustic_suppress")
    after, counts = planes_of(cm, dev.fetch(d_maps, nw))
    fused = dev.fetch(d, n, capi.RAY_F64)
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


# ---- 6b. the map kernels on hand-made records, at the smallest shapes at which the gather can go wrong ---------------------------------------------
HAND = dict(spin=0.9, r_disc=20.0, dx=0.5, dy=0.25, eps_frac=0.01)


def disc_records(bundles, nx, ny, r_isco, seed, trailing):
    """caustic_testlib.synthetic's pattern (steps <= 0, the status bits, another winding next door, satellites with another rdot_flips / far away in
    phi) as records that end on the disc: r varies smoothly inside [r_isco, r_disc), so determinants exist (of either sign on the long
    planes); theta near the equator, constants of motion and emit for which redshift(dest, reverse) is positive.  Sprinkled on top:
    centre rays with r < r_isco, with r >= r_disc, with emit < 0 (g < 0) and emit = NaN (g = NaN); in bundle mode satellites beyond r_disc (no
    determinant) and pixels whose east and west satellites are swapped (the opposite sign among its neighbours: the suppression pass has work).
    `trailing` records that would be hits follow: they are no pixels, but the pass owes them their redshift."""
    rng = np.random.default_rng(seed + 77)
    rpb = 5 if bundles else 1
    rays = synthetic("plane", bundles, nx, ny, seed).reshape(nx, ny, rpb)
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    da, db = (0.0, 1.0, -1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0, -1.0)
    span = HAND["r_disc"] - r_isco - 2.0
    for m in range(rpb):
        a, b = ix + 0.01 * da[m], iy + 0.01 * db[m]
        q = rays[:, :, m]
        q["r"] = r_isco + 1.0 + span * (0.4 + 0.6 * a / nx - 0.4 * b / ny)
        q["theta"] = math.pi / 2 - 1e-3 * (1 + (ix + iy) % 3)
        q["k"], q["h"], q["Q"] = 1.0, 0.5 + 0.02 * a - 0.01 * b, 4.0 + 0.05 * b
        q["rdot_sign"], q["thetadot_sign"] = np.where((ix + iy) % 2 == 0, 1, -1), np.where(ix % 2 == 0, 1, -1)
        q["emit"] = 0.9 + 0.001 * a
        q["redshift"] = -5.0                                               # overwritten by the pass
    c = rays[:, :, 0]
    pick = rng.random((nx, ny))
    c["r"][pick < 0.04] = 0.5 * r_isco + 0.6
    c["r"][(pick >= 0.04) & (pick < 0.08)] = HAND["r_disc"] + 0.03 * ix[(pick >= 0.04) & (pick < 0.08)]
    c["r"][(pick >= 0.08) & (pick < 0.09)] = HAND["r_disc"]                 # the outer edge itself is outside
    c["emit"][(pick >= 0.09) & (pick < 0.12)] *= -1
    c["emit"][(pick >= 0.12) & (pick < 0.14)] = math.nan
    if bundles:
        spick, sat = rng.random((nx, ny)), rng.integers(1, 5, size=(nx, ny))
        for m in range(1, 5):
            rays[:, :, m]["r"][(sat == m) & (spick < 0.05)] = HAND["r_disc"] + 1.0
        swap = (spick >= 0.05) & (spick < 0.15)
        east = rays[:, :, 1][swap].copy()
        rays[:, :, 1][swap] = rays[:, :, 2][swap]
        rays[:, :, 2][swap] = east
    out = rays.reshape(-1)
    if trailing:
        tail = np.repeat(rays[nx // 2, ny // 2, :1], trailing)
        tail["r"], tail["steps"], tail["status"], tail["emit"] = 0.5 * (r_isco + HAND["r_disc"]), 50, capi.STATUS_DEST, 0.9
        out = np.concatenate([out, tail])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", ["bundles", "grid"])
def test_disc_maps_on_hand_made_records(dev, mode, shape):
    """kr_post_caustic_disc_dev_f64 + kr_caustic_suppress_dev_f64 on hand-made records at the last-chunk shapes of the 64-pixel bundle pass and the
    256-thread grid pass and on planes that are all border, with 37 trailing records, judged by caustic_rules on the records read back (they carry the
    device's redshift) with the bars of test_map_kernels_match_the_rules_on_the_same_records: c = 1e-12 r_disc on PHI, X_DISC, Y_DISC, det_bound on
    DET_J, SIGN_J wherever |det| is not below that bound (no such pixel may exist here); everything else equal.  Every word of the 0xFF-prefilled
    buffer is written; the records, trailing ones included, equal kr_redshift_dest_dev_f64 on a copy in every field; suppression is bit-exact against
    the rules on the device's own maps; the same words come out with the trailing records cut off."""
    L, (nx, ny), bundles = dev.lib, shape, mode == "bundles"
    r_isco = L.kr_kerr_isco(HAND["spin"], 1)
    g = dict(HAND, nx=nx, ny=ny)
    cm = caustic_struct(g, r_isco, bundles)
    nw, npix, rpb = api.caustic_words(cm), nx * ny, 5 if bundles else 1
    rays = disc_records(bundles, nx, ny, r_isco, seed=nx * 1000 + ny, trailing=37)
    n = len(rays)
    assert n == rpb * npix + 37

    def run(records):
        d = dev.upload(records)
        d_maps = dev.alloc(nw * 8)
        capi.check(L, L.kr_memset(d_maps, 0xff, nw * 8), "kr_memset")
        capi.check(L, L.kr_post_caustic_disc_dev_f64(-HAND["spin"], 1, C.byref(cm), d, len(records), d_maps, None), "kr_post_caustic_disc")
        before = dev.fetch(d_maps, nw)
        capi.check(L, L.kr_caustic_suppress_dev_f64(C.byref(cm), d_maps, None), "kr_caustic_suppress")
        return before, dev.fetch(d_maps, nw), dev.fetch(d, len(records), capi.RAY_F64)

    words_before, words_after, fused = run(rays)
    d_copy = dev.upload(rays)
    capi.check(L, L.kr_redshift_dest_dev_f64(-HAND["spin"], 1, d_copy, n, None), "kr_redshift_dest")
    separate = dev.fetch(d_copy, n, capi.RAY_F64)
    for f in fused.dtype.names:
        assert same_bits(fused[f], separate[f]).all(), f
    with np.errstate(invalid="ignore"):
        positive = fused["redshift"] > 0
    assert positive.mean() > 0.8 and positive[-37:].all()
    for w in (words_before, words_after):
        assert not (w.view(np.uint64) == 0xFFFFFFFFFFFFFFFF).any() and not np.isnan(w[9 * npix:]).any(), "a word was not written"
    before, counts_before = planes_of(cm, words_before)
    after, counts = planes_of(cm, words_after)

    want, want_counts, G = (cr.bundle_maps if bundles else cr.grid_maps)(fused, nx, ny, r_isco, HAND["r_disc"], cm.eps_x, cm.eps_y)
    assert counts_before["suppressed"] == 0
    for k, v in want_counts.items():
        assert counts_before[k] == v == counts[k], (k, counts_before[k], v)
    for k in ("HIT", "ORDER"):
        assert np.array_equal(before[k], want[k]), k
    for k in ("RADIUS", "REDSHIFT"):
        assert cr.bits_equal(before[k], want[k]).all(), k
    c = 1e-12 * HAND["r_disc"]
    worst = {}
    for k in ("PHI", "X_DISC", "Y_DISC"):
        diff = np.abs(before[k] - want[k])
        worst[k] = float(diff.max())
        assert (diff <= c).all(), (k, worst[k], c)
    gd, wd = before["DET_J"], want["DET_J"]
    assert np.array_equal(np.isnan(gd), np.isnan(wd)) and np.array_equal(gd == cr.SENTINEL, wd == cr.SENTINEL)
    defined = ~np.isnan(wd) & (wd != cr.SENTINEL)
    bound = cr.det_bound(c, min(cm.eps_x, cm.eps_y), G)
    ratio = (np.abs(gd - wd)[defined] / bound[defined]) if defined.any() else np.zeros(1)
    hits, n_sentinel = want_counts["disc_count"], int((wd == cr.SENTINEL).sum())
    print(mode, shape, "hits", hits, "defined", int(defined.sum()), "sentinel", n_sentinel, "g <= 0 or NaN", int((~positive).sum()), "worst coordinate differences",
          worst, "worst |d det| / bound", float(ratio.max()), "suppressed", counts["suppressed"])
    assert (ratio <= 1).all(), float(ratio.max())
    ambiguous = defined & (np.abs(wd) < bound)
    assert not ambiguous.any()
    assert np.array_equal(before["SIGN_J"], want["SIGN_J"])
    parity.record_margin("test_disc_maps_on_hand_made_records", f"{mode}-{nx}x{ny}",
                         {"n_traced": int(defined.sum()), "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(ratio.max())}, worst_coordinate_difference=max(worst.values()))
    if not bundles and (nx < 3 or ny < 3):
        assert np.isnan(gd).all() and (before["SIGN_J"] == 0).all()
    if npix >= 63:
        assert 0 < hits < npix and (~positive).any()
        if bundles or (nx >= 3 and ny >= 3):
            assert defined.any()
    if npix >= 129 and (bundles or min(nx, ny) >= 5):
        assert n_sentinel > 0

    # the suppression pass on the device's own maps: no tolerance
    expect = {"DET_J": before["DET_J"].copy(), "SIGN_J": before["SIGN_J"].copy()}
    n_supp = cr.suppress(expect)
    assert counts["suppressed"] == n_supp
    assert cr.bits_equal(after["DET_J"], expect["DET_J"]).all() and np.array_equal(after["SIGN_J"], expect["SIGN_J"])
    for k in ("ORDER", "HIT", "RADIUS", "PHI", "X_DISC", "Y_DISC", "REDSHIFT"):
        assert cr.bits_equal(after[k], before[k]).all(), k
    if bundles and npix >= 129:
        assert n_supp > 0
    # trailing records are no pixels
    cut_before, cut_after, _ = run(rays[:rpb * npix])
    assert cut_before.tobytes() == words_before.tobytes() and cut_after.tobytes() == words_after.tobytes()


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
