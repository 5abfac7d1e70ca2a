"""GPU: emission-line profiles and transfer functions (kr_line_bins; kr_reduce_line_*, kr_post_line_dev_f64, kr_line_from_image_dev_f64,
api.line_profile, apps/kr_line_profile) against the reference's own image (tests/golden/apps/imageplane_rk4.fits, through the notebook's
per-pixel rule), the compiled reference's rays, the separate passes, and each other.  Bin rules restated in numpy: tests/line_rules.py."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import line_rules as lr
import oracle_lib as ol
import parity
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPS = os.path.join(ROOT, "tests", "golden", "apps")
FITS = os.path.join(APPS, "imageplane_rk4.fits")
PAR = os.path.join(APPS, "imageplane_rk4.par")
EMIS_DAT = os.path.join(APPS, "emissivity.dat")
SPIN, DIST, INCL, R_DISC = 0.998, 10000.0, 80.0, 30.0


def r_isco():
    return api.lib().kr_kerr_isco(SPIN, 1)


def image_params():
    """What kr_imageplane_disc_image / kr_line_profile trace with (RK4, the default hybrid arithmetic)."""
    p = capi.default_params(-SPIN)
    p.precision, p.integrator, p.theta_max, p.r_max = 100.0, capi.RK4, math.pi / 2, 1.1 * DIST
    p.stop_kind, p.flags = capi.STOP_THETA, capi.FLAG_HYBRID
    return p


def plane(nx):
    d = 2 * R_DISC / nx
    return ol.imageplane_spec(DIST, INCL, -R_DISC, R_DISC, d, -R_DISC, R_DISC, d, SPIN)


def image_bins(img_nx):
    ib = capi.ImageBins()
    ib.x0 = ib.y0 = -R_DISC
    ib.img_dx = ib.img_dy = 2 * R_DISC / img_nx
    ib.r_isco, ib.r_disc = r_isco(), R_DISC
    ib.q1, ib.rb1, ib.q2, ib.rb2, ib.q3 = 3.0, 4.0, 3.0, 10.0, 3.0
    ib.img_nx = ib.img_ny = img_nx
    ib.flip_image = 1
    return ib


def line_bins(**kw):
    base = dict(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=r_isco(), r_disc=R_DISC, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0)
    base.update(kw)
    return capi.line_bins(**base)


def table_bins(b):
    r_min, dr, emis, time = lr.read_emissivity_dat(EMIS_DAT)
    return b.with_table(r_min, dr, emis, time)


def post_line(b, rays):
    """kr_post_line_dev_f64 on a device copy of `rays` (traced, not yet redshifted): (histogram dict, rays after the pass)."""
    L = api.lib()
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(api.line_words(b) * 8)
        capi.check(L, L.kr_post_line_dev_f64(-SPIN, -1.0, 1, 0, 0, -math.pi, math.pi, C.byref(b), d, len(rays), h, None), "kr_post_line")
        out, words = dev.fetch(d, len(rays), rays.dtype), dev.fetch(h, api.line_words(b))
    return api.line_from_words(b, words), out


def reduce_line_dev(b, rays):
    L = api.lib()
    with DeviceScope(L) as dev:
        d, h = dev.upload(rays), dev.zeros(api.line_words(b) * 8)
        capi.check(L, L.kr_reduce_line_dev_f64(C.byref(b), d, len(rays), h, None), "kr_reduce_line_dev")
        return api.line_from_words(b, dev.fetch(h, api.line_words(b)))


def check(test, case, got, want, rtol=1e-6, slack=1, max_excluded=None):
    problems, m = lr.compare_line(got, want, rtol=rtol, slack=slack, max_excluded=max_excluded)
    parity.record_margin(test, case, {"n_traced": int(np.asarray(want["count"]).sum()), "n_bad": m["bins_excluded"], "frac_bad": 0.0,
                                      "worst_ok": m["worst_flux_rel"]}, rtol, max_count_diff=m["max_count_diff"], allowed_excluded=m["allowed"])
    assert problems == [], (case, problems, m)
    return m


# ---- 3. against the reference's own image -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_axis", [False, True])
def test_pixels_mode_matches_the_notebook_line_of_the_reference_image(krlib, time_axis):
    want_b = line_bins()
    if time_axis:
        import fits_lite
        t = {h["name"]: h["data"] for h in fits_lite.read(FITS)}["TIME"]
        lo, hi = float(np.nanmin(t)), float(np.nanmax(t))
        want_b = line_bins(nt=8, t0=lo - 1.0, dt=(hi - lo + 2.0) / 8)
    want = lr.line_from_fits(want_b, FITS)
    assert want["binned"] > 50
    got = api.line_profile(plane(31), image_params(), want_b, mode="pixels", image_bins=image_bins(16))
    assert abs(got["on_disc"] - want["on_disc"]) <= 2
    check("test_pixels_mode_matches_the_notebook_line_of_the_reference_image", f"imageplane_rk4-time{int(time_axis)}", got, want)


# ---- 4. against the compiled reference's rays ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_rays():
    """129 x 129 image plane through the compiled reference: ctor -> redshift_start -> RK4 -> redshift(-1, reverse) -> range_phi.
    Returns (initial records after redshift_start, the reference's final records)."""
    if ol.ref() is None:
        pytest.fail("compiled reference (oracle/_ref) not available")
    src = ol.RefSource(plane(128))
    src.lib.ref_redshift_start(src.h, 0.0, 1, 0)
    init = src.snapshot()
    src.run(image_params())
    src.lib.ref_redshift(src.h, -1.0, 1, 0, 0)
    src.lib.ref_range_phi(src.h, -math.pi, math.pi)
    out = src.snapshot()
    src.close()
    return init, out


@pytest.fixture(scope="module")
def traced(krlib, ref_rays):
    init, _ = ref_rays
    out, _ = api.trace(image_params(), init)
    return out


def _tau_range(b, rays):
    m = lr.disc_filter(b, rays)
    _, _, tau, ok = lr.items(b, rays["r"][m], rays["redshift"][m], rays["t"][m])
    tau = tau[ok & np.isfinite(tau)]
    return float(tau.min()), float(tau.max())


def _variants(ref_out):
    out = {}
    for log_e in (False, True):
        for table in (False, True):
            for time_axis in (False, True):
                kw = dict(log_e=True, e_min=1.0, de=1.02, ne=120) if log_e else {}
                b = line_bins(**kw)
                if table:
                    b = table_bins(b)
                if time_axis:
                    lo, hi = _tau_range(b, ref_out)
                    kw.update(nt=20, t0=0.0, dt=(hi - lo) * 1.02 / 20)
                    b = line_bins(**kw)
                    if table:
                        b = table_bins(b)
                    b.t0 = lo - 0.01 * (hi - lo)
                out[f"{'log' if log_e else 'lin'}-{'table' if table else 'pl3'}-{'t' if time_axis else 'not'}"] = b
    return out


def test_post_line_matches_the_reference_rays(ref_rays, traced):
    _, ref_out = ref_rays
    for case, b in _variants(ref_out).items():
        want = lr.line_from_rays(b, ref_out)
        assert want["binned"] > 1000, case
        got, _ = post_line(b, traced)
        assert abs(got["on_disc"] - want["on_disc"]) <= 16, case
        check("test_post_line_matches_the_reference_rays", case, got, want)


# ---- 5. fused == separate ----------------------------------------------------------------------------------------------------------
def test_fused_equals_separate_passes(ref_rays, traced):
    _, ref_out = ref_rays
    sep = traced.copy()
    api.redshift(-SPIN, -1.0, 1, 0, sep)
    api.range_phi(sep, -math.pi, math.pi)
    for case, b in _variants(ref_out).items():
        fused, fused_rays = post_line(b, traced)
        assert ol.rays_equal_bitwise(fused_rays, sep) == [], case
        for name, other in (("reduce_line_dev", reduce_line_dev(b, sep)), ("reduce_line_f64", api.reduce_line(b, fused_rays))):
            assert (other["count"] == fused["count"]).all() and other["on_disc"] == fused["on_disc"] and other["binned"] == fused["binned"], (case, name)
            check("test_fused_equals_separate_passes", f"{case}-{name}", other, fused, rtol=1e-12, slack=0, max_excluded=0)
        # and the device's own records through the numpy rules: the same bins, up to the last-ulp log / pow of an item on a bin edge
        check("test_fused_equals_separate_passes", f"{case}-numpy", fused, lr.line_from_rays(b, fused_rays), rtol=1e-9, slack=1, max_excluded=2)


# ---- 6. LDS and global histograms agree; edge cases -------------------------------------------------------------------------------
def test_lds_and_global_paths_agree(ref_rays, traced):
    _, ref_out = ref_rays
    _, rays = post_line(line_bins(), traced)
    lo, hi = _tau_range(line_bins(), rays)
    small = line_bins(ne=100, nt=10, t0=lo - 1.0, dt=(hi - lo + 2.0) / 10)         # 2002 words: LDS
    big = line_bins(ne=100, nt=40, t0=lo - 1.0, dt=(hi - lo + 2.0) / 40)           # 8002 words: global atomics
    assert api.line_words(small) <= 4096 < api.line_words(big)
    for b in (small, big):
        got = api.reduce_line(b, rays)
        check("test_lds_and_global_paths_agree", f"nt{b.nt}", got, lr.line_from_rays(b, rays), rtol=1e-9, slack=1, max_excluded=2)
    # the 40 fine time bins summed in fours are the 10 coarse ones, bin for bin
    g_small, g_big = api.reduce_line(small, rays), api.reduce_line(big, rays)
    assert (g_big["count"].reshape(10, 4, 100).sum(axis=1) == g_small["count"]).all()
    np.testing.assert_allclose(g_big["flux"].reshape(10, 4, 100).sum(axis=1), g_small["flux"], rtol=1e-12, atol=0)


def _edge_rays():
    rays = np.zeros(10, dtype=capi.RAY_F64)
    rays["steps"], rays["theta"] = 1, np.pi / 2
    rays["r"] = [5.0, 5.0, 5.0, 5.0, 0.5, 50.0, 5.0, 5.0, 12.0, 5.0]
    rays["redshift"] = [1.0, 0.5, np.nan, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, -1.0]
    rays["t"] = [0.0, 0.0, 0.0, 99.0, 0.0, 0.0, 1.5, 0.0, 0.25, 0.0]
    return rays


@pytest.mark.parametrize("nt", [2, 4000])
@pytest.mark.parametrize("table", [False, True])
def test_edge_cases_on_both_paths(krlib, nt, table):
    """E exactly on a bin edge (lower in, upper out), NaN and negative redshift, rays outside the table and at a NaN table entry,
    tau outside the time range -- identical on the LDS (nt = 2) and the global (nt = 4000) histogram."""
    rays = _edge_rays()
    b = capi.line_bins(line_energy=4.0, e_min=1.0, de=0.5, ne=14, nt=nt, t0=0.0, dt=1.0, r_isco=0.1, r_disc=1e9)
    if table:
        b.with_table(1.0, 2.0, np.array([1.0, 2.0, 3.0, np.nan]), np.array([0.0, 0.5, 0.0, 0.0]))
    assert (api.line_words(b) <= 4096) == (nt == 2)
    got, want = api.reduce_line(b, rays), lr.line_from_rays(b, rays)
    assert got["on_disc"] == want["on_disc"] == 8 and got["binned"] == want["binned"]
    assert got["binned"] == (3 if table else 6) + (nt > 99)          # t = 99 is inside the 4000 time bins only
    assert (got["count"] == want["count"]).all()
    np.testing.assert_allclose(got["flux"], want["flux"], rtol=1e-14, atol=0)


# ---- 7. rays vs pixels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True])
def test_rays_and_pixels_modes_agree_with_one_ray_per_pixel(krlib, table):
    spec = plane(128)
    b = line_bins(log_e=True, e_min=1.0, de=1.02, ne=120)
    if table:
        b = table_bins(b)
    rays = api.line_profile(spec, image_params(), b, mode="rays")
    pix = api.line_profile(spec, image_params(), b, mode="pixels")          # default image bins: one pixel per ray, centred on it
    assert rays["on_disc"] == pix["on_disc"] > 2000
    check("test_rays_and_pixels_modes_agree_with_one_ray_per_pixel", f"table{int(table)}", pix, rays, rtol=1e-12, slack=1, max_excluded=4)
    assert abs(rays["binned"] - pix["binned"]) <= 2


# ---- 8. the app -------------------------------------------------------------------------------------------------------------------
def run_app(*extra):
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_line_profile")
    assert os.path.exists(exe), "kr_line_profile not built (__graft_entry__.build())"
    with tempfile.TemporaryDirectory() as w:
        out = os.path.join(w, "line.dat")
        r = subprocess.run([exe, f"--parfile={PAR}", f"--outfile={out}", "--timing", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "timing: rays" in r.stdout
        rows = np.array([[float(x) for x in l.split()] for l in open(out) if l.strip()])
    return rows


@pytest.mark.parametrize("mode", ["rays", "pixels"])
@pytest.mark.parametrize("table", [False, True])
def test_line_profile_app(krlib, mode, table):
    extra = [f"--line_mode={mode}", "--e_min=1", "--e_max=10", "--ne=90"]
    b = line_bins()
    if table:
        extra.append(f"--emis_file={EMIS_DAT}")
        b = table_bins(b)
    rows = run_app(*extra)
    assert rows.shape == (90, 4) and np.isnan(rows[:, 0]).all()
    np.testing.assert_allclose(rows[:, 1], 1.05 + 0.1 * np.arange(90), rtol=1e-7)
    got = {"count": rows[None, :, 3], "flux": rows[None, :, 2]}
    if mode == "pixels":
        want = lr.line_from_fits(b, FITS)                           # test 3's expectation: the reference image's notebook line
    else:
        want = api.line_profile(plane(31), image_params(), b, mode="rays")
    check("test_line_profile_app", f"{mode}-table{int(table)}", got, want, rtol=1e-6)
    assert rows[:, 3].sum() > 50


def test_line_profile_app_time_axis(krlib):
    # the arrival times of this geometry lie in 9984 .. 10047 (TIME plane of the reference's image)
    rows = run_app("--line_mode=rays", "--log_e=1", "--e_min=2", "--e_max=9", "--ne=60", "--nt=5", "--t0=9980", "--dt=15")
    assert rows.shape == (300, 4)
    b = line_bins(log_e=True, e_min=2.0, de=math.exp(math.log(9 / 2) / 60), ne=60, nt=5, t0=9980.0, dt=15.0)
    want = api.line_profile(plane(31), image_params(), b, mode="rays")
    assert want["binned"] > 100 and (want["count"].sum(axis=1) > 0).sum() >= 3
    np.testing.assert_allclose(rows[::60, 0], 9980 + 15 * (np.arange(5) + 0.5))
    check("test_line_profile_app_time_axis", "rays-log-t", {"count": rows[:, 3].reshape(5, 60), "flux": rows[:, 2].reshape(5, 60)}, want, rtol=1e-6)


# ---- 9. more distinct tables than the device table store keeps --------------------------------------------------------------------
def test_line_tables_survive_churn_of_the_table_store(traced):
    """300 distinct emissivity tables (the fixture's, scaled) against a store of 256 per device: each one's line through kr_reduce_line_dev_f64
    on the same records, every tenth through kr_post_line_dev_f64 as well -- each against the numpy rules for that table."""
    L = api.lib()
    _, rays = post_line(line_bins(), traced)
    r_min, dr, emis, time = lr.read_emissivity_dat(EMIS_DAT)
    with DeviceScope(L) as dev:
        d = dev.upload(rays)
        for i in range(300):
            b = line_bins().with_table(r_min, dr, emis * (1 + 0.01 * i), time)
            want = lr.line_from_rays(b, rays)
            with DeviceScope(L) as one:
                h = one.zeros(api.line_words(b) * 8)
                capi.check(L, L.kr_reduce_line_dev_f64(C.byref(b), d, len(rays), h, None), "kr_reduce_line_dev")
                got = api.line_from_words(b, one.fetch(h, api.line_words(b)))
            problems, m = lr.compare_line(got, want, rtol=1e-9, slack=1, max_excluded=2)
            assert problems == [], (i, problems, m)
            if i % 10 == 0:
                got, _ = post_line(b, traced)
                problems, m = lr.compare_line(got, want, rtol=1e-9, slack=1, max_excluded=2)
                assert problems == [], (i, "post_line", problems, m)
