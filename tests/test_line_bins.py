"""CPU: the emission-line ABI (kr_line_bins) -- struct layout, refusal of invalid bins before any device work -- and the numpy restatement
of the binning rules (tests/line_rules.py) against the reference notebook's own computation (python/line_from_image.ipynb) on the
reference's image FITS file."""
import ctypes as C
import os

import numpy as np
import pytest

import line_rules as lr
from raytrace_cpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITS = os.path.join(ROOT, "tests", "golden", "apps", "imageplane_rk4.fits")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def test_line_bins_layout_matches_header(lib):
    assert C.sizeof(capi.LineBins) == 160
    off = {n: getattr(capi.LineBins, n).offset for n, _ in capi.LineBins._fields_}
    assert off["line_energy"] == 0 and off["g_index"] == 96 and off["table_dr"] == 112
    assert off["table_emis"] == 120 and off["table_time"] == 128 and off["ne"] == 136 and off["pad"] == 156
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()


def _valid():
    return capi.line_bins(e_min=1.0, de=0.1, ne=90, r_isco=1.237, r_disc=30.0)


EMIS = np.ones(4)


def _invalid_cases():
    def mk(**kw):
        b = _valid()
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    cases = {
        "ne0": mk(ne=0), "nt0": mk(nt=0), "de0": mk(de=0.0), "de_neg": mk(de=-0.1),
        "log_de1": mk(log_e=1, de=1.0), "log_emin0": mk(log_e=1, de=1.1, e_min=0.0),
        "nt2_dt0": mk(nt=2, dt=0.0), "nan_emin": mk(e_min=float("nan")), "inf_line": mk(line_energy=float("inf")),
        "nan_dt": mk(dt=float("nan")), "nan_gindex": mk(g_index=float("nan")), "too_many_bins": mk(ne=4097, nt=4097, dt=1.0),
    }
    b = _valid()
    b.table_time = EMIS.ctypes.data_as(C.POINTER(C.c_double))
    b.table_nr = 4
    cases["time_without_emis"] = b
    b = _valid().with_table(1.0, 1.1, EMIS)
    b.table_nr = 0
    cases["table_nr0"] = b
    return cases


@pytest.mark.parametrize("case", sorted(_invalid_cases()))
def test_invalid_line_bins_are_refused_without_a_device(lib, case):
    b = _invalid_cases()[case]
    rays = np.zeros(4, dtype=capi.RAY_F64)
    out = np.zeros(8)
    img = capi.ImageBins()
    img.img_nx = img.img_ny = 1
    dummy = C.c_void_p(16)          # never dereferenced: validation comes first
    calls = [
        ("kr_reduce_line", lambda: lib.kr_reduce_line_f64(C.byref(b), rays.ctypes.data_as(C.c_void_p), len(rays), out.ctypes.data_as(C.c_void_p))),
        ("kr_reduce_line", lambda: lib.kr_reduce_line_dev_f64(C.byref(b), dummy, 4, dummy, None)),
        ("kr_post_line", lambda: lib.kr_post_line_dev_f64(-0.998, -1.0, 1, 0, 0, -np.pi, np.pi, C.byref(b), dummy, 4, dummy, None)),
        ("kr_line_from_image", lambda: lib.kr_line_from_image_dev_f64(C.byref(b), C.byref(img), dummy, dummy, None)),
    ]
    for name, call in calls:
        assert call() == capi.KR_EINVAL, (case, name)
        msg = lib.kr_last_error().decode()
        assert msg.startswith(name + ":") and len(msg) > len(name) + 3, (case, msg)


def test_valid_line_bins_pass_validation(lib):
    """A valid bin set gets past validation: without a GPU the call then reports the missing device, not EINVAL."""
    if lib.kr_device_count() > 0:
        pytest.skip("a GPU is visible")
    for b in (_valid(), capi.line_bins(log_e=True, e_min=1.0, de=1.02, ne=120, nt=50, t0=-5.0, dt=2.0).with_table(1.2, 1.1, EMIS, EMIS)):
        rays = np.zeros(4, dtype=capi.RAY_F64)
        out = np.zeros(2 * b.nt * b.ne + 2)
        assert lib.kr_reduce_line_f64(C.byref(b), rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_ENODEVICE


def test_numpy_rules_reproduce_the_notebook_line():
    """line_rules' per-pixel form on the reference's image FITS file == the notebook's computation, with the notebook's broken power law
    written as powerlaw3 (q3 = q2, rb2 beyond the disc) and its bins np.arange(1, 10, 0.1)."""
    edges = np.arange(1, 10, 0.1)
    for q1, rbreak, q2 in ((3.0, 5.0, 3.0), (2.0, 6.0, 3.5)):
        want_flux, want_count = lr.notebook_line(FITS, 6.4, edges, q1, rbreak, q2)
        b = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=len(edges) - 1, r_isco=0.0, r_disc=1e300, q1=q1, rb1=rbreak, q2=q2, rb2=1e9, q3=q2)
        got = lr.line_from_fits(b, FITS)
        assert got["count"].sum() > 50 and want_count.sum() == got["binned"]
        problems, margins = lr.compare_line(got, {"count": want_count[None, :], "flux": want_flux[None, :]}, rtol=1e-12, slack=0)
        assert problems == [], (problems, margins)


def test_numpy_rules_time_axis_and_log_bins():
    """Hand-made records: bin edges (lower edge in, upper edge out), NaN redshift, rays outside the table, tau outside the time range."""
    rays = np.zeros(8, dtype=capi.RAY_F64)
    rays["steps"], rays["theta"] = 1, np.pi / 2
    rays["r"] = [5.0, 5.0, 5.0, 5.0, 0.5, 50.0, 5.0, 5.0]
    rays["redshift"] = [1.0, 0.5, np.nan, 1.0, 1.0, 1.0, 1.0, 1.0]
    rays["t"] = [0.0, 0.0, 0.0, 99.0, 0.0, 0.0, 1.5, 0.0]
    b = capi.line_bins(line_energy=4.0, e_min=1.0, de=0.5, ne=14, nt=2, t0=0.0, dt=1.0, r_isco=0.1, r_disc=1e9)
    got = lr.line_from_rays(b, rays)
    # on the disc: all but the NaN one (7); binned: E = 4 (bin 6) for rays 0, 4, 5 (no table), ray 6 in time bin 1; E = 8 is the upper edge
    assert got["on_disc"] == 7 and got["binned"] == 5
    assert got["count"][0, 6] == 4 and got["count"][1, 6] == 1 and got["count"].sum() == 5
    b.with_table(1.0, 2.0, np.array([1.0, 2.0, 3.0, np.nan]), np.array([0.0, 0.5, 0.0, 0.0]))
    got = lr.line_from_rays(b, rays)
    # table index of r = 5: trunc(log2(5)) = 2; r = 0.5 -> -1 (outside); r = 50 -> 5 (outside); tau of ray 6 = 1.5 + 0 -> time bin 1
    assert got["on_disc"] == 7 and got["binned"] == 3 and got["count"][0, 6] == 2 and got["count"][1, 6] == 1
    assert np.isclose(got["flux"][0, 6], 2 * 3.0)
