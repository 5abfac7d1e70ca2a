"""CPU: the C ABI of the passes over rays that landed on a disc surface (kr_disc_surface; kr_angles_surface_*, kr_post_/kr_reduce_line_surface_*,
kr_post_/kr_reduce_spectrum_surface_*, kr_post_/kr_reduce_response_surface_*): the struct's size against the header's static_assert, every refusal with
its message -- before any device is touched, so the dummy device pointers below are never dereferenced --, the output layouts against the api's
*_from_words, the api's own refusals and, on a machine without a GPU, KR_ENODEVICE for a valid call (there is no CPU fallback)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.capi import KrError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
DUMMY = C.c_void_p(16)          # a "device pointer": only ever handed to calls that are refused, or made where there is no device
POST = (-0.5, 1, -math.pi, math.pi)          # spin as stored, reverse, lo, hi
GOOD = (4.233, 30.0, 0.1, 1.0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def line_bins(**kw):
    b = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=4.233, r_disc=30.0)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def table(**kw):
    m = capi.spectrum_model("table", 0.1, 0.1, 64, r_isco=4.233, r_disc=30.0, s=np.ones((2, 16)), s_e_min=0.05, s_de=1.5)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def thermal():
    return capi.spectrum_model("thermal", 0.1, 0.1, 64, r_isco=4.233, r_disc=30.0, f_col=1.7, table_r_min=4.233, table_dr=1.1, table_kt=np.full(40, 0.5))


def response(spec=None, **kw):
    R = capi.response_model(spec if spec is not None else table(), 1000.0, 1.0, 8)
    for k, v in kw.items():
        setattr(R, k, v)
    return R


def entry_points(lib, sref, b=None, m=None, R=None, law=None, d=DUMMY, n=4, out=DUMMY):
    """who -> a call of every device entry point with the surface reference `sref`; the rest valid unless given."""
    b = b if b is not None else line_bins()
    m = m if m is not None else table()
    R = R if R is not None else response()
    law = C.byref(law if law is not None else capi.limb_law("laor"))
    keep = (b, m, R)                                                                   # (alive while the lambdas are)
    return {
        "kr_angles_surface": lambda: (keep, lib.kr_angles_surface_dev_f64(sref, -0.5, 1, d, n, out, None))[1],
        "kr_post_line_surface": lambda: lib.kr_post_line_surface_dev_f64(sref, *POST, C.byref(b), law, d, n, out, None),
        "kr_reduce_line_surface": lambda: lib.kr_reduce_line_surface_dev_f64(sref, C.byref(b), d, n, out, None),
        "kr_post_spectrum_surface": lambda: lib.kr_post_spectrum_surface_dev_f64(sref, *POST, C.byref(m), law, d, n, out, None),
        "kr_reduce_spectrum_surface": lambda: lib.kr_reduce_spectrum_surface_dev_f64(sref, C.byref(m), d, n, out, None),
        "kr_post_response_surface": lambda: lib.kr_post_response_surface_dev_f64(sref, *POST, C.byref(R), law, d, n, out, None),
        "kr_reduce_response_surface": lambda: lib.kr_reduce_response_surface_dev_f64(sref, C.byref(R), d, n, out, None),
    }


def host_entry_points(lib, sref, m=None, R=None, rays=None, out=None, n=4):
    m = m if m is not None else table()
    R = R if R is not None else response()
    return {
        "kr_angles_surface": lambda: lib.kr_angles_surface_f64(sref, -0.5, 1, rays, n, out),
        "kr_reduce_spectrum_surface": lambda: (m, lib.kr_reduce_spectrum_surface_f64(sref, C.byref(m), rays, n, out))[1],
        "kr_reduce_response_surface": lambda: (R, lib.kr_reduce_response_surface_f64(sref, C.byref(R), rays, n, out))[1],
    }


def test_struct_size_and_symbols(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_disc_surface\) == (\d+)", header).group(1))
    assert C.sizeof(capi.DiscSurface) == size == 32
    assert [capi.DiscSurface.r_in.offset, capi.DiscSurface.r_out.offset, capi.DiscSurface.slope.offset, capi.DiscSurface.scale.offset] == [0, 8, 16, 24]
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()                          # additive: ten more entry points
    names = ["kr_angles_surface_dev_f64", "kr_angles_surface_f64", "kr_post_line_surface_dev_f64", "kr_reduce_line_surface_dev_f64",
             "kr_post_spectrum_surface_dev_f64", "kr_reduce_spectrum_surface_dev_f64", "kr_reduce_spectrum_surface_f64", "kr_post_response_surface_dev_f64",
             "kr_reduce_response_surface_dev_f64", "kr_reduce_response_surface_f64"]
    for name in names:
        assert name in capi.PROTOTYPES and hasattr(lib, name) and re.search(rf"\bint {name}\(const kr_disc_surface\* s,", header), name
    s = capi.disc_surface(GOOD)
    assert (s.r_in, s.r_out, s.slope, s.scale) == GOOD and capi.disc_surface(s) is s
    # the surface is the stop_params of the thick-disc stop, in its order
    p = api.thick_disc_params(capi.default_params(-0.5), *GOOD)
    assert p.stop_kind == capi.STOP_THICKDISC and tuple(p.stop_params[:4]) == GOOD


SURFACES = [
    ("null surface", None, "null surface"),
    ("r_in 0", (0.0, 30.0, 0.1, 1.0), "surface: r_in must be positive and finite"),
    ("r_in negative", (-1.0, 30.0, 0.1, 1.0), "surface: r_in must be positive and finite"),
    ("r_in nan", (NAN, 30.0, 0.1, 1.0), "surface: r_in must be positive and finite"),
    ("r_in inf", (INF, 30.0, 0.1, 1.0), "surface: r_in must be positive and finite"),
    ("r_out nan", (4.2, NAN, 0.1, 1.0), "surface: r_out must be finite (<= 0: open)"),
    ("r_out inf", (4.2, INF, 0.1, 1.0), "surface: r_out must be finite (<= 0: open)"),
    ("slope negative", (4.2, 30.0, -0.1, 1.0), "surface: slope must be non-negative and finite"),
    ("slope nan", (4.2, 30.0, NAN, 1.0), "surface: slope must be non-negative and finite"),
    ("scale negative", (4.2, 30.0, 0.1, -1.0), "surface: scale must be non-negative and finite"),
    ("scale inf", (4.2, 30.0, 0.1, INF), "surface: scale must be non-negative and finite"),
]


@pytest.mark.parametrize("label,surface,why", SURFACES, ids=[s[0] for s in SURFACES])
def test_bad_surfaces_are_refused_before_any_device_work(lib, label, surface, why):
    s = capi.disc_surface(surface) if surface is not None else None
    sref = C.byref(s) if s is not None else None
    for who, call in entry_points(lib, sref).items():
        assert call() == capi.KR_EINVAL, (who, label)
        assert lib.kr_last_error().decode() == f"{who}: {why}", (who, label)
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(600, 7.0)
    for who, call in host_entry_points(lib, sref, rays=rays.ctypes.data_as(C.c_void_p), out=out.ctypes.data_as(C.c_void_p)).items():
        assert call() == capi.KR_EINVAL, (who, label)
        assert lib.kr_last_error().decode() == f"{who}: {why}", (who, label)
    assert (out == 7.0).all()                                                       # a refused call writes nothing


def test_the_stop_refuses_the_same_surfaces(lib):
    """The surface's rules are the stop's own: what kr_trace refuses of the stop_params of KR_STOP_THICKDISC, the surface passes refuse, and an open
    surface (r_out <= 0) and a flat one (slope = scale = 0) pass both."""
    rays = np.zeros(4, dtype=capi.RAY_F64)
    for label, surface, _ in SURFACES[1:]:
        p = api.thick_disc_params(capi.default_params(-0.5), *surface)
        p.integrator = capi.RK4
        assert lib.kr_trace_f64(C.byref(p), rays.ctypes.data_as(C.c_void_p), 4, None) == capi.KR_EINVAL, label
        assert "KR_STOP_THICKDISC" in lib.kr_last_error().decode(), label
    for surface in ((4.2, 0.0, 0.0, 0.0), (4.2, -1.0, 0.1, 0.0)):
        s = capi.disc_surface(surface)
        rc = lib.kr_angles_surface_dev_f64(C.byref(s), -0.5, 1, None, 0, None, None)
        assert rc in (capi.KR_OK, capi.KR_ENODEVICE), surface


def test_the_flat_validation_stays(lib):
    """The bins, the model, the response and the limb law are validated as the flat twins validate them, under the surface entry point's name."""
    s = C.byref(capi.disc_surface(GOOD))
    cases = [
        (dict(b=line_bins(ne=0)), ("kr_post_line_surface", "kr_reduce_line_surface"), "ne and nt must be >= 1"),
        (dict(b=line_bins(de=0.0)), ("kr_post_line_surface", "kr_reduce_line_surface"), "de must be positive"),
        (dict(b=line_bins(nt=3, dt=0.0)), ("kr_post_line_surface", "kr_reduce_line_surface"), "nt > 1 needs dt > 0"),
        (dict(m=table(ne=4097)), ("kr_post_spectrum_surface", "kr_reduce_spectrum_surface"), "ne must be in 1 ... 4096"),
        (dict(m=table(model=2)), ("kr_post_spectrum_surface", "kr_reduce_spectrum_surface"), "model must be 0 (thermal) or 1 (table)"),
        (dict(m=table(s_ne=1)), ("kr_post_spectrum_surface", "kr_reduce_spectrum_surface"), "s_ne must be >= 2"),
        (dict(R=response(thermal())), ("kr_post_response_surface", "kr_reduce_response_surface"), "the response needs the table model (spec.model == 1)"),
        (dict(R=response(nt=0)), ("kr_post_response_surface", "kr_reduce_response_surface"), "nt must be >= 1"),
        (dict(R=response(dt=0.0)), ("kr_post_response_surface", "kr_reduce_response_surface"), "dt must be positive and finite"),
        (dict(law=capi.limb_law((3, 0.0))), ("kr_post_line_surface", "kr_post_spectrum_surface", "kr_post_response_surface"),
         "limb law must be 0 (isotropic), 1 (1 + coeff mu) or 2 (log(1 + 1 / mu))"),
        (dict(law=capi.limb_law((1, NAN))), ("kr_post_line_surface", "kr_post_spectrum_surface", "kr_post_response_surface"), "non-finite limb coefficient"),
    ]
    for kw, whos, why in cases:
        calls = entry_points(lib, s, **kw)
        for who in whos:
            assert calls[who]() == capi.KR_EINVAL, (who, why)
            assert lib.kr_last_error().decode() == f"{who}: {why}", (who, why)
    # null bins, model, law
    b, m, R, law = line_bins(), table(), response(), capi.limb_law("laor")
    nulls = {"kr_post_line_surface: null bins": lambda: lib.kr_post_line_surface_dev_f64(s, *POST, None, C.byref(law), DUMMY, 4, DUMMY, None),
             "kr_reduce_line_surface: null bins": lambda: lib.kr_reduce_line_surface_dev_f64(s, None, DUMMY, 4, DUMMY, None),
             "kr_post_line_surface: null limb law": lambda: lib.kr_post_line_surface_dev_f64(s, *POST, C.byref(b), None, DUMMY, 4, DUMMY, None),
             "kr_post_spectrum_surface: null model": lambda: lib.kr_post_spectrum_surface_dev_f64(s, *POST, None, C.byref(law), DUMMY, 4, DUMMY, None),
             "kr_reduce_spectrum_surface: null model": lambda: lib.kr_reduce_spectrum_surface_dev_f64(s, None, DUMMY, 4, DUMMY, None),
             "kr_post_spectrum_surface: null limb law": lambda: lib.kr_post_spectrum_surface_dev_f64(s, *POST, C.byref(m), None, DUMMY, 4, DUMMY, None),
             "kr_post_response_surface: null model": lambda: lib.kr_post_response_surface_dev_f64(s, *POST, None, C.byref(law), DUMMY, 4, DUMMY, None),
             "kr_reduce_response_surface: null model": lambda: lib.kr_reduce_response_surface_dev_f64(s, None, DUMMY, 4, DUMMY, None),
             "kr_post_response_surface: null limb law": lambda: lib.kr_post_response_surface_dev_f64(s, *POST, C.byref(R), None, DUMMY, 4, DUMMY, None)}
    for msg, call in nulls.items():
        assert call() == capi.KR_EINVAL, msg
        assert lib.kr_last_error().decode() == msg


def test_null_pointers_and_negative_counts_are_refused(lib):
    s = C.byref(capi.disc_surface(GOOD))
    for d, n, out in ((None, 4, DUMMY), (DUMMY, 4, None), (DUMMY, -1, DUMMY)):
        for who, call in entry_points(lib, s, d=d, n=n, out=out).items():
            assert call() == capi.KR_EINVAL, (who, d, n, out)
            assert lib.kr_last_error().decode() == f"{who}: null argument or negative n", who
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(600, 7.0)
    r, o = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for rr_, n, oo in ((None, 4, o), (r, 4, None), (r, -1, o)):
        for who, call in host_entry_points(lib, s, rays=rr_, out=oo, n=n).items():
            assert call() == capi.KR_EINVAL, (who, n)
            assert lib.kr_last_error().decode() == f"{who}: null argument or negative n", who
    assert (out == 7.0).all()


def test_layouts_are_the_flat_passes(lib):
    """The line 2 nt ne + 3 words (the limb line's), the spectrum ne + 4, the response nt ne + 4: read by the api's *_from_words, word for word."""
    b = line_bins(ne=5, nt=3, dt=2.0)
    nw = api.line_words(b) + 1
    assert nw == 2 * 3 * 5 + 3
    words = np.arange(nw, dtype=np.float64)
    line = api.line_from_words(b, words[:-1])
    assert line["count"].shape == (3, 5) and line["count"][1, 2] == 7 and line["flux"][1, 2] == 15 + 7 and (line["on_disc"], line["binned"]) == (30, 31) and words[-1] == 32
    m = table(ne=6)
    words = np.arange(api.spectrum_words(m), dtype=np.float64)
    assert len(words) == 6 + 4
    spec = api.spectrum_from_words(m, words)
    assert np.array_equal(spec["flux"], np.arange(6.0)) and (spec["on_disc"], spec["used"], spec["bad_angle"]) == (6, 7, 8)
    R = response(table(ne=6), nt=4)
    words = np.arange(api.response_words(R), dtype=np.float64)
    assert len(words) == 4 * 6 + 4
    resp = api.response_from_words(R, words)
    assert resp["resp"].shape == (4, 6) and resp["resp"][2, 1] == 13 and (resp["on_disc"], resp["used"], resp["bad_angle"], resp["outside"]) == (24, 25, 26, 27)


def test_api_refuses_a_surface_with_plunge_or_pol():
    import oracle_lib as ol
    spec = ol.imageplane_spec(1000.0, 75.0, -8.0, 8.0, 0.5, -8.0, 8.0, 0.5, 0.5)
    p = api.thick_disc_params(capi.default_params(-0.5), *GOOD)
    rays = np.zeros(4, dtype=capi.RAY_F64)
    with pytest.raises(KrError, match="surface cannot be combined with V = V_PLUNGE"):
        api.line_profile(spec, p, line_bins(), V=capi.V_PLUNGE, surface=GOOD)
    with pytest.raises(KrError, match="a surface needs mode='rays'"):
        api.line_profile(spec, p, line_bins(), mode="pixels", surface=GOOD)
    with pytest.raises(KrError, match="surface cannot be combined with V = V_PLUNGE"):
        api.disc_spectrum(spec, p, table(), V=capi.V_PLUNGE, surface=GOOD)
    with pytest.raises(KrError, match="surface cannot be combined with pol"):
        api.disc_spectrum(spec, p, table(), pol="chandrasekhar", surface=GOOD)
    with pytest.raises(KrError, match="surface cannot be combined with V = V_PLUNGE"):
        api.disc_response(spec, p, response(), V=capi.V_PLUNGE, surface=capi.disc_surface(GOOD))
    with pytest.raises(KrError, match="surface cannot be combined with V = V_PLUNGE"):
        api.arrival_angles(rays, -0.5, capi.V_PLUNGE, 1, 0, surface=GOOD)


def test_text_rows_of_a_surface():
    res = {"surface": GOOD, "on_disc": 3, "used": 2, "bad_angle": 0, "energy": np.array([1.0]), "flux": np.array([2.0])}
    text = api.spectrum_text(res).splitlines()
    assert text[0] == "%20s%20.8e" % ("# DISCSLOP", 0.1) and text[1] == "%20s%20.8e" % ("# DISCSCAL", 1.0) and text[2] == "%20s%20.8e" % ("# DISCRIN", 4.233)
    assert text[3].split() == ["#", "ON_DISC", "3"] and len(text) == 7
    del res["surface"]
    assert api.spectrum_text(res).splitlines()[0].split() == ["#", "ON_DISC", "3"]
    b = line_bins(ne=2)
    line = {"surface": GOOD, "count": np.array([[1, 0]]), "flux": np.array([[0.5, 0.0]])}
    rows = api.line_text(line, b, limb=(1, 2.06)).splitlines()
    assert rows[0].split() == ["#", "DISCSLOP", "1.00000000e-01"] and rows[3].split() == ["#", "LIMB", "1"] and rows[4].split() == ["#", "LIMBCOEF", "2.06000000e+00"]
    assert rows[5].split() == ["nan", "1.05000000e+00", "5.00000000e-01", "1"] and rows[7] == "" and len(rows) == 8


def test_valid_calls_reach_the_device_check(lib):
    """Without a GPU a valid call ends in KR_ENODEVICE.  With one, only n = 0 is tried here (anything else would run kernels on the dummy pointers): KR_OK."""
    s = C.byref(capi.disc_surface(GOOD))
    if lib.kr_device_count() > 0:
        for who, call in entry_points(lib, s, d=None, n=0).items():
            assert call() == capi.KR_OK, who
        return
    for who, call in entry_points(lib, s).items():
        assert call() == capi.KR_ENODEVICE, who
        assert b"no HIP device" in lib.kr_last_error()
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(600, 7.0)
    for who, call in host_entry_points(lib, s, rays=rays.ctypes.data_as(C.c_void_p), out=out.ctypes.data_as(C.c_void_p)).items():
        assert call() == capi.KR_ENODEVICE, who
    assert (out == 7.0).all()
