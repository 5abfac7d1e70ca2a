"""CPU: the C ABI of the (r, phi) illumination map (kr_illum_bins; kr_post_illum_dev_f64, kr_reduce_illum_dev_f64, kr_reduce_illum_f64): the struct's
size and offsets against the header and against a compiled C snippet, every refusal of the struct's comment with its message -- before any device is
touched, so the dummy device pointers below are never dereferenced -- n == 0, and, on a machine without a GPU, KR_ENODEVICE for a valid call (there is
no CPU fallback)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
DUMMY = C.c_void_p(16)          # a "device pointer": only ever handed to calls that are refused, or made where there is no device
POST = (0.9, -1.0, 0, 0, 0, -math.pi, math.pi)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def bins(nr=12, nphi=16, phi_shift=0.0137, **rad):
    b = capi.EmisBins()
    b.r_min, b.dr, b.r_isco, b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = 1.2, 1.3, 2.32, 2.0, 0.9, 1e4, nr, 1
    for k, v in rad.items():
        setattr(b, k, v)
    return capi.illum_bins(b, nphi, phi_shift)


def test_struct_size_offsets_and_abi_version(lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_illum_bins\) == (\d+)", header).group(1))
    assert C.sizeof(capi.IllumBins) == size == 72
    body = re.search(r"typedef struct kr_illum_bins \{(.*?)\} kr_illum_bins;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", body))
    assert [n for pair in names for n in pair if n] == ["rad", "phi_shift", "nphi", "pad"]
    S = capi.IllumBins
    offsets = [getattr(S, n).offset for n in ("rad", "phi_shift", "nphi", "pad")]
    assert offsets == [0, 56, 64, 68] and C.sizeof(capi.EmisBins) == 56
    # the same from the C compiler's side of the header
    src = tmp_path / "illum_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kr_trace.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(kr_illum_bins), '
                   'offsetof(kr_illum_bins, rad), offsetof(kr_illum_bins, phi_shift), offsetof(kr_illum_bins, nphi), offsetof(kr_illum_bins, pad)); return 0; }\n')
    exe = tmp_path / "illum_layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [size] + offsets
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()                          # additive: three more entry points
    for name in ("kr_post_illum_dev_f64", "kr_reduce_illum_dev_f64", "kr_reduce_illum_f64"):
        assert name in capi.PROTOTYPES and hasattr(lib, name)
    m = bins()
    assert (m.rad.nr, m.nphi, m.phi_shift, m.rad.r_isco, m.rad.logbin, m.pad) == (12, 16, 0.0137, 2.32, 1, 0)
    assert api.illum_words(m) == 5 * 12 * 16 + 2


REFUSALS = [
    ("null bins", None, "null bins"),
    ("nr 0", lambda: bins(nr=0), "nr must be positive"),
    ("nr negative", lambda: bins(nr=-3), "nr must be positive"),
    ("nphi 0", lambda: bins(nphi=0), "nphi must be positive"),
    ("nphi negative", lambda: bins(nphi=-16), "nphi must be positive"),
    ("too many cells", lambda: bins(nr=1024, nphi=1025), "nr * nphi must not exceed 2^20"),
    ("too many cells, one ring", lambda: bins(nr=1, nphi=(1 << 20) + 1), "nr * nphi must not exceed 2^20"),
    ("too many cells, int overflow", lambda: bins(nr=2 ** 31 - 1, nphi=2 ** 31 - 1), "nr * nphi must not exceed 2^20"),
    ("phi_shift nan", lambda: bins(phi_shift=NAN), "phi_shift must be finite"),
    ("phi_shift inf", lambda: bins(phi_shift=INF), "phi_shift must be finite"),
    ("phi_shift -inf", lambda: bins(phi_shift=-INF), "phi_shift must be finite"),
]


@pytest.mark.parametrize("label,make,why", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_bins_are_refused_before_any_device_work(lib, label, make, why):
    m = make() if make else None
    ref = C.byref(m) if m is not None else None
    out = np.full(1024, 7.0)
    rays = np.zeros(4, dtype=capi.RAY_F64)
    calls = {"kr_post_illum": lambda: lib.kr_post_illum_dev_f64(*POST, ref, DUMMY, 4, DUMMY, None),
             "kr_reduce_illum": lambda: lib.kr_reduce_illum_dev_f64(ref, DUMMY, 4, DUMMY, None)}
    for who, call in calls.items():
        assert call() == capi.KR_EINVAL, (who, label)
        assert lib.kr_last_error().decode() == f"{who}: {why}", (who, label)
    assert lib.kr_reduce_illum_f64(ref, rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == f"kr_reduce_illum: {why}"
    assert (out == 7.0).all()                                                       # a refused call writes nothing
    if m is not None:
        with pytest.raises(capi.KrError, match=re.escape(why)):
            api.reduce_illum(m, rays)


def test_bad_pointers_counts_and_the_plunging_flow_are_refused(lib):
    m = bins()
    for args in ((None, 4, DUMMY), (DUMMY, 4, None), (DUMMY, -1, DUMMY)):
        assert lib.kr_post_illum_dev_f64(*POST, C.byref(m), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_post_illum: null argument or negative n"
        assert lib.kr_reduce_illum_dev_f64(C.byref(m), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_illum: null argument or negative n"
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(5 * 12 * 16 + 2, 7.0)
    p, o = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((None, 4, o), (p, 4, None), (p, -1, o)):
        assert lib.kr_reduce_illum_f64(C.byref(m), *args) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_illum: null argument or negative n"
    assert (out == 7.0).all()
    plunge = (0.9, capi.V_PLUNGE, 0, 0, 0, -math.pi, math.pi)
    assert lib.kr_post_illum_dev_f64(*plunge, C.byref(m), DUMMY, 4, DUMMY, None) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == "kr_post_illum: V = KR_V_PLUNGE (the plunging disc flow) is not supported here"


@pytest.mark.parametrize("make", [bins, lambda: bins(nr=1, nphi=1), lambda: bins(nr=1024, nphi=1024), lambda: bins(nr=1, nphi=1 << 20),
                                  lambda: bins(r_min=-1.0, dr=0.0), lambda: bins(phi_shift=-12389.0)],
                         ids=["plain", "one cell", "largest", "one ring", "quotients that bin nothing", "a large shift"])
def test_valid_bins_reach_the_device_check(lib, make):
    """Without a GPU a valid call ends in KR_ENODEVICE.  With one, only n = 0 is tried here (anything else would run kernels on the dummy pointers): KR_OK,
    and nothing is added."""
    m = make()
    if lib.kr_device_count() > 0:
        assert lib.kr_post_illum_dev_f64(*POST, C.byref(m), None, 0, DUMMY, None) == capi.KR_OK
        assert lib.kr_reduce_illum_dev_f64(C.byref(m), None, 0, DUMMY, None) == capi.KR_OK
        return
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(16, 7.0)
    assert lib.kr_post_illum_dev_f64(*POST, C.byref(m), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert b"no HIP device" in lib.kr_last_error()
    assert lib.kr_reduce_illum_dev_f64(C.byref(m), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert lib.kr_reduce_illum_f64(C.byref(m), rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_ENODEVICE
    assert (out == 7.0).all()


def test_the_api_refuses_what_it_can_see_without_a_device():
    with pytest.raises(capi.KrError, match="PointSourceSpec, a PointSourceVelSpec or a HealpixSource"):
        api.illumination_map(object(), capi.default_params(0.9), bins())


# ---- kr_illum_table and the six entry points that take it -------------------------------------------------------------------------------------
def table(time=True, shape=(3, 4), **kw):
    """A valid 3 x 4 table; kw: fields to overwrite (a refused call never reads the planes)."""
    t = capi.illum_table(np.ones(shape), 1.3, 1.5, logbin=True, time=np.full(shape, 2.0) if time else None, phi_shift=0.0137)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def line(**kw):
    b = capi.line_bins(e_min=1.0, de=0.1, ne=20, t0=0.0, dt=1.0, nt=4, r_isco=1.3, r_disc=30.0)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def response(**kw):
    spec = capi.spectrum_model("table", 0.5, 1.2, 8, log_e=True, r_isco=1.3, r_disc=30.0, s=np.ones((1, 4)), s_e_min=0.05, s_de=1.5)
    return capi.response_model(spec, 0.0, 1.0, 4, **kw)


def table_calls(lib, b, law, r, t):
    """who -> call of every entry point that takes a table, on dummy device pointers / four host records"""
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(256, 7.0)
    hp, ho = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    ref = lambda x: C.byref(x) if x is not None else None      # noqa: E731
    return out, {
        "kr_post_line_illum": lambda V=-1.0: lib.kr_post_line_illum_dev_f64(0.9, V, 1, 0, 0, -math.pi, math.pi, ref(b), ref(law), ref(t), DUMMY, 4, DUMMY, None),
        "kr_reduce_line_illum": lambda V=-1.0: lib.kr_reduce_line_illum_dev_f64(ref(b), ref(t), DUMMY, 4, DUMMY, None),
        "kr_reduce_line_illum host": lambda V=-1.0: lib.kr_reduce_line_illum_f64(ref(b), ref(t), hp, 4, ho),
        "kr_post_response_illum": lambda V=-1.0: lib.kr_post_response_illum_dev_f64(0.9, V, 1, 0, 0, -math.pi, math.pi, ref(r), ref(law), ref(t), DUMMY, 4, DUMMY, None),
        "kr_reduce_response_illum": lambda V=-1.0: lib.kr_reduce_response_illum_dev_f64(ref(r), ref(t), DUMMY, 4, DUMMY, None),
        "kr_reduce_response_illum host": lambda V=-1.0: lib.kr_reduce_response_illum_f64(ref(r), ref(t), hp, 4, ho),
    }


def test_table_struct_size_and_offsets(lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_illum_table\) == (\d+)", header).group(1))
    assert C.sizeof(capi.IllumTable) == size == 56              # three doubles, two pointers, four int32
    S = capi.IllumTable
    names = ("r_min", "dr", "phi_shift", "emis", "time", "nr", "nphi", "logbin", "pad")
    offsets = [getattr(S, n).offset for n in names]
    assert offsets == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    src = tmp_path / "table_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kr_trace.h"\nint main(void) { printf("%zu", sizeof(kr_illum_table));\n'
                   + "".join(f'printf(" %zu", offsetof(kr_illum_table, {n}));\n' for n in names) + 'return 0; }\n')
    exe = tmp_path / "table_layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [size] + offsets
    for name in ("kr_post_line_illum_dev_f64", "kr_reduce_line_illum_dev_f64", "kr_reduce_line_illum_f64", "kr_post_response_illum_dev_f64",
                 "kr_reduce_response_illum_dev_f64", "kr_reduce_response_illum_f64"):
        assert name in capi.PROTOTYPES and hasattr(lib, name)
    t = table()
    assert (t.nr, t.nphi, t.logbin, t.r_min, t.dr, t.phi_shift) == (3, 4, 1, 1.3, 1.5, 0.0137) and t.emis[11] == 1.0 and t.time[0] == 2.0
    d = {"emis": np.ones((2, 5)), "time": None, "r_min": 1.0, "dr": 2.0, "logbin": 0, "phi_shift": 0.25}
    t = capi.illum_table(d)
    assert (t.nr, t.nphi, t.logbin, t.phi_shift) == (2, 5, 0, 0.25) and not t.time and capi.illum_table(d, phi_shift=-1.0).phi_shift == -1.0


TABLE_REFUSALS = [
    ("null table", lambda: None, "null table"),
    ("no emis", lambda: table(emis=None), "the table needs emis"),
    ("nr 0", lambda: table(nr=0), "table nr must be positive"),
    ("nphi 0", lambda: table(nphi=0), "table nphi must be positive"),
    ("nphi negative", lambda: table(nphi=-4), "table nphi must be positive"),
    ("too many cells", lambda: table(nr=1 << 10, nphi=(1 << 10) + 1), "table nr * nphi must not exceed 2^20"),
    ("r_min nan", lambda: table(r_min=NAN), "non-finite table r_min, dr or phi_shift"),
    ("dr inf", lambda: table(dr=INF), "non-finite table r_min, dr or phi_shift"),
    ("phi_shift nan", lambda: table(phi_shift=NAN), "non-finite table r_min, dr or phi_shift"),
    ("phi_shift inf", lambda: table(phi_shift=-INF), "non-finite table r_min, dr or phi_shift"),
]


@pytest.mark.parametrize("label,make,why", TABLE_REFUSALS, ids=[r[0] for r in TABLE_REFUSALS])
def test_bad_tables_are_refused_before_any_device_work(lib, label, make, why):
    out, calls = table_calls(lib, line(), capi.limb_law("isotropic"), response(), make())
    for who, call in calls.items():
        assert call() == capi.KR_EINVAL, (who, label)
        assert lib.kr_last_error().decode() == f"{who.split()[0]}: {why}", (who, label)
    assert (out == 7.0).all()


def test_what_the_twin_refuses_a_second_table_and_the_plunging_flow_are_refused(lib):
    iso, t = capi.limb_law("isotropic"), table()
    # what the flat twin refuses: bad bins, a bad model, a bad law
    out, calls = table_calls(lib, line(ne=0), iso, response(), t)
    for who in ("kr_post_line_illum", "kr_reduce_line_illum", "kr_reduce_line_illum host"):
        assert calls[who]() == capi.KR_EINVAL and lib.kr_last_error().decode() == f"{who.split()[0]}: ne and nt must be >= 1"
    bad_r = response()
    bad_r.nt = 0
    out, calls = table_calls(lib, line(), iso, bad_r, t)
    for who in ("kr_post_response_illum", "kr_reduce_response_illum", "kr_reduce_response_illum host"):
        assert calls[who]() == capi.KR_EINVAL and lib.kr_last_error().decode() == f"{who.split()[0]}: nt must be >= 1"
    out, calls = table_calls(lib, line(), capi.limb_law((7, 0.0)), response(), t)
    for who in ("kr_post_line_illum", "kr_post_response_illum"):
        assert calls[who]() == capi.KR_EINVAL and who in lib.kr_last_error().decode()
    out, calls = table_calls(lib, None, iso, None, t)
    for who, call in calls.items():
        assert call() == capi.KR_EINVAL and lib.kr_last_error().decode().startswith(who.split()[0] + ": null")
    # bins / a model with a radial table of their own
    flat = line().with_table(1.3, 1.5, np.ones(5), np.ones(5))
    spec = capi.spectrum_model("table", 0.5, 1.2, 8, log_e=True, r_isco=1.3, r_disc=30.0, s=np.ones((1, 4)), s_e_min=0.05, s_de=1.5, table_emis=np.ones(5), table_r_min=1.3,
                               table_dr=1.5)
    for r in (capi.response_model(spec, 0.0, 1.0, 4), capi.response_model(spec, 0.0, 1.0, 4, table_time=np.ones(5))):
        out, calls = table_calls(lib, flat, iso, r, t)
        for who, call in calls.items():
            what = "bins carry" if "line" in who else "model carries"
            assert call() == capi.KR_EINVAL and lib.kr_last_error().decode() == f"{who.split()[0]}: the {what} a radial table as well as the (r, phi) table", who
    time_only = response(table_time=np.ones(5))
    time_only.spec.table_r_min, time_only.spec.table_dr = 1.3, 1.5
    out, calls = table_calls(lib, line(), iso, time_only, t)
    assert calls["kr_reduce_response_illum"]() == capi.KR_EINVAL and "model carries a radial table" in lib.kr_last_error().decode()
    # the plunging flow
    out, calls = table_calls(lib, line(), iso, response(), t)
    for who in ("kr_post_line_illum", "kr_post_response_illum"):
        assert calls[who](capi.V_PLUNGE) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == f"{who}: V = KR_V_PLUNGE (the plunging disc flow) is not supported here"
    # pointers and counts
    b, r = line(), response()
    for args in ((None, 4, DUMMY), (DUMMY, 4, None), (DUMMY, -1, DUMMY)):
        assert lib.kr_reduce_line_illum_dev_f64(C.byref(b), C.byref(t), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_line_illum: null argument or negative n"
        assert lib.kr_reduce_response_illum_dev_f64(C.byref(r), C.byref(t), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_response_illum: null argument or negative n"
        assert lib.kr_post_line_illum_dev_f64(0.9, -1.0, 1, 0, 0, -math.pi, math.pi, C.byref(b), C.byref(iso), C.byref(t), *args, None) == capi.KR_EINVAL
        assert lib.kr_post_response_illum_dev_f64(0.9, -1.0, 1, 0, 0, -math.pi, math.pi, C.byref(r), C.byref(iso), C.byref(t), *args, None) == capi.KR_EINVAL
    assert (out == 7.0).all()


@pytest.mark.parametrize("make", [table, lambda: table(time=False), lambda: table(shape=(1, 1)), lambda: table(logbin=0, dr=0.0)],
                         ids=["plain", "no time", "one cell", "a quotient that finds no ring"])
def test_valid_tables_reach_the_device_check(lib, make):
    out, calls = table_calls(lib, line(), capi.limb_law("laor"), response(), make())
    if lib.kr_device_count() > 0:
        t, b, r = make(), line(), response()
        assert lib.kr_reduce_line_illum_dev_f64(C.byref(b), C.byref(t), None, 0, DUMMY, None) == capi.KR_OK
        assert lib.kr_reduce_response_illum_dev_f64(C.byref(r), C.byref(t), None, 0, DUMMY, None) == capi.KR_OK
        return
    for who, call in calls.items():
        assert call() == capi.KR_ENODEVICE, who
        assert b"no HIP device" in lib.kr_last_error()
    assert (out == 7.0).all()


def test_the_api_refuses_illum_with_a_surface_pol_or_the_plunging_flow():
    tab = {"emis": np.ones((2, 3)), "time": None, "r_min": 1.3, "dr": 1.5, "logbin": 1, "phi_shift": 0.0}
    plane, p = capi.ImagePlaneSpec(), capi.default_params(-0.9)
    for kw in (dict(surface=(1.3, 0.0, 0.05, 0.0)), dict(V=capi.V_PLUNGE)):
        with pytest.raises(capi.KrError, match="illum cannot be combined"):
            api.line_profile(plane, p, line(), illum=tab, **kw)
        with pytest.raises(capi.KrError, match="illum cannot be combined"):
            api.disc_response(plane, p, response(), illum=tab, **kw)
    with pytest.raises(capi.KrError, match="illum needs mode='rays'"):
        api.line_profile(plane, p, line(), illum=tab, mode="pixels")
