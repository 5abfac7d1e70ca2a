"""CPU: the C ABI of the reverberation response (kr_response_model; kr_post_response_dev_f64, kr_reduce_response_dev_f64, kr_reduce_response_f64): the
struct's size and offsets against the header, every refusal of the model's comment with its message -- before any device is touched, so the dummy device
pointers below are never dereferenced -- and, on a machine without a GPU, KR_ENODEVICE for a valid call (there is no CPU fallback)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from raytrace_cpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
DUMMY = C.c_void_p(16)          # a "device pointer": only ever handed to calls that are refused, or made where there is no device
POST = (0.998, -1.0, 1, 0, 0, -math.pi, math.pi)
NULL_F64 = C.POINTER(C.c_double)()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def response(spec=None, t0=0.0, dt=1.0, nt=8, table_time=None, **kw):
    """A valid response model; spec: fields of its SpectrumModel to overwrite; kw: fields of the ResponseModel to overwrite."""
    m = capi.spectrum_model("table", 0.1, 0.1, 64, r_isco=1.237, r_disc=30.0, s=np.ones((2, 16)), s_e_min=0.05, s_de=1.5, table_r_min=1.2, table_dr=1.3)
    r = capi.response_model(m, t0, dt, nt, table_time=table_time)
    for k, v in (spec or {}).items():
        setattr(r.spec, k, v)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def thermal_response():
    m = capi.spectrum_model("thermal", 0.1, 0.1, 64, r_isco=1.237, r_disc=30.0, f_col=1.7, table_r_min=1.237, table_dr=1.1, table_kt=np.full(40, 0.5))
    return capi.response_model(m, 0.0, 1.0, 8)


def test_struct_size_offsets_and_abi_version(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_response_model\) == (\d+)", header).group(1))
    assert C.sizeof(capi.ResponseModel) == size == 200
    body = re.search(r"typedef struct kr_response_model \{(.*?)\} kr_response_model;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", body))
    assert [n for pair in names for n in pair if n] == ["spec", "t0", "dt", "table_time", "nt", "pad"]
    R = capi.ResponseModel
    assert (R.spec.offset, R.t0.offset, R.dt.offset, R.table_time.offset, R.nt.offset, R.pad.offset) == (0, 168, 176, 184, 192, 196)
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()                          # additive: three more entry points
    for name in ("kr_post_response_dev_f64", "kr_reduce_response_dev_f64", "kr_reduce_response_f64"):
        assert name in capi.PROTOTYPES and hasattr(lib, name)
    r = response(table_time=np.arange(5.0))
    assert (r.spec.model, r.spec.nz, r.spec.s_ne, r.nt, r.spec.table_nr) == (1, 2, 16, 8, 5) and r.table_time[4] == 4.0 and not r.spec.table_emis


REFUSALS = [
    ("null model", None, "null model"),
    # everything spectrum_validate refuses
    ("model 2", lambda: response(spec=dict(model=2)), "model must be 0 (thermal) or 1 (table)"),
    ("ne 0", lambda: response(spec=dict(ne=0)), "ne must be in 1 ... 4096"),
    ("ne 4097", lambda: response(spec=dict(ne=4097)), "ne must be in 1 ... 4096"),
    ("de 0", lambda: response(spec=dict(de=0.0)), "de must be positive"),
    ("log_e de 1", lambda: response(spec=dict(log_e=1, de=1.0)), "log_e: de (the ratio between edges) must be > 1"),
    ("log_e e_min 0", lambda: response(spec=dict(log_e=1, de=1.1, e_min=0.0)), "log_e: e_min must be positive"),
    ("nan e_min", lambda: response(spec=dict(e_min=NAN)), "non-finite model parameter"),
    ("inf r_disc", lambda: response(spec=dict(r_disc=INF)), "non-finite model parameter"),
    ("nan q2", lambda: response(spec=dict(q2=NAN)), "non-finite model parameter"),
    ("no s", lambda: response(spec=dict(s=NULL_F64)), "the table model needs s"),
    ("s_ne 1", lambda: response(spec=dict(s_ne=1)), "s_ne must be >= 2"),
    ("s_de 1", lambda: response(spec=dict(s_de=1.0)), "s_de (the ratio between nodes) must be > 1"),
    ("s_e_min 0", lambda: response(spec=dict(s_e_min=0.0)), "s_e_min must be positive"),
    ("nz 0", lambda: response(spec=dict(nz=0)), "nz must be >= 1"),
    ("nz s_ne too large", lambda: response(spec=dict(nz=1025, s_ne=1024)), "nz * s_ne must not exceed 2^20"),
    ("table_emis table_nr 0", lambda: response(spec=dict(table_emis=np.ones(8).ctypes.data_as(C.POINTER(C.c_double)), table_nr=0)), "table_nr must be >= 1 with a table"),
    # the response's own
    ("thermal", thermal_response, "the response needs the table model (spec.model == 1)"),
    ("nt 0", lambda: response(nt=0), "nt must be >= 1"),
    ("nt negative", lambda: response(nt=-3), "nt must be >= 1"),
    ("dt 0", lambda: response(dt=0.0), "dt must be positive and finite"),
    ("dt negative", lambda: response(dt=-1.0), "dt must be positive and finite"),
    ("dt nan", lambda: response(dt=NAN), "dt must be positive and finite"),
    ("dt inf", lambda: response(dt=INF), "dt must be positive and finite"),
    ("t0 nan", lambda: response(t0=NAN), "non-finite t0"),
    ("t0 inf", lambda: response(t0=-INF), "non-finite t0"),
    ("nt ne too large", lambda: response(nt=(1 << 18) + 1), "nt * ne must not exceed 2^24"),
    ("table_time table_nr 0", lambda: response(table_time=np.ones(8), spec=dict(table_nr=0)), "table_nr must be >= 1 with a table"),
    ("table_time nan table_dr", lambda: response(table_time=np.ones(8), spec=dict(table_dr=NAN)), "non-finite model parameter"),
]


@pytest.mark.parametrize("label,make,why", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_models_are_refused_before_any_device_work(lib, label, make, why):
    r = make() if make else None
    ref = C.byref(r) if r is not None else None
    law = capi.limb_law("isotropic")
    out = np.full(4100, 7.0)
    rays = np.zeros(4, dtype=capi.RAY_F64)
    calls = {"kr_post_response": lambda: lib.kr_post_response_dev_f64(*POST, ref, C.byref(law), DUMMY, 4, DUMMY, None),
             "kr_reduce_response": lambda: lib.kr_reduce_response_dev_f64(ref, DUMMY, 4, DUMMY, None)}
    for who, call in calls.items():
        assert call() == capi.KR_EINVAL, (who, label)
        assert lib.kr_last_error().decode() == f"{who}: {why}", (who, label)
    assert lib.kr_reduce_response_f64(ref, rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == f"kr_reduce_response: {why}"
    assert (out == 7.0).all()                                                       # a refused call writes nothing


def test_bad_laws_pointers_and_counts_are_refused(lib):
    r, iso = response(), capi.limb_law("isotropic")
    for law in (None, C.byref(capi.limb_law((3, 0.0)))):
        assert lib.kr_post_response_dev_f64(*POST, C.byref(r), law, DUMMY, 4, DUMMY, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode().startswith("kr_post_response: ")
    moving = (0.998, -1.0, 1, 0, 1, -math.pi, math.pi)
    assert lib.kr_post_response_dev_f64(*moving, C.byref(r), C.byref(capi.limb_law("laor")), DUMMY, 4, DUMMY, None) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == "kr_post_response: motion != 0 needs limb law 0 (only the orbiting observer has the frame of mu)"
    for args in ((C.byref(iso), None, 4, DUMMY), (C.byref(iso), DUMMY, 4, None), (C.byref(iso), DUMMY, -1, DUMMY)):
        assert lib.kr_post_response_dev_f64(*POST, C.byref(r), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_post_response: null argument or negative n"
    for args in ((None, 4, DUMMY), (DUMMY, 4, None), (DUMMY, -1, DUMMY)):
        assert lib.kr_reduce_response_dev_f64(C.byref(r), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_response: null argument or negative n"
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(8 * 64 + 4, 7.0)
    p, o = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((None, 4, o), (p, 4, None), (p, -1, o)):
        assert lib.kr_reduce_response_f64(C.byref(r), *args) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_response: null argument or negative n"
    assert (out == 7.0).all()


@pytest.mark.parametrize("make", [response, lambda: response(table_time=np.ones(8)),
                                  lambda: response(table_time=np.ones(8), spec=dict(table_emis=np.ones(8).ctypes.data_as(C.POINTER(C.c_double)))),
                                  lambda: response(nt=1 << 18)], ids=["plain", "time", "emis+time", "largest"])
def test_valid_models_reach_the_device_check(lib, make):
    """Without a GPU a valid call ends in KR_ENODEVICE.  With one, only n = 0 is tried here (anything else would run kernels on the dummy pointers): KR_OK."""
    r, law = make(), capi.limb_law("laor")
    if lib.kr_device_count() > 0:
        assert lib.kr_post_response_dev_f64(*POST, C.byref(r), C.byref(law), None, 0, DUMMY, None) == capi.KR_OK
        assert lib.kr_reduce_response_dev_f64(C.byref(r), None, 0, DUMMY, None) == capi.KR_OK
        return
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(16, 7.0)
    assert lib.kr_post_response_dev_f64(*POST, C.byref(r), C.byref(law), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert b"no HIP device" in lib.kr_last_error()
    assert lib.kr_reduce_response_dev_f64(C.byref(r), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert lib.kr_reduce_response_f64(C.byref(r), rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_ENODEVICE
    assert (out[:16] == 7.0).all()
