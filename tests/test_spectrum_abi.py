"""CPU: the C ABI of the continuum spectrum (kr_spectrum_model; kr_post_spectrum_dev_f64, kr_reduce_spectrum_dev_f64, kr_reduce_spectrum_f64): the
struct's size against the header's static_assert, every refusal of the model's comment with its message -- before any device is touched, so the dummy
device pointers below are never dereferenced -- and, on a machine without a GPU, KR_ENODEVICE for a valid call (there is no CPU fallback)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from raytrace_cpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
DUMMY = C.c_void_p(16)          # a "device pointer": only ever handed to calls that are refused, or made where there is no device
POST = (0.998, -1.0, 1, 0, 0, -math.pi, math.pi)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def thermal(**kw):
    m = capi.spectrum_model("thermal", 0.1, 0.1, 64, r_isco=1.237, r_disc=30.0, f_col=1.7, table_r_min=1.237, table_dr=1.1, table_kt=np.full(40, 0.5))
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def table(**kw):
    m = capi.spectrum_model("table", 0.1, 0.1, 64, r_isco=1.237, r_disc=30.0, s=np.ones((2, 16)), s_e_min=0.05, s_de=1.5)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_struct_size_and_abi_version(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_spectrum_model\) == (\d+)", header).group(1))
    assert C.sizeof(capi.SpectrumModel) == size == 168
    assert capi.SpectrumModel.table_kt.offset == 112 and capi.SpectrumModel.model.offset == 136 and capi.SpectrumModel.nz.offset == 160
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()                          # additive: three more entry points
    for name in ("kr_post_spectrum_dev_f64", "kr_reduce_spectrum_dev_f64", "kr_reduce_spectrum_f64"):
        assert name in capi.PROTOTYPES and hasattr(lib, name)
    m = capi.spectrum_model("table", 1.0, 1.1, 8, log_e=True, s=np.ones(5), s_e_min=0.5, s_de=2.0)
    assert (m.model, m.nz, m.s_ne, m.log_e, m.table_nr) == (1, 1, 5, 1, 0) and not m.table_kt and not m.table_emis


NULL_F64 = C.POINTER(C.c_double)()
REFUSALS = [
    ("null model", None, "null model"),
    ("model 2", lambda: thermal(model=2), "model must be 0 (thermal) or 1 (table)"),
    ("model -1", lambda: table(model=-1), "model must be 0 (thermal) or 1 (table)"),
    ("ne 0", lambda: thermal(ne=0), "ne must be in 1 ... 4096"),
    ("ne 4097", lambda: table(ne=4097), "ne must be in 1 ... 4096"),
    ("de 0", lambda: thermal(de=0.0), "de must be positive"),
    ("de negative", lambda: table(de=-0.1), "de must be positive"),
    ("log_e de 1", lambda: thermal(log_e=1, de=1.0), "log_e: de (the ratio between edges) must be > 1"),
    ("log_e e_min 0", lambda: thermal(log_e=1, de=1.1, e_min=0.0), "log_e: e_min must be positive"),
    ("nan e_min", lambda: thermal(e_min=NAN), "non-finite model parameter"),
    ("inf r_disc", lambda: table(r_disc=float("inf")), "non-finite model parameter"),
    ("nan f_col", lambda: thermal(f_col=NAN), "non-finite model parameter"),
    ("nan q2", lambda: table(q2=NAN), "non-finite model parameter"),
    ("nan s_de", lambda: table(s_de=NAN), "non-finite model parameter"),
    ("nan table_dr", lambda: thermal(table_dr=NAN), "non-finite model parameter"),
    ("no table_kt", lambda: thermal(table_kt=NULL_F64), "the thermal model needs table_kt"),
    ("f_col 0", lambda: thermal(f_col=0.0), "f_col must be positive"),
    ("f_col negative", lambda: thermal(f_col=-1.0), "f_col must be positive"),
    ("table_nr 0", lambda: thermal(table_nr=0), "table_nr must be >= 1 with a table"),
    ("no s", lambda: table(s=NULL_F64), "the table model needs s"),
    ("s_ne 1", lambda: table(s_ne=1), "s_ne must be >= 2"),
    ("s_de 1", lambda: table(s_de=1.0), "s_de (the ratio between nodes) must be > 1"),
    ("s_e_min 0", lambda: table(s_e_min=0.0), "s_e_min must be positive"),
    ("nz 0", lambda: table(nz=0), "nz must be >= 1"),
    ("nz s_ne too large", lambda: table(nz=1025, s_ne=1024), "nz * s_ne must not exceed 2^20"),
]


@pytest.mark.parametrize("label,make,why", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_models_are_refused_before_any_device_work(lib, label, make, why):
    m = make() if make else None
    ref = C.byref(m) if m is not None else None
    law = capi.limb_law("isotropic")
    out = np.full(4100, 7.0)
    rays = np.zeros(4, dtype=capi.RAY_F64)
    calls = {"kr_post_spectrum": lambda: lib.kr_post_spectrum_dev_f64(*POST, ref, C.byref(law), DUMMY, 4, DUMMY, None),
             "kr_reduce_spectrum": lambda: lib.kr_reduce_spectrum_dev_f64(ref, DUMMY, 4, DUMMY, None)}
    for who, call in calls.items():
        assert call() == capi.KR_EINVAL, (who, label)
        assert lib.kr_last_error().decode() == f"{who}: {why}", (who, label)
    assert lib.kr_reduce_spectrum_f64(ref, rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == f"kr_reduce_spectrum: {why}"
    assert (out == 7.0).all()                                                       # a refused call writes nothing


def test_bad_laws_pointers_and_counts_are_refused(lib):
    m, iso = thermal(), capi.limb_law("isotropic")
    cases = [(lambda: lib.kr_post_spectrum_dev_f64(*POST, C.byref(m), None, DUMMY, 4, DUMMY, None), "kr_post_spectrum: "),
             (lambda: lib.kr_post_spectrum_dev_f64(*POST, C.byref(m), C.byref(capi.limb_law((3, 0.0))), DUMMY, 4, DUMMY, None), "kr_post_spectrum: ")]
    for call, prefix in cases:
        assert call() == capi.KR_EINVAL and lib.kr_last_error().decode().startswith(prefix)
    moving = (0.998, -1.0, 1, 0, 1, -math.pi, math.pi)
    assert lib.kr_post_spectrum_dev_f64(*moving, C.byref(m), C.byref(capi.limb_law("laor")), DUMMY, 4, DUMMY, None) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == "kr_post_spectrum: motion != 0 needs limb law 0 (only the orbiting observer has the frame of mu)"
    for args in ((C.byref(iso), None, 4, DUMMY), (C.byref(iso), DUMMY, 4, None), (C.byref(iso), DUMMY, -1, DUMMY)):
        assert lib.kr_post_spectrum_dev_f64(*POST, C.byref(m), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_post_spectrum: null argument or negative n"
    for args in ((None, 4, DUMMY), (DUMMY, 4, None), (DUMMY, -1, DUMMY)):
        assert lib.kr_reduce_spectrum_dev_f64(C.byref(m), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_spectrum: null argument or negative n"
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.zeros(68)
    r, o = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((None, 4, o), (r, 4, None), (r, -1, o)):
        assert lib.kr_reduce_spectrum_f64(C.byref(m), *args) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_spectrum: null argument or negative n"


@pytest.mark.parametrize("make", [thermal, table, lambda: table(table_emis=np.ones(8).ctypes.data_as(C.POINTER(C.c_double)), table_nr=8, table_r_min=1.2, table_dr=1.3)],
                         ids=["thermal", "table", "table+emis"])
def test_valid_models_reach_the_device_check(lib, make):
    """Without a GPU a valid call ends in KR_ENODEVICE.  With one, only n = 0 is tried here (anything else would run kernels on the dummy pointers): KR_OK."""
    m, law = make(), capi.limb_law("laor")
    if lib.kr_device_count() > 0:
        assert lib.kr_post_spectrum_dev_f64(*POST, C.byref(m), C.byref(law), None, 0, DUMMY, None) == capi.KR_OK
        assert lib.kr_reduce_spectrum_dev_f64(C.byref(m), None, 0, DUMMY, None) == capi.KR_OK
        return
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(68, 7.0)
    assert lib.kr_post_spectrum_dev_f64(*POST, C.byref(m), C.byref(law), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert b"no HIP device" in lib.kr_last_error()
    assert lib.kr_reduce_spectrum_dev_f64(C.byref(m), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert lib.kr_reduce_spectrum_f64(C.byref(m), rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_ENODEVICE
    assert (out == 7.0).all()
