"""CPU: the C ABI of the source-to-observer link (kr_observer_spec; kr_post_observer_dev_f64, kr_reduce_observer_dev_f64, kr_reduce_observer_f64): the
struct's size and offsets against the header, every refusal of the spec's comment with its message -- before any device is touched, so the dummy device
pointers below are never dereferenced -- n == 0, and, on a machine without a GPU, KR_ENODEVICE for a valid call (there is no CPU fallback)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
DUMMY = C.c_void_p(16)          # a "device pointer": only ever handed to calls that are refused, or made where there is no device
POST = (0.998, -1.0, 0, 0, 0, -math.pi, math.pi)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def observer(**kw):
    """A valid spec; kw: fields to overwrite."""
    sp = api.observer_spec(0.998, 1.237, 400.0, 1000.0, nmu=20, gamma=2.0, dist=1000.0, t0=990.0, dt=0.5, nt=64)
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def test_struct_size_offsets_and_abi_version(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_observer_spec\) == (\d+)", header).group(1))
    assert C.sizeof(capi.ObserverSpec) == size == 120
    body = re.search(r"typedef struct kr_observer_spec \{(.*?)\} kr_observer_spec;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", body))
    assert [n for pair in names for n in pair if n] == ["cls", "spin", "mu0", "dmu", "t0", "dt", "dist", "gamma", "nmu", "nt"]
    S = capi.ObserverSpec
    assert [getattr(S, n).offset for n in ("cls", "spin", "mu0", "dmu", "t0", "dt", "dist", "gamma", "nmu", "nt")] == [0, 56, 64, 72, 80, 88, 96, 104, 112, 116]
    assert C.sizeof(capi.ReturnBins) == 56
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()                          # additive: three more entry points
    for name in ("kr_post_observer_dev_f64", "kr_reduce_observer_dev_f64", "kr_reduce_observer_f64"):
        assert name in capi.PROTOTYPES and hasattr(lib, name)
    sp = observer()
    assert (sp.nmu, sp.nt, sp.dmu, sp.cls.source_r, sp.cls.r_esc, sp.spin) == (20, 64, 0.05, 0.0, 1000.0, 0.998)


REFUSALS = [
    ("null spec", None, "null spec"),
    ("nmu 0", lambda: observer(nmu=0), "nmu must be in 1 ... 4096"),
    ("nmu negative", lambda: observer(nmu=-4), "nmu must be in 1 ... 4096"),
    ("nmu 4097", lambda: observer(nmu=4097), "nmu must be in 1 ... 4096"),
    ("nt negative", lambda: observer(nt=-1), "nt must be >= 0"),
    ("too many words", lambda: observer(nmu=4096, nt=4093), "nmu * (4 + nt) must not exceed 2^24"),
    ("too many words, int overflow", lambda: observer(nmu=4096, nt=2 ** 31 - 1), "nmu * (4 + nt) must not exceed 2^24"),
    ("dmu 0", lambda: observer(dmu=0.0), "dmu must be positive and finite"),
    ("dmu negative", lambda: observer(dmu=-0.1), "dmu must be positive and finite"),
    ("dmu nan", lambda: observer(dmu=NAN), "dmu must be positive and finite"),
    ("dmu inf", lambda: observer(dmu=INF), "dmu must be positive and finite"),
    ("dt 0", lambda: observer(dt=0.0), "dt must be positive and finite"),
    ("dt negative", lambda: observer(dt=-1.0), "dt must be positive and finite"),
    ("dt nan", lambda: observer(dt=NAN), "dt must be positive and finite"),
    ("dt inf", lambda: observer(dt=INF), "dt must be positive and finite"),
    ("mu0 nan", lambda: observer(mu0=NAN), "non-finite mu0, t0, gamma or spin"),
    ("mu0 inf", lambda: observer(mu0=-INF), "non-finite mu0, t0, gamma or spin"),
    ("t0 nan", lambda: observer(t0=NAN), "non-finite mu0, t0, gamma or spin"),
    ("t0 inf", lambda: observer(t0=INF), "non-finite mu0, t0, gamma or spin"),
    ("gamma nan", lambda: observer(gamma=NAN), "non-finite mu0, t0, gamma or spin"),
    ("gamma inf", lambda: observer(gamma=INF), "non-finite mu0, t0, gamma or spin"),
    ("spin nan", lambda: observer(spin=NAN), "non-finite mu0, t0, gamma or spin"),
    ("dist negative", lambda: observer(dist=-1.0), "dist must be >= 0 and finite"),
    ("dist nan", lambda: observer(dist=NAN), "dist must be >= 0 and finite"),
    ("dist inf", lambda: observer(dist=INF), "dist must be >= 0 and finite"),
]


@pytest.mark.parametrize("label,make,why", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_specs_are_refused_before_any_device_work(lib, label, make, why):
    sp = make() if make else None
    ref = C.byref(sp) if sp is not None else None
    out = np.full(4100, 7.0)
    rays = np.zeros(4, dtype=capi.RAY_F64)
    calls = {"kr_post_observer": lambda: lib.kr_post_observer_dev_f64(*POST, ref, DUMMY, 4, DUMMY, None),
             "kr_reduce_observer": lambda: lib.kr_reduce_observer_dev_f64(ref, DUMMY, 4, DUMMY, None)}
    for who, call in calls.items():
        assert call() == capi.KR_EINVAL, (who, label)
        assert lib.kr_last_error().decode() == f"{who}: {why}", (who, label)
    assert lib.kr_reduce_observer_f64(ref, rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == f"kr_reduce_observer: {why}"
    assert (out == 7.0).all()                                                       # a refused call writes nothing


def test_bad_pointers_counts_and_the_plunging_flow_are_refused(lib):
    sp = observer()
    for args in ((None, 4, DUMMY), (DUMMY, 4, None), (DUMMY, -1, DUMMY)):
        assert lib.kr_post_observer_dev_f64(*POST, C.byref(sp), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_post_observer: null argument or negative n"
        assert lib.kr_reduce_observer_dev_f64(C.byref(sp), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_observer: null argument or negative n"
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(20 * 68 + 10, 7.0)
    p, o = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((None, 4, o), (p, 4, None), (p, -1, o)):
        assert lib.kr_reduce_observer_f64(C.byref(sp), *args) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_observer: null argument or negative n"
    assert (out == 7.0).all()
    plunge = (0.998, capi.V_PLUNGE, 0, 0, 0, -math.pi, math.pi)
    assert lib.kr_post_observer_dev_f64(*plunge, C.byref(sp), DUMMY, 4, DUMMY, None) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == "kr_post_observer: V = KR_V_PLUNGE (the plunging disc flow) is not supported here"


@pytest.mark.parametrize("make", [observer, lambda: observer(nt=0, dt=0.0), lambda: observer(nt=0, dt=NAN), lambda: observer(dist=0.0, gamma=0.0),
                                  lambda: observer(nmu=4096, nt=4092), lambda: observer(nmu=1, nt=(1 << 24) - 4)],
                         ids=["plain", "no time axis", "no time axis, dt unused", "counts", "largest", "longest row"])
def test_valid_specs_reach_the_device_check(lib, make):
    """Without a GPU a valid call ends in KR_ENODEVICE.  With one, only n = 0 is tried here (anything else would run kernels on the dummy pointers): KR_OK,
    and nothing is added."""
    sp = make()
    if lib.kr_device_count() > 0:
        assert lib.kr_post_observer_dev_f64(*POST, C.byref(sp), None, 0, DUMMY, None) == capi.KR_OK
        assert lib.kr_reduce_observer_dev_f64(C.byref(sp), None, 0, DUMMY, None) == capi.KR_OK
        return
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(16, 7.0)
    assert lib.kr_post_observer_dev_f64(*POST, C.byref(sp), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert b"no HIP device" in lib.kr_last_error()
    assert lib.kr_reduce_observer_dev_f64(C.byref(sp), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert lib.kr_reduce_observer_f64(C.byref(sp), rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_ENODEVICE
    assert (out == 7.0).all()


def test_the_api_refuses_what_it_can_see_without_a_device():
    sp = observer()
    p = capi.default_params(0.5)
    with pytest.raises(capi.KrError, match="spec.spin is not the spin of params"):
        api.source_to_observer(capi.PointSourceSpec(), p, sp)
    with pytest.raises(capi.KrError, match="PointSourceSpec, a PointSourceVelSpec or a HealpixSource"):
        api.source_to_observer(object(), capi.default_params(0.998), sp)
