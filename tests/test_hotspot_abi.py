"""CPU: the C ABI of the orbiting hot spot (kr_hotspot; kr_post_hotspot_dev_f64, kr_reduce_hotspot_dev_f64, kr_reduce_hotspot_f64): the struct's size
against the header's static_assert, every refusal of the struct's comment with its message -- before any device is touched, so the dummy device pointers
below are never dereferenced -- and, on a machine without a GPU, KR_ENODEVICE for a valid call (there is no CPU fallback)."""
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


def spot(**kw):
    h = capi.hot_spot(10.0, 1.5, spin=0.998, t0=9990.0, dt=2.0, nt=8, line_energy=6.4, e_min=1.0, de=0.5, ne=4, r_isco=1.237, r_disc=30.0)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_struct_size_and_abi_version(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_hotspot\) == (\d+)", header).group(1))
    assert C.sizeof(capi.HotSpot) == size == 136
    assert (capi.HotSpot.r_spot.offset, capi.HotSpot.a_orbit.offset, capi.HotSpot.r_disc.offset) == (0, 40, 104)
    assert (capi.HotSpot.nt.offset, capi.HotSpot.ne.offset, capi.HotSpot.log_e.offset, capi.HotSpot.shear.offset, capi.HotSpot.pad.offset) == (112, 116, 120, 124, 128)
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()                          # additive: three more entry points
    for name in ("kr_post_hotspot_dev_f64", "kr_reduce_hotspot_dev_f64", "kr_reduce_hotspot_f64"):
        assert name in capi.PROTOTYPES and hasattr(lib, name)


REFUSALS = [
    ("null spot", None, "null spot"),
    ("nt 0", lambda: spot(nt=0), "nt must be in 1 ... 4096"),
    ("nt 4097", lambda: spot(nt=4097, ne=0), "nt must be in 1 ... 4096"),
    ("ne -1", lambda: spot(ne=-1), "ne must be in 0 ... 4096"),
    ("ne 4097", lambda: spot(ne=4097), "ne must be in 0 ... 4096"),
    ("nt ne too large", lambda: spot(nt=1025, ne=1024), "nt * ne must not exceed 2^20"),
    ("sigma 0", lambda: spot(sigma=0.0), "sigma must be positive"),
    ("sigma negative", lambda: spot(sigma=-1.0), "sigma must be positive"),
    ("cut 0", lambda: spot(cut=0.0), "cut must be positive"),
    ("r_spot 0", lambda: spot(r_spot=0.0), "r_spot must be positive"),
    ("nan sigma", lambda: spot(sigma=NAN), "non-finite spot parameter"),
    ("inf omega", lambda: spot(omega=float("inf")), "non-finite spot parameter"),
    ("nan t0", lambda: spot(t0=NAN), "non-finite spot parameter"),
    ("nan dt", lambda: spot(dt=NAN), "non-finite spot parameter"),
    ("nan phi0", lambda: spot(phi0=NAN), "non-finite spot parameter"),
    ("nan g_index", lambda: spot(g_index=NAN), "non-finite spot parameter"),
    ("inf r_disc", lambda: spot(r_disc=float("inf")), "non-finite spot parameter"),
    ("nan e_min without a grid", lambda: spot(ne=0, e_min=NAN), "non-finite spot parameter"),
    ("de 0", lambda: spot(de=0.0), "de must be positive"),
    ("log_e de 1", lambda: spot(log_e=1, de=1.0), "log_e: de (the ratio between edges) must be > 1"),
    ("log_e e_min 0", lambda: spot(log_e=1, de=1.1, e_min=0.0), "log_e: e_min must be positive"),
    ("line_energy 0", lambda: spot(line_energy=0.0), "line_energy must be positive"),
    ("shear 2", lambda: spot(shear=2), "shear must be 0 or 1"),
    ("shear -1", lambda: spot(shear=-1), "shear must be 0 or 1"),
    ("shear a_orbit", lambda: spot(shear=1, a_orbit=-2.0), "shear: a_orbit + r_isco sqrt(r_isco) must be positive"),
]


@pytest.mark.parametrize("label,make,why", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_spots_are_refused_before_any_device_work(lib, label, make, why):
    h = make() if make else None
    ref = C.byref(h) if h is not None else None
    law = capi.limb_law("isotropic")
    out = np.full(64, 7.0)
    rays = np.zeros(4, dtype=capi.RAY_F64)
    calls = {"kr_post_hotspot": lambda: lib.kr_post_hotspot_dev_f64(*POST, ref, C.byref(law), DUMMY, 4, DUMMY, None),
             "kr_reduce_hotspot": lambda: lib.kr_reduce_hotspot_dev_f64(ref, DUMMY, 4, DUMMY, None)}
    for who, call in calls.items():
        assert call() == capi.KR_EINVAL, (who, label)
        assert lib.kr_last_error().decode() == f"{who}: {why}", (who, label)
    assert lib.kr_reduce_hotspot_f64(ref, rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == f"kr_reduce_hotspot: {why}"
    assert (out == 7.0).all()                                                       # a refused call writes nothing


def test_a_grid_that_is_not_used_is_not_judged(lib):
    """ne == 0: de, e_min and line_energy may hold anything finite."""
    h = spot(ne=0, de=-1.0, line_energy=0.0, log_e=1, e_min=0.0)
    rc = lib.kr_reduce_hotspot_dev_f64(C.byref(h), None, 0, DUMMY, None)
    assert rc in (capi.KR_OK, capi.KR_ENODEVICE)


def test_bad_laws_pointers_and_counts_are_refused(lib):
    h, iso = spot(), capi.limb_law("isotropic")
    cases = [(lambda: lib.kr_post_hotspot_dev_f64(*POST, C.byref(h), None, DUMMY, 4, DUMMY, None), "kr_post_hotspot: "),
             (lambda: lib.kr_post_hotspot_dev_f64(*POST, C.byref(h), C.byref(capi.limb_law((3, 0.0))), DUMMY, 4, DUMMY, None), "kr_post_hotspot: ")]
    for call, prefix in cases:
        assert call() == capi.KR_EINVAL and lib.kr_last_error().decode().startswith(prefix)
    moving = (0.998, -1.0, 1, 0, 1, -math.pi, math.pi)
    assert lib.kr_post_hotspot_dev_f64(*moving, C.byref(h), C.byref(capi.limb_law("laor")), DUMMY, 4, DUMMY, None) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == "kr_post_hotspot: motion != 0 needs limb law 0 (only the orbiting observer has the frame of mu)"
    for args in ((C.byref(iso), None, 4, DUMMY), (C.byref(iso), DUMMY, 4, None), (C.byref(iso), DUMMY, -1, DUMMY)):
        assert lib.kr_post_hotspot_dev_f64(*POST, C.byref(h), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_post_hotspot: null argument or negative n"
    for args in ((None, 4, DUMMY), (DUMMY, 4, None), (DUMMY, -1, DUMMY)):
        assert lib.kr_reduce_hotspot_dev_f64(C.byref(h), *args, None) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_hotspot: null argument or negative n"
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.zeros(64)
    r, o = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((None, 4, o), (r, 4, None), (r, -1, o)):
        assert lib.kr_reduce_hotspot_f64(C.byref(h), *args) == capi.KR_EINVAL
        assert lib.kr_last_error().decode() == "kr_reduce_hotspot: null argument or negative n"


@pytest.mark.parametrize("make", [spot, lambda: spot(ne=0), lambda: spot(shear=1), lambda: spot(omega=0.0), lambda: spot(omega=-0.03, log_e=1, de=1.2)],
                         ids=["spectrogram", "light curve", "shear", "static", "retrograde-log"])
def test_valid_spots_reach_the_device_check(lib, make):
    """Without a GPU a valid call ends in KR_ENODEVICE.  With one, only n = 0 is tried here (anything else would run kernels on the dummy pointers): KR_OK."""
    h, law = make(), capi.limb_law("laor")
    if lib.kr_device_count() > 0:
        assert lib.kr_post_hotspot_dev_f64(*POST, C.byref(h), C.byref(law), None, 0, DUMMY, None) == capi.KR_OK
        assert lib.kr_reduce_hotspot_dev_f64(C.byref(h), None, 0, DUMMY, None) == capi.KR_OK
        return
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.full(64, 7.0)
    assert lib.kr_post_hotspot_dev_f64(*POST, C.byref(h), C.byref(law), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert b"no HIP device" in lib.kr_last_error()
    assert lib.kr_reduce_hotspot_dev_f64(C.byref(h), DUMMY, 4, DUMMY, None) == capi.KR_ENODEVICE
    assert lib.kr_reduce_hotspot_f64(C.byref(h), rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_ENODEVICE
    assert (out == 7.0).all()
