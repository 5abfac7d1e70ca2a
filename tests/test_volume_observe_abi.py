"""CPU: the observing entry points (kr_trace_observe_*) are additive -- the ABI version and the pinned struct sizes stay -- and refuse every bad
argument before they touch a device, with a message that names the field."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_cpu_amd import api, capi


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_abi_version_and_struct_sizes(lib):
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_observe_bins\) == (\d+)", header).group(1))
    assert C.sizeof(capi.ObserveBins) == size == 48
    assert [capi.ObserveBins.__dict__[f].offset for f in ("en0", "den", "t0", "dt", "nen", "nt", "logbin_en", "pad")] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert capi.ABI_VERSION == 16 and lib.kr_abi_version() == 16
    assert C.sizeof(capi.VolumeMap) == 72 and C.sizeof(capi.Params) == 128 and C.sizeof(capi.Stats) == 136


def _grid(**kw):
    m = api.volume_map_struct(1.2, 40.0, 24, 16, 1, False)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _bins(**kw):
    b = api.observe_bins_struct(0.5, 1.5, 32, t0=0.0, tmax=100.0, nt=20)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _calls(lib, p, m, b, n=4, null=()):
    """the host-pointer and the device-pointer form (with never-dereferenced non-null pointers); -> [(rc, message), (rc, message)]"""
    rays = np.zeros(max(n, 1), dtype=capi.RAY_F64)
    ncell = m.nr * m.ntheta * m.nphi
    cells = np.ones(ncell if 0 < ncell < 1 << 20 else 16)
    words = np.zeros(api.observe_words(b) if 0 < b.nen < 1 << 12 and 0 <= b.nt < 1 << 8 else 16)
    image = np.zeros(max(n, 1))
    fake = C.c_void_p(4096)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    pp = None if "p" in null else C.byref(p)
    mm = None if "m" in null else C.byref(m)
    bb = None if "b" in null else C.byref(b)
    rc1 = lib.kr_trace_observe_f64(pp, mm, bb, None if "emis" in null else vp(cells), None, None, None if "rays" in null else vp(rays), n,
                                   None if "out" in null else vp(words), vp(image), None)
    e1 = lib.kr_last_error().decode()
    rc2 = lib.kr_trace_observe_dev_f64(pp, mm, bb, None if "emis" in null else fake, None, None, None if "rays" in null else fake, n, None if "out" in null else fake,
                                       None, None, None)
    e2 = lib.kr_last_error().decode()
    assert (rays["r"] == 0).all() and (words == 0).all() and (image == 0).all()
    return [(rc1, e1), (rc2, e2)]


NAN, INF = float("nan"), float("inf")
REFUSALS = [
    # what volume_validate refuses
    ("nr 0", dict(), dict(nr=0), dict(), "at least 1"),
    ("too many cells", dict(), dict(nr=1024, ntheta=1024, nphi=129), dict(), "more than 2^27 cells"),
    ("dr NaN", dict(), dict(dr=NAN), dict(), "dr, dtheta and dphi"),
    ("dtheta 0", dict(), dict(dtheta=0.0), dict(), "dr, dtheta and dphi"),
    ("log dr 1", dict(), dict(logbin=1, dr=1.0), dict(), "needs dr > 1"),
    ("log r_min 0", dict(), dict(logbin=1, dr=1.1, r_min=0.0), dict(), "needs r_min > 0"),
    ("mode 2", dict(), dict(mode=2), dict(), "unknown mode"),
    ("motion 2", dict(), dict(motion=2), dict(), "unknown motion"),
    ("fast math", dict(flags=capi.FLAG_FAST_MATH), dict(), dict(), "KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted"),
    ("hybrid", dict(flags=capi.FLAG_HYBRID), dict(), dict(), "KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted"),
    ("rk45", dict(integrator=capi.RK45), dict(), dict(), "RK45"),
    ("euler + destination", dict(integrator=capi.EULER, stop_kind=capi.STOP_FLATDISC), dict(), dict(), "does not support RayDestination"),
    # the bins
    ("nen 0", dict(), dict(), dict(nen=0), "nen"),
    ("nen negative", dict(), dict(), dict(nen=-3), "nen"),
    ("nt negative", dict(), dict(), dict(nt=-1), "nt"),
    ("too many bins", dict(), dict(), dict(nen=1 << 14, nt=1 << 13), "2 nen + nen nt"),
    ("too many bins, no response", dict(), dict(), dict(nen=(1 << 26) + 1, nt=0), "2 nen + nen nt"),
    ("den 0", dict(), dict(), dict(den=0.0), "den"),
    ("den negative", dict(), dict(), dict(den=-0.1), "den"),
    ("den NaN", dict(), dict(), dict(den=NAN), "den"),
    ("den inf", dict(), dict(), dict(den=INF), "den"),
    ("log den 1", dict(), dict(), dict(logbin_en=1, den=1.0), "den > 1"),
    ("log den below 1", dict(), dict(), dict(logbin_en=1, den=0.5), "den > 1"),
    ("log en0 0", dict(), dict(), dict(logbin_en=1, den=1.1, en0=0.0), "en0 > 0"),
    ("log en0 negative", dict(), dict(), dict(logbin_en=1, den=1.1, en0=-1.0), "en0 > 0"),
    ("dt 0", dict(), dict(), dict(dt=0.0), "dt"),
    ("dt negative", dict(), dict(), dict(dt=-1.0), "dt"),
    ("dt NaN", dict(), dict(), dict(dt=NAN), "dt"),
    ("dt inf", dict(), dict(), dict(dt=INF), "dt"),
    ("en0 NaN", dict(), dict(), dict(en0=NAN), "en0"),
    ("en0 inf", dict(), dict(), dict(en0=INF), "en0"),
    ("t0 NaN", dict(), dict(), dict(t0=NAN), "t0"),
    ("t0 inf", dict(), dict(), dict(t0=-INF), "t0"),
]


@pytest.mark.parametrize("what,pkw,mkw,bkw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_device_work(lib, what, pkw, mkw, bkw, msg):
    p = capi.copy_params(capi.default_params(0.998), **pkw)
    for rc, err in _calls(lib, p, _grid(**mkw), _bins(**bkw)):
        assert rc == capi.KR_EINVAL and msg in err and err.startswith("kr_trace_observe:"), (rc, err)


def test_a_bad_dt_is_only_refused_when_there_is_a_response(lib):
    """nt = 0: dt is not read -- the call gets past validation (to the device, or to its absence)"""
    p = capi.default_params(0.998)
    for rc, err in _calls(lib, p, _grid(), _bins(nt=0, dt=0.0)):
        assert rc != capi.KR_EINVAL, (rc, err)


def test_null_pointers_and_negative_n_are_refused(lib):
    p, m, b = capi.default_params(0.998), _grid(), _bins()
    for null, msg in (("p", "null argument"), ("m", "null argument"), ("b", "bins"), ("emis", "emis"), ("out", "out"), ("rays", "rays")):
        for rc, err in _calls(lib, p, m, b, null=(null,)):
            assert rc == capi.KR_EINVAL and "null" in err and msg in err, (null, rc, err)
    for rc, err in _calls(lib, p, m, b, n=-1):
        assert rc == capi.KR_EINVAL and "negative n" in err, (rc, err)


def test_a_valid_call_needs_a_device(lib):
    """(the refusals above are not an artefact of a missing device: a valid call gets past them)"""
    if lib.kr_device_count() > 0:
        return
    p, m = capi.copy_params(capi.default_params(0.998), integrator=capi.RK4), _grid(mode=1, logbin=1, dr=1.2)
    for b in (_bins(), _bins(nt=0), _bins(logbin_en=1, den=1.05, en0=0.3)):
        for rc, err in _calls(lib, p, m, b):
            assert rc == capi.KR_ENODEVICE and "no HIP device" in err
    with pytest.raises(capi.KrError, match="no HIP device"):
        api.trace_observe(p, np.zeros(4, dtype=capi.RAY_F64), m, _bins(), np.ones(24 * 16))


def test_bins_struct_and_words():
    b = api.observe_bins_struct(0.5, 1.5, 32, t0=10.0, tmax=110.0, nt=20)
    assert (b.en0, b.den, b.t0, b.dt, b.nen, b.nt, b.logbin_en) == (0.5, 1.0 / 32, 10.0, 5.0, 32, 20, 0) and api.observe_words(b) == 64 + 640 + 6
    words = np.arange(api.observe_words(b), dtype=np.float64)
    res = api.observe_from_words(b, words)
    assert res["spectrum"].tolist() == list(range(32)) and res["hits"][0] == 32 and res["response"].shape == (32, 20) and res["response"][1, 2] == 64 + 22
    assert [res[k] for k in api.OBSERVE_TALLIES] == [704, 705, 706, 707, 708, 709] and len(res["energy"]) == 33 and res["energy"][-1] == 1.5
    b0 = api.observe_bins_struct(0.5, 1.5, 8)
    assert b0.nt == 0 and api.observe_words(b0) == 22 and api.observe_from_words(b0, np.zeros(22))["response"].shape == (8, 0)
