"""CPU: the entry points of the point source with any four-velocity (kr_pointsource_vel_*) and of the angular distribution (kr_*_angdist_*) are
additive -- the ABI version and the pinned struct sizes stay -- and refuse every bad argument, with its message, before they touch a device; without a
GPU a valid call answers KR_ENODEVICE like everything else (no CPU fallback)."""
import ctypes as C
import math

import numpy as np
import pytest

import source_vel_rules as sv
from raytrace_cpu_amd import api, capi


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_abi_version_and_struct_layouts(lib):
    assert capi.ABI_VERSION == 16 and lib.kr_abi_version() == 16
    assert C.sizeof(capi.PointSourceVelSpec) == 136 and C.sizeof(capi.AngdistSpec) == 72
    assert C.sizeof(capi.PointSourceSpec) == 112 and C.sizeof(capi.ReturnBins) == 56 and C.sizeof(capi.ReturnMap) == 88
    S = capi.PointSourceVelSpec
    assert (S.pos.offset, S.u.offset, S.spin.offset, S.tol.offset, S.E.offset, S.dcosalpha.offset, S.betamax.offset) == (0, 32, 64, 72, 80, 88, 128)
    assert capi.AngdistSpec.dangle.offset == 56 and capi.AngdistSpec.labels.offset == 64


FAKE = C.c_void_p(4096)


def _init_calls(lib, spec, n, null_rays=False):
    """the three init forms: the device ones with a (never dereferenced) non-null pointer, the host one with a real array that must stay untouched"""
    rays = np.zeros(max(n, 1), dtype=capi.RAY_F64)
    s = C.byref(spec) if spec is not None else None
    out = []
    out.append((lib.kr_pointsource_vel_init_dev_f64(s, None if null_rays else FAKE, n, None), lib.kr_last_error().decode(), "kr_pointsource_vel_init:"))
    out.append((lib.kr_pointsource_vel_init_emit_dev_f64(s, None if null_rays else FAKE, n, None), lib.kr_last_error().decode(), "kr_pointsource_vel_init_emit:"))
    out.append((lib.kr_pointsource_vel_init_f64(s, None if null_rays else rays.ctypes.data_as(C.c_void_p), n), lib.kr_last_error().decode(), "kr_pointsource_vel_init:"))
    assert (rays["r"] == 0).all() and (rays["steps"] == 0).all()
    return out


def _spec(**kw):
    pos = kw.pop("pos", (0.0, 6.0, 1.2, 0.3))
    u = kw.pop("u", (1.3, 0.2, -0.01, 0.08))
    return api.pointsource_vel_spec(pos, u, kw.pop("spin", 0.998), kw.pop("dcosalpha", 0.06), kw.pop("dbeta", 0.18), **kw)


NAN, INF = float("nan"), float("inf")
REFUSALS = [
    ("NaN pos", dict(pos=(0.0, NAN, 1.2, 0.3)), "pos is not finite"),
    ("infinite pos", dict(pos=(INF, 6.0, 1.2, 0.3)), "pos is not finite"),
    ("NaN u", dict(u=(1.3, NAN, 0.0, 0.0)), "u is not finite"),
    ("infinite u", dict(u=(INF, 0.0, 0.0, 0.0)), "u is not finite"),
    ("spacelike u", dict(u=(1.0, 1.5, 0.0, 0.0)), "u is not timelike"),
    ("faster than light in phi", dict(u=(1.0, 0.0, 0.0, 0.5)), "u is not timelike"),
    ("at rest in the ergosphere", dict(pos=(0.0, 1.5, math.pi / 2, 0.0), u=(1.0, 0.0, 0.0, 0.0)), "u is not timelike"),
    ("past-directed u", dict(u=(-1.3, 0.2, -0.01, -0.08)), "u^t must be positive"),
    ("u^t zero", dict(u=(0.0, 0.0, 0.0, 0.0)), "u^t must be positive"),
    ("inside the horizon", dict(pos=(0.0, 1.05, 1.2, 0.3)), "r <= horizon"),
    ("on the horizon", dict(pos=(0.0, 2.0, 1.2, 0.3), spin=0.0), "r <= horizon"),
    ("spin beyond 1", dict(spin=1.5), "r <= horizon"),
    ("zero grid step", dict(dcosalpha=0.0), "ray count is not a non-negative int"),
    ("NaN grid", dict(betamax=NAN), "ray count is not a non-negative int"),
    ("count beyond int", dict(dcosalpha=1e-6, dbeta=1e-6), "ray count is not a non-negative int"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_device_work(lib, what, kw, msg):
    spec = _spec(**kw)
    n = max(int(lib.kr_pointsource_vel_count(C.byref(spec), None, None)), 0)
    for rc, err, who in _init_calls(lib, spec, n):
        assert rc == capi.KR_EINVAL and msg in err and err.startswith(who), (what, rc, err)
    assert lib.kr_pointsource_vel_tetrad(C.byref(spec), np.zeros(16).ctypes.data_as(C.c_void_p)) == capi.KR_EINVAL
    assert msg in lib.kr_last_error().decode()


def test_null_pointers_negative_n_and_a_wrong_count_are_refused(lib):
    spec = _spec()
    n = api.pointsource_vel_count(spec)[0]
    assert n == sv.grid(spec)[0] > 1000
    for rc, err, who in _init_calls(lib, None, n):
        assert rc == capi.KR_EINVAL and err == who + " null spec", err
    for rc, err, who in _init_calls(lib, spec, -1):
        assert rc == capi.KR_EINVAL and err == who + " negative n", err
    for rc, err, who in _init_calls(lib, spec, n, null_rays=True):
        assert rc == capi.KR_EINVAL and err == who + " null ray buffer", err
    for wrong in (n - 1, n + 1, 1, 0):
        for rc, err, who in _init_calls(lib, spec, wrong):
            assert rc == capi.KR_EINVAL and err == who + " n is not kr_pointsource_vel_count()", (wrong, err)
    assert lib.kr_pointsource_vel_count(None, None, None) == -1
    assert lib.kr_pointsource_vel_tetrad(C.byref(spec), None) == capi.KR_EINVAL and "null argument" in lib.kr_last_error().decode()
    assert lib.kr_pointsource_vel_tetrad(None, None) == capi.KR_EINVAL


def _angdist_calls(lib, sp, n=4, d=FAKE, out=FAKE):
    s = C.byref(sp) if sp is not None else None
    rays, words = np.zeros(max(n, 1), dtype=capi.RAY_F64), np.full(14 * 4096 + 8, 7.0)
    res = [(lib.kr_reduce_angdist_dev_f64(s, d, n, out, None), lib.kr_last_error().decode(), "kr_reduce_angdist:"),
           (lib.kr_post_angdist_dev_f64(0.998, -1.0, 0, 0, 0, -math.pi, math.pi, s, d, n, out, None), lib.kr_last_error().decode(), "kr_post_angdist:"),
           (lib.kr_reduce_angdist_f64(s, rays.ctypes.data_as(C.c_void_p) if d else None, n, words.ctypes.data_as(C.c_void_p) if out else None),
            lib.kr_last_error().decode(), "kr_reduce_angdist:")]
    assert (words == 7.0).all()
    return res


@pytest.mark.parametrize("dangle,nangle", [(0.1, 62), (2 * math.pi / 62.5, 62), (2 * math.pi / 63.5, 63), (2 * math.pi / 4096.5, 4096), (2 * math.pi, 1)])
def test_nangle_is_the_truncated_quotient(lib, dangle, nangle):
    sp = api.angdist_spec(1.24, 500.0, 1000.0, dangle=dangle)
    assert lib.kr_angdist_nangle(C.byref(sp)) == nangle == sv.nangle_of(sp) and api.angdist_words(sp) == 14 * nangle + 8


@pytest.mark.parametrize("dangle", [0.0, -0.1, NAN, INF, 7.0, 2 * math.pi / 4097.5], ids=["zero", "negative", "NaN", "infinite", "wider than the circle", "4097 bins"])
def test_angdist_refuses_a_bad_dangle(lib, dangle):
    sp = api.angdist_spec(1.24, 500.0, 1000.0, dangle=dangle)
    assert lib.kr_angdist_nangle(C.byref(sp)) == -1
    for rc, err, who in _angdist_calls(lib, sp):
        assert rc == capi.KR_EINVAL and err.startswith(who) and "dangle must give 1 ... 4096 bins" in err, err


@pytest.mark.parametrize("labels", [-1, 2])
def test_angdist_refuses_unknown_labels(lib, labels):
    sp = api.angdist_spec(1.24, 500.0, 1000.0, labels=labels)
    assert lib.kr_angdist_nangle(C.byref(sp)) == -1
    for rc, err, who in _angdist_calls(lib, sp):
        assert rc == capi.KR_EINVAL and err == who + " labels must be 0 (PointSource) or 1 (PointSourceVel)", err


def test_angdist_refuses_null_pointers_and_negative_n(lib):
    sp = api.angdist_spec(1.24, 500.0, 1000.0)
    for rc, err, who in _angdist_calls(lib, None):
        assert rc == capi.KR_EINVAL and err == who + " null spec", err
    for kw in (dict(n=-1), dict(d=None), dict(out=None)):
        for rc, err, who in _angdist_calls(lib, sp, **kw):
            assert rc == capi.KR_EINVAL and err == who + " null argument or negative n", (kw, err)


def test_no_device_means_enodevice_not_a_cpu_loop(lib):
    if lib.kr_device_count() > 0:
        pytest.skip("a GPU is visible")
    spec = _spec()
    n = api.pointsource_vel_count(spec)[0]
    for rc, err, _ in _init_calls(lib, spec, n):
        assert rc == capi.KR_ENODEVICE and "no HIP device" in err
    for rc, err, _ in _angdist_calls(lib, api.angdist_spec(1.24, 500.0, 1000.0)):
        assert rc == capi.KR_ENODEVICE and "no HIP device" in err
    with pytest.raises(capi.KrError, match="no HIP device"):
        api.pointsource_vel_init(spec)
    with pytest.raises(capi.KrError, match="no HIP device"):
        api.source_angdist(spec, capi.default_params(0.998), api.angdist_spec(1.24, 500.0, 1000.0, labels=1))
