"""CPU: the crossing entry points (kr_trace_crossings_*, kr_reduce_crossing_image_dev_f64) are additive -- the ABI version and the pinned struct sizes
stay -- and refuse every bad argument before they touch a device, with a message that names it, writing nothing to the caller's buffers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import golden_cases as gc
from raytrace_cpu_amd import api, capi

ROOT = gc.ROOT
FAKE = 4096          # a never-dereferenced, 32-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_abi_version_and_struct_size(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_crossing_spec\) == (\d+)", header).group(1))
    assert C.sizeof(capi.CrossingSpec) == size == 32
    assert [capi.CrossingSpec.__dict__[f].offset for f in ("V", "max_crossings", "stop_when_full", "reverse", "projradius", "motion", "pad")] == [0, 8, 12, 16, 20, 24, 28]
    assert capi.ABI_VERSION == 16 and lib.kr_abi_version() == 16
    assert C.sizeof(capi.Params) == 128 and C.sizeof(capi.Stats) == 136 and C.sizeof(capi.VolumeMap) == 72 and C.sizeof(capi.PathSpec) == 24


def test_spec_constructor():
    s = api.crossing_spec()
    assert (s.V, s.max_crossings, s.stop_when_full, s.reverse, s.projradius, s.motion, s.pad) == (-1.0, 4, 1, 0, 0, 0, 0)
    s = api.crossing_spec(max_crossings=2, stop_when_full=False, V=0.3, reverse=1, projradius=1, motion=1)
    assert (s.V, s.max_crossings, s.stop_when_full, s.reverse, s.projradius, s.motion) == (0.3, 2, 0, 1, 1, 1)


def _calls(lib, p, spec, n=4, null=(), rows_at=FAKE):
    """the host-pointer and the device-pointer form (with never-dereferenced non-null pointers); -> [(rc, message), (rc, message)]"""
    M = spec.max_crossings if 1 <= spec.max_crossings <= 16 else 16
    rays = np.zeros(max(n, 1), dtype=capi.RAY_F64)
    rows = np.full((max(n, 1), M, 4), 7.0)
    seen = np.full(max(n, 1), -5, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    pp = None if "p" in null else C.byref(p)
    ss = None if "spec" in null else C.byref(spec)
    rc1 = lib.kr_trace_crossings_f64(pp, ss, None if "rays" in null else vp(rays), n, None if "rows" in null else vp(rows), None if "seen" in null else vp(seen),
                                     None)
    e1 = lib.kr_last_error().decode()
    fake = C.c_void_p(FAKE)
    rc2 = lib.kr_trace_crossings_dev_f64(pp, ss, None if "rays" in null else fake, n, None if "rows" in null else C.c_void_p(rows_at), None if "seen" in null else fake,
                                         None, None)
    e2 = lib.kr_last_error().decode()
    assert (rays["r"] == 0).all() and (rows == 7.0).all() and (seen == -5).all()          # (nothing was written)
    return [(rc1, e1), (rc2, e2)]


REFUSALS = [
    ("M 0", dict(), dict(max_crossings=0), "max_crossings must be 1..16"),
    ("M negative", dict(), dict(max_crossings=-1), "max_crossings must be 1..16"),
    ("M 17", dict(), dict(max_crossings=17), "max_crossings must be 1..16"),
    ("motion 2", dict(), dict(motion=2), "unknown motion"),
    ("motion negative", dict(), dict(motion=-1), "unknown motion"),
    # what paths_validate refuses of a kr_params
    ("fast math", dict(flags=capi.FLAG_FAST_MATH), dict(), "KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted"),
    ("hybrid", dict(flags=capi.FLAG_HYBRID), dict(), "KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted"),
    ("rk45", dict(integrator=capi.RK45), dict(), "RK45"),
    ("euler + destination", dict(integrator=capi.EULER, stop_kind=capi.STOP_FLATDISC), dict(), "does not support RayDestination"),
]


def _spec(**kw):
    s = api.crossing_spec()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("what,pkw,skw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_device_work(lib, what, pkw, skw, msg):
    p = capi.copy_params(capi.default_params(0.998), **pkw)
    for rc, err in _calls(lib, p, _spec(**skw)):
        assert rc == capi.KR_EINVAL and msg in err and err.startswith("kr_trace_crossings:"), (rc, err)


def test_null_pointers_negative_n_and_alignment_are_refused(lib):
    p, s = capi.default_params(0.998), _spec()
    for null in ("p", "spec", "rays", "rows", "seen"):
        for rc, err in _calls(lib, p, s, null=(null,)):
            assert rc == capi.KR_EINVAL and "null" in err and err.startswith("kr_trace_crossings:"), (null, rc, err)
    for rc, err in _calls(lib, p, s, n=-1):
        assert rc == capi.KR_EINVAL and "negative n" in err, (rc, err)
    for off in (8, 16, 24):
        rc, err = _calls(lib, p, s, rows_at=FAKE + off)[1]
        assert rc == capi.KR_EINVAL and "d_rows must be 32-byte aligned" in err, (off, rc, err)


def _reduce(lib, bins, M, order, n=4, null=()):
    fake = C.c_void_p(FAKE)
    arg = lambda k: None if k in null else fake      # noqa: E731
    rc = lib.kr_reduce_crossing_image_dev_f64(None if "bins" in null else C.byref(bins), M, order, -np.pi, np.pi, arg("rays"), arg("rows"), arg("seen"), n, arg("planes"), None)
    return rc, lib.kr_last_error().decode()


def test_reducer_refusals(lib):
    bins = gc.image_bins(gc.cases()["ip16"]["source"])
    for M, order, msg in ((4, 4, "order must be"), (4, -2, "order must be"), (1, 1, "order must be"), (0, 0, "max_crossings must be 1..16"), (17, 0, "max_crossings must be 1..16")):
        rc, err = _reduce(lib, bins, M, order)
        assert rc == capi.KR_EINVAL and msg in err and err.startswith("kr_reduce_crossing_image:"), (M, order, rc, err)
    for null in ("bins", "rays", "rows", "seen", "planes"):
        rc, err = _reduce(lib, bins, 4, 0, null=(null,))
        assert rc == capi.KR_EINVAL and "null argument" in err, (null, rc, err)
    rc, err = _reduce(lib, bins, 4, 0, n=-1)
    assert rc == capi.KR_EINVAL and "negative n" in err
    empty = gc.image_bins(gc.cases()["ip16"]["source"])
    empty.img_nx = 0
    rc, err = _reduce(lib, empty, 4, 0)
    assert rc == capi.KR_EINVAL and "image size must be positive" in err


def test_a_valid_call_needs_a_device(lib):
    """(the refusals above are not an artefact of a missing device: a valid call gets past them)"""
    if lib.kr_device_count() > 0:
        return
    bins = gc.image_bins(gc.cases()["ip16"]["source"])
    for p in (capi.default_params(0.998), capi.copy_params(capi.default_params(0.998), integrator=capi.RK4, theta_max=0.0),
              capi.copy_params(capi.default_params(0.5), integrator=capi.RK4, stop_kind=capi.STOP_DISC_ISCO, stop_params=(4.2, 400.0, np.pi / 2))):
        for s in (_spec(), _spec(max_crossings=1, stop_when_full=0), _spec(max_crossings=16, motion=1, V=0.3)):
            for rc, err in _calls(lib, p, s) + _calls(lib, p, s, n=0):
                assert rc == capi.KR_ENODEVICE and "no HIP device" in err, (rc, err)
    for order in (-1, 0, 3):
        rc, err = _reduce(lib, bins, 4, order)
        assert rc == capi.KR_ENODEVICE and "no HIP device" in err
    rays = np.zeros(4, dtype=capi.RAY_F64)
    with pytest.raises(capi.KrError, match="no HIP device"):
        api.trace_crossings(capi.default_params(0.998), rays, api.crossing_spec())
    with pytest.raises(capi.KrError, match="no HIP device"):
        api.reduce_crossing_image(bins, rays, np.zeros((4, 2, 4)), np.zeros(4, dtype=np.int32), 0)
    with pytest.raises(capi.KrError, match="no HIP device"):
        api.order_images(gc.cases()["ip16"]["source"], capi.copy_params(capi.default_params(-0.998), integrator=capi.RK4, theta_max=0.0), bins, api.crossing_spec(), [0, 1, -1])
    with pytest.raises(capi.KrError, match="rows must be shaped"):
        api.reduce_crossing_image(bins, rays, np.zeros((3, 2, 4)), np.zeros(4, dtype=np.int32), 0)


def test_program_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        return
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raytrace_cpu_amd", "apps")], check=True)
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_imageplane_orders")
    out = tmp_path / "orders.fits"
    r = subprocess.run([exe, f"--parfile={os.path.join(ROOT, 'tests', 'golden', 'apps', 'imageplane_orders.par')}", f"--outfile={out}"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and list(tmp_path.iterdir()) == []
    assert "no HIP device available" in r.stderr
