"""CPU: the ray-path entry points (kr_trace_paths_*) are additive -- the ABI version and the pinned struct sizes stay -- and refuse every bad
argument before they touch a device; without a GPU a valid call answers KR_ENODEVICE like everything else (no CPU integration loop)."""
import ctypes as C

import numpy as np
import pytest

from raytrace_cpu_amd import api, capi


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_abi_version_and_struct_sizes_unchanged(lib):
    assert capi.ABI_VERSION == 16 and lib.kr_abi_version() == 16
    assert C.sizeof(capi.PathSpec) == 24
    assert C.sizeof(capi.Params) == 128 and C.sizeof(capi.Stats) == 136
    assert capi.PathSpec.write_rmin.offset == 0 and capi.PathSpec.write_rmax.offset == 8 and capi.PathSpec.write_step.offset == 16


def _args(n=4):
    rays = np.zeros(n, dtype=capi.RAY_F64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    traced = np.zeros(n, dtype=np.uint8)
    return rays, offsets, traced


def _host_call(lib, p, w, n=4, null=None):
    rays, offsets, traced = _args(max(n, 1))
    rows, total = C.c_void_p(), C.c_int64()
    a = dict(p=C.byref(p) if p is not None else None, w=C.byref(w) if w is not None else None, rays=rays.ctypes.data_as(C.c_void_p),
             offsets=offsets.ctypes.data_as(C.c_void_p), rows=C.byref(rows), total=C.byref(total))
    if null:
        a[null] = None
    rc = lib.kr_trace_paths_f64(a["p"], a["w"], a["rays"], n, a["offsets"], traced.ctypes.data_as(C.c_void_p), a["rows"], a["total"], None)
    assert (rays["r"] == 0).all() and not rows.value
    return rc, lib.kr_last_error().decode()


def _dev_calls(lib, p, w, n=4):
    """both device-pointer forms with (never dereferenced) non-null pointers"""
    fake = C.c_void_p(4096)
    total = C.c_int64()
    rc1 = lib.kr_trace_paths_count_dev_f64(C.byref(p), C.byref(w), fake, n, fake, None, C.byref(total), None)
    m1 = lib.kr_last_error().decode()
    rc2 = lib.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w), fake, n, fake, fake, 0, None, None)
    return (rc1, m1), (rc2, lib.kr_last_error().decode())


REFUSALS = [
    ("write_step 0", dict(), dict(write_step=0), "write_step must be positive"),
    ("write_step negative", dict(), dict(write_step=-3), "write_step must be positive"),
    ("NaN write_rmin", dict(), dict(write_rmin=float("nan")), "must not be NaN"),
    ("NaN write_rmax", dict(), dict(write_rmax=float("nan")), "must not be NaN"),
    ("fast math", dict(flags=capi.FLAG_FAST_MATH), dict(), "KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted"),
    ("hybrid", dict(flags=capi.FLAG_HYBRID), dict(), "KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted"),
    ("rk45", dict(integrator=capi.RK45), dict(), "RK45 paths are not recorded"),
    ("euler + destination", dict(integrator=capi.EULER, stop_kind=capi.STOP_FLATDISC), dict(), "Integrator::Euler does not support RayDestination stopping conditions"),
    ("unknown integrator", dict(integrator=7), dict(), "unknown integrator"),
    ("unknown stop kind", dict(integrator=capi.RK4, stop_kind=9), dict(), "unknown stop_kind"),
]


@pytest.mark.parametrize("what,pkw,wkw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_device_work(lib, what, pkw, wkw, msg):
    p = capi.copy_params(capi.default_params(0.998), **pkw)
    w = api.path_spec(**wkw)
    rc, err = _host_call(lib, p, w)
    assert rc == capi.KR_EINVAL and msg in err and err.startswith("kr_trace_paths:"), err
    for (rc, err), who in zip(_dev_calls(lib, p, w), ("kr_trace_paths_count:", "kr_trace_paths_record:")):
        assert rc == capi.KR_EINVAL and msg in err and err.startswith(who), err


def test_null_pointers_and_negative_n_are_refused(lib):
    p, w = capi.default_params(0.998), api.path_spec()
    for null in ("p", "w", "offsets", "rows", "total"):
        rc, err = _host_call(lib, p, w, null=null)
        assert rc == capi.KR_EINVAL and "null argument" in err, (null, err)
    rc, err = _host_call(lib, p, w, n=-1)
    assert rc == capi.KR_EINVAL and "negative n" in err
    fake, total = C.c_void_p(4096), C.c_int64()
    assert lib.kr_trace_paths_count_dev_f64(C.byref(p), C.byref(w), fake, -1, fake, None, C.byref(total), None) == capi.KR_EINVAL
    assert lib.kr_trace_paths_count_dev_f64(C.byref(p), C.byref(w), fake, 4, None, None, C.byref(total), None) == capi.KR_EINVAL
    assert lib.kr_trace_paths_count_dev_f64(C.byref(p), C.byref(w), fake, 4, fake, None, None, None) == capi.KR_EINVAL
    assert lib.kr_trace_paths_count_dev_f64(C.byref(p), C.byref(w), None, 4, fake, None, C.byref(total), None) == capi.KR_EINVAL
    assert lib.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w), fake, 4, fake, None, 0, None, None) == capi.KR_EINVAL
    assert lib.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w), fake, 4, None, fake, 0, None, None) == capi.KR_EINVAL
    assert lib.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w), fake, 4, fake, fake, -1, None, None) == capi.KR_EINVAL
    assert lib.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w), fake, 4, fake, C.c_void_p(4096 + 8), 0, None, None) == capi.KR_EINVAL
    assert "32-byte aligned" in lib.kr_last_error().decode()


def test_no_device_means_enodevice_not_a_cpu_loop(lib):
    if lib.kr_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, w = capi.copy_params(capi.default_params(0.998), integrator=capi.RK4), api.path_spec(write_step=10)
    rc, err = _host_call(lib, p, w)
    assert rc == capi.KR_ENODEVICE and "no HIP device" in err
    for rc, err in _dev_calls(lib, p, w):
        assert rc == capi.KR_ENODEVICE and "no HIP device" in err
    with pytest.raises(capi.KrError, match="no HIP device"):
        api.trace_paths(p, np.zeros(4, dtype=capi.RAY_F64))


def test_paths_text_is_the_reference_file_format():
    offsets = np.array([0, 2, 2, 2, 3])
    rows = np.array([[0.0, 1.2369706630706787, -1e-3, 1e100], [1.0, 2.0, 3.0, 4.0], [float("nan"), -float("inf"), 5.0, 6.0]])
    traced = np.array([1, 1, 0, 1], dtype=np.uint8)
    text = api.paths_text(offsets, rows, traced)
    assert text == ("      0.00000000e+00      1.23697066e+00     -1.00000000e-03     1.00000000e+100\n"
                    "      1.00000000e+00      2.00000000e+00      3.00000000e+00      4.00000000e+00\n\n\n"
                    "\n\n"
                    "                 nan                -inf      5.00000000e+00      6.00000000e+00\n\n\n")


def test_fixture_files_have_the_shape_the_comparison_expects():
    import paths_rules as pr
    want = {"ps_euler": 35, "ps_euler_window": 35, "ip_euler": 25, "rk4_theta": 35, "rk4_isco": 35, "rk4_window": 35}
    for name in pr.CASES:
        text = pr.reference_text(name)
        assert len(pr.blocks_of(text)) == want[name]
        res = pr.compare_texts(text, text)
        assert res["n_bad"] == 0 and res["frac_blocks_identical"] == 1.0
    assert len(pr.blocks_of(pr.reference_text("ps_euler_window"))) and sum(map(len, pr.blocks_of(pr.reference_text("ps_euler_window")))) == 4207
    assert sum(map(len, pr.blocks_of(pr.reference_text("ip_euler")))) == 1134
    rec = pr.reference_records("rk4_window")
    live = rec["steps"] >= 0            # (the allocation is the int-truncated product of doubles, pointsource.cpp:12: 43 records, 35 rays)
    assert len(rec) == 43 and live.sum() == 35 and (rec["steps"][~live] == -1).all() and np.isfinite(rec["r"][live]).all()
    assert pr.field_close("9.99999999e+00", "1.00000000e+01") and not pr.field_close("1.00000000e+00", "1.00000002e+00")
