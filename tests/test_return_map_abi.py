"""CPU: the landing-map entry points (kr_*_return_map_*) are additive -- the ABI version and the pinned struct sizes stay -- and refuse every bad
argument before they touch a device; without a GPU a valid call answers KR_ENODEVICE like everything else (no CPU reducer)."""
import ctypes as C

import numpy as np
import pytest

from raytrace_cpu_amd import api, capi

FAKE = C.c_void_p(4096)            # a non-null pointer that is never dereferenced
PASS = (0.998, -1.0, 0, 0, 0, -np.pi, np.pi)


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def a_map(nr=7):
    return api.return_map_struct(1.2, 500.0, 500.0, 6.0, 1.5707, 1.2, 2.0, nr, 1)


def test_abi_version_and_struct_sizes(lib):
    assert capi.ABI_VERSION == 16 and lib.kr_abi_version() == 16
    assert C.sizeof(capi.ReturnMap) == 88 and C.sizeof(capi.ReturnBins) == 56
    assert [getattr(capi.ReturnMap, f).offset for f in ("cls", "r_min", "dr", "gamma", "nr", "logbin")] == [0, 56, 64, 72, 80, 84]
    assert C.sizeof(capi.Params) == 128 and C.sizeof(capi.Stats) == 136 and C.sizeof(capi.EmisBins) == 56


def calls(lib, m, rays=FAKE, n=4, out=FAKE):
    """The three single-item forms with the same arguments: [(name, rc, message)]."""
    mp = C.byref(m) if m is not None else None
    host = np.zeros(max(n, 1), dtype=capi.RAY_F64)
    h_out = np.zeros(5 * 4096 + 6)
    res = []
    for name, call in (("kr_reduce_return_map", lambda: lib.kr_reduce_return_map_dev_f64(mp, rays, n, out, None)),
                       ("kr_post_return_map", lambda: lib.kr_post_return_map_dev_f64(*PASS, mp, rays, n, out, None)),
                       ("kr_reduce_return_map", lambda: lib.kr_reduce_return_map_f64(mp, host.ctypes.data_as(C.c_void_p) if rays else None, n,
                                                                                     h_out.ctypes.data_as(C.c_void_p) if out else None))):
        rc = call()
        res.append((name, rc, lib.kr_last_error().decode()))
    return res


REFUSALS = [("null map", dict(m=None), "null map"), ("nr 0", dict(m=a_map(0)), "nr must be positive"), ("nr negative", dict(m=a_map(-3)), "nr must be positive"),
            ("negative n", dict(m=a_map(), n=-1), "negative n"), ("null rays", dict(m=a_map(), rays=None), "null"), ("null out", dict(m=a_map(), out=None), "null argument")]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_single_forms_refuse_before_any_device_work(lib, what, kw, msg):
    for name, rc, err in calls(lib, **kw):
        assert rc == capi.KR_EINVAL and msg in err, (name, rc, err)
        assert err.startswith(name) or what in ("negative n", "null rays"), err


def batch(lib, count, maps, rays, ns, outs):
    k = max(count, len(ns) if ns is not None else 1, 1)
    mm = (capi.ReturnMap * k)(*maps) if maps is not None else None
    dd = (C.c_void_p * k)(*rays) if rays is not None else None
    nn = (C.c_int64 * k)(*ns) if ns is not None else None
    oo = (C.c_void_p * k)(*outs) if outs is not None else None
    rc = lib.kr_post_return_map_batch_dev_f64(count, *PASS, mm, dd, nn, oo, None)
    return rc, lib.kr_last_error().decode()


def test_batch_form_refuses_before_any_device_work(lib):
    good = dict(maps=[a_map(), a_map(1025)], rays=[4096, 8192], ns=[4, 4], outs=[4096, 8192])
    for what, kw, msg in (("negative count", dict(count=-1), "negative count"), ("null maps", dict(maps=None), "null argument"),
                          ("null rays array", dict(rays=None), "null argument"), ("null n", dict(ns=None), "null argument"),
                          ("null outs array", dict(outs=None), "null argument"), ("nr 0", dict(maps=[a_map(), a_map(0)]), "nr must be positive"),
                          ("negative n", dict(ns=[4, -1]), "negative n"), ("null ray buffer", dict(rays=[4096, None]), "null buffer"),
                          ("null out buffer", dict(outs=[None, 8192]), "null buffer")):
        rc, err = batch(lib, **dict(dict(count=2, **good), **kw))
        assert rc == capi.KR_EINVAL and msg in err and err.startswith("kr_post_return_map_batch"), (what, rc, err)


def test_empty_batch_is_ok_and_needs_no_device(lib):
    assert lib.kr_post_return_map_batch_dev_f64(0, *PASS, None, None, None, None, None) == capi.KR_OK
    rc, _ = batch(lib, 0, [a_map()], [None], [0], [None])
    assert rc == capi.KR_OK


def test_valid_arguments_reach_the_device_or_say_there_is_none(lib):
    """Without a GPU: KR_ENODEVICE, from every form and from the Python entries (no CPU reducer).  With one: the same calls on empty record sets are KR_OK."""
    gpu = lib.kr_device_count() > 0
    want = capi.KR_OK if gpu else capi.KR_ENODEVICE
    for name, rc, err in calls(lib, a_map(), n=0):
        assert rc == want and (gpu or "no HIP device" in err), (name, rc, err)
    rc, err = batch(lib, 2, [a_map(), a_map()], [None, None], [0, 0], [None, None])
    assert rc == want and (gpu or "no HIP device" in err)
    if not gpu:
        for name, rc, err in calls(lib, a_map()):
            assert rc == capi.KR_ENODEVICE and "no HIP device" in err, (name, rc, err)
        with pytest.raises(capi.KrError, match="no HIP device"):
            api.reduce_return_map(a_map(), np.zeros(4, dtype=capi.RAY_F64))
        with pytest.raises(capi.KrError, match="no HIP device"):
            api.return_radiation(0.998, [6.0], 0.04, 0.04 * np.pi, nr=4)


def test_words_to_dict():
    m = a_map(3)
    words = np.arange(21, dtype=np.float64)
    d = api.return_map_from_words(m, words)
    assert api.return_map_words(m) == 21
    assert d["count"].tolist() == [0, 1, 2] and d["time"].tolist() == [12, 13, 14] and d["ray_count"] == 15 and d["lost"] == 18
    assert d["on_disc"] == 19 and d["binned"] == 20 and np.allclose(d["r_edges"], [1.2, 2.4, 4.8, 9.6])
