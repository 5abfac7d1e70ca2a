"""CPU: the device-resident pipelines of api.py, run against a recording stand-in for libkrtrace.  Two things are pinned.
1. The sequence of library calls (entry point, byte counts, which buffer and offset every device pointer is, the integer arguments) is the one
   recorded in tests/golden/api_call_traces.json, every buffer is freed exactly once, and none is freed later relative to the other calls.
2. Whichever call fails, the function raises KrError and every buffer handed out so far has been freed exactly once.
The stand-in fills what kr_memcpy_d2h reads back with 0, 1, 2, .., so the golden file also pins what each pipeline makes of its result buffers
(key order, dtype, shape and sums).  The golden file was recorded from the hand-written allocation code, before the pipelines moved onto
raytrace_cpu_amd/devmem.py; `PYTHONPATH=. python tests/test_api_device_calls.py --record` rewrites it from the code as it is."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from raytrace_cpu_amd import api, capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_call_traces.json")
HOST_ONLY = ("kr_kerr_isco", "kr_disc_velocity", "kr_kerr_horizon", "kr_params_default")      # and every kr_*_count: answered by the real library
HBM_BYTES = 16384
BASE, STRIDE = 1 << 32, 1 << 24
_CArg = type(C.byref(C.c_int()))


class FakeLib:
    """Every entry point of capi.PROTOTYPES: returns KR_OK and logs [name, arg, ..]; the fail_at-th logged call returns KR_EHIP instead."""

    def __init__(self, real, fail_at=None, int32_copies=()):
        self.real, self.fail_at, self.int32_copies = real, fail_at, set(int32_copies)
        self.log, self.allocs, self.frees, self.calls = [], [], {}, 0
        for name in capi.PROTOTYPES:
            if name in HOST_ONLY or name.endswith("_count"):
                setattr(self, name, getattr(real, name))
            elif not hasattr(type(self), name):
                setattr(self, name, lambda *a, _n=name: self._call(_n, a))

    def kr_last_error(self):
        return b"injected"

    def _where(self, addr):
        if not addr:
            return None
        for i, (base, nbytes) in enumerate(self.allocs):
            if base <= addr < base + max(nbytes, 1):
                return [i, addr - base] if i not in self.frees else ["freed", i, addr - base]
        return "host"

    def _arg(self, a):
        if isinstance(a, np.generic):
            a = a.item()
        if a is None or isinstance(a, (bool, int, float)):
            return a
        if isinstance(a, C.c_void_p):
            return self._where(a.value)
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                return [self._where(v) for v in a]
            return list(a) if a._type_ in (C.c_int64, C.c_double) else f"{a._type_.__name__}[{len(a)}]"
        return "ref" if isinstance(a, _CArg) else type(a).__name__

    def _call(self, name, args, effect=None):
        k, self.calls = self.calls, self.calls + 1
        self.log.append([name] + [self._arg(a) for a in args])
        if k == self.fail_at:
            self.failed = len(self.log) - 1
            return capi.KR_EHIP
        if effect:
            effect()
        return capi.KR_OK

    def kr_malloc(self, ref, nbytes):
        def hand_out():
            ref._obj.value = BASE + STRIDE * len(self.allocs)
            self.allocs.append((ref._obj.value, nbytes))
        return self._call("kr_malloc", (ref, nbytes), hand_out)

    def kr_free(self, d):
        where = self._where(d.value)
        self.log.append(["kr_free", where])
        assert isinstance(where, list) and where[0] != "freed" and where[1] == 0, f"kr_free of {where}"
        self.frees[where[0]] = len([e for e in self.log if e[0] != "kr_free"])       # the calls that came before it
        return capi.KR_OK

    def kr_device_info(self, cus, khz, mem, name, size):
        def fill():
            mem._obj.value = HBM_BYTES
        return self._call("kr_device_info", (), fill)

    def kr_trace_volume_dev_f64(self, *a):
        def count_rays():
            a[-1]._obj.rays_traced = a[3]
        return self._call("kr_trace_volume_dev_f64", a, count_rays)

    def kr_memcpy_d2h(self, dst, src, nbytes):
        def fill():
            if nbytes in self.int32_copies:
                a = np.arange(nbytes // 4, dtype=np.int32) % 3
            else:
                a = np.arange(nbytes // 8, dtype=np.float64)
            C.memmove(dst, a.ctypes.data, a.nbytes)
        return self._call("kr_memcpy_d2h", (dst, src, nbytes), fill)


def _plane(n=3):
    s = capi.ImagePlaneSpec()
    s.dist, s.inc_deg, s.spin, s.phi0, s.precision = 100.0, 60.0, 0.9, 0.0, 100.0
    s.x0, s.xmax, s.dx, s.y0, s.ymax, s.dy = -3.0, 3.0, 6.0 / n, -2.0, 2.0, 2.0
    return s


def _source(r=6.0):
    return api.return_radiation_sources(0.9, [r], 0.9, 1.2)[0]


def _emis_bins(nr):
    b = capi.EmisBins()
    b.r_min, b.dr, b.r_isco, b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = 1.3, 1.5, 1.3, 2.0, 0.9, 10.0, nr, 1
    return b


def _image_bins():
    ib = capi.ImageBins()
    ib.x0, ib.y0, ib.img_dx, ib.img_dy, ib.r_isco, ib.r_disc, ib.img_nx, ib.img_ny, ib.flip_image = -3.0, -2.0, 3.0, 2.0, 1.3, 50.0, 2, 3, 1
    return ib


def _line_bins():
    return capi.line_bins(ne=3, nt=2, dt=5.0, r_isco=1.3, r_disc=50.0)


def _params():
    return capi.copy_params(capi.default_params(-0.9), integrator=capi.RK4)


def _volume():
    return api.volume_map_struct(1.5, 20.0, 3, 2, 4, True)


def _healpix(rays_per_pixel=5):
    return api.healpix_spec((0.0, 5.0, 0.3, 0.0), 0.0, 0.9, 0, rays_per_pixel=rays_per_pixel)


def _healpix_map(rays_per_pixel, **kw):
    return api.healpix_map(_healpix(rays_per_pixel), _params(), api.healpix_map_struct(12, 1.3, 50.0, 100.0, rays_per_pixel=rays_per_pixel), **kw)


def _crossing_inputs():
    n, M = 4, 2
    return np.zeros(n, dtype=capi.RAY_F64), np.zeros((n, M, 4)), np.zeros(n, dtype=np.int32)


RR = dict(dcosalpha=0.9, dbeta=1.2, r_disc=50.0, r_esc=100.0, nr=3)
# name -> (call, the byte counts whose read-back is int32)
CASES = {
    "return_radiation": (lambda: api.return_radiation(0.9, [4.0, 6.0, 9.0], **RR), ()),
    "return_radiation_records": (lambda: api.return_radiation(0.9, [4.0, 6.0, 9.0], return_records=True, logbin=True, **RR), ()),
    "return_radiation_no_sources": (lambda: api.return_radiation(0.9, [], **RR), ()),
    "line_profile_rays": (lambda: api.line_profile(_plane(), _params(), _line_bins(), mode="rays"), ()),
    "line_profile_pixels": (lambda: api.line_profile(_plane(), _params(), _line_bins(), mode="pixels"), ()),
    "line_profile_pixels_own_bins": (lambda: api.line_profile(_plane(), _params(), _line_bins(), mode="pixels", image_bins=_image_bins()), ()),
    "line_profile_limb": (lambda: api.line_profile(_plane(), _params(), _line_bins(), limb="laor"), ()),
    "arrival_angles_dev": (lambda: api.arrival_angles((C.c_void_p(4096), 5), 0.9), ()),
    "arrival_angles_dev_int_pointer": (lambda: api.arrival_angles((4096, 5), 0.9, 0.5, 1, 1), ()),
    "arrival_angles_dev_empty": (lambda: api.arrival_angles((4096, 0), 0.9), ()),
    "emissivity_angles": (lambda: api.emissivity_angles(_source(), _params(), _emis_bins(3), 2), ()),
    "emissivity_angles_nmu0": (lambda: api.emissivity_angles(_source(), _params(), _emis_bins(3), 0), ()),
    "caustic_map_bundles": (lambda: api.caustic_map(_plane(), 50.0), ()),
    "caustic_map_grid": (lambda: api.caustic_map(_plane(), 50.0, eps_frac=0), ()),
    "caustic_source_sphere": (lambda: api.caustic_source_map(_plane(), "sphere"), ()),
    "caustic_source_plane_bundles": (lambda: api.caustic_source_map(_plane(), "plane"), ()),
    "caustic_source_plane_grid": (lambda: api.caustic_source_map(_plane(), "plane", eps_frac=0), ()),
    "volume_map": (lambda: api.volume_map([_source(4.0), _source(6.0)], _params(), _volume()), ()),
    "volume_spectrum": (lambda: api.volume_spectrum([_source()], _plane(), _params(), _params(), _volume(), api.observe_bins_struct(0.5, 1.5, 3, tmax=10.0, nt=2)), ()),
    "volume_spectrum_kappa": (lambda: api.volume_spectrum([_source()], _plane(), _params(), _params(), _volume(), api.observe_bins_struct(0.5, 1.5, 3),
                                                          kappa=np.ones((3, 2, 4))), ()),
    "reduce_crossing_image": (lambda: api.reduce_crossing_image(_image_bins(), *_crossing_inputs(), order=1), ()),
    "order_images": (lambda: api.order_images(_plane(), _params(), _image_bins(), api.crossing_spec(2), [0, -1]), (12 * 4,)),
    "healpix_vectors": (lambda: api.healpix_vectors(0), ()),
    "healpix_vectors_strided": (lambda: api.healpix_vectors(1, first_pix=3, stride=5), ()),
    "healpix_vectors_empty": (lambda: api.healpix_vectors(0, count=0), ()),
    "healpix_init_emit": (lambda: api.healpix_init(_healpix(), emit=True, reverse=1), ()),
    "healpix_init_plain": (lambda: api.healpix_init(_healpix(1), emit=False, first=1, stride=2), ()),
    "healpix_map": (lambda: _healpix_map(5), ()),
    "healpix_map_records": (lambda: _healpix_map(1, return_records=True), ()),
}


def _summary(v):
    """What a pipeline returned, in a form JSON holds: key order, dtypes, shapes and sums."""
    if isinstance(v, dict):
        return {"dict": [[k, _summary(x)] for k, x in v.items() if k not in ("maps", "specs")]}
    if isinstance(v, (list, tuple)):
        return {type(v).__name__: [_summary(x) for x in v]}
    if isinstance(v, np.ndarray):
        nums = v.view(np.float64) if v.dtype.names else v
        nums = np.asarray(nums, dtype=np.float64).ravel()
        with np.errstate(invalid="ignore"):
            sums = [float(np.nansum(nums)), float(np.nansum(nums * np.arange(1, nums.size + 1)))]      # the second tells a permutation
        return {"array": [str(v.dtype) if not v.dtype.names else "record", list(v.shape), sums, int(np.isnan(nums).sum())]}
    return {type(v).__name__: None if v is None else v if not isinstance(v, np.generic) else v.item()}


@functools.lru_cache(None)
def _real():
    return capi.load()


def _run(monkeypatch, name, fail_at=None):
    call, int32_copies = CASES[name]
    fake = FakeLib(_real(), fail_at, int32_copies)
    monkeypatch.setattr(api, "_lib", fake)
    return fake, call


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_cases_take_the_branches_they_name(monkeypatch):
    fake, call = _run(monkeypatch, "return_radiation")
    call()
    batches = [e[1] for e in fake.log if e[0] == "kr_post_return_map_batch_dev_f64"]
    assert batches == [2, 1], "three radii must run as a group of two and a group of one"
    assert api.imageplane_count(_plane()) == (12, 4, 3)


@pytest.mark.parametrize("name", list(CASES))
def test_same_calls_as_recorded(monkeypatch, golden, name):
    fake, call = _run(monkeypatch, name)
    result = _summary(call())
    want = golden[name]
    calls = lambda log: [e for e in log if e[0] != "kr_free"]      # noqa: E731
    assert json.loads(json.dumps(calls(fake.log))) == calls(want["log"])
    assert json.loads(json.dumps(result)) == want["result"]
    assert sorted(fake.frees) == list(range(len(fake.allocs))), "every buffer is freed exactly once"
    for i, at in fake.frees.items():
        assert at <= want["frees"][str(i)], f"buffer {i} is freed after call {at}, was after call {want['frees'][str(i)]}"


@pytest.mark.parametrize("name", list(CASES))
def test_nothing_leaks_when_a_call_fails(monkeypatch, golden, name):
    ncalls = len([e for e in golden[name]["log"] if e[0] != "kr_free"])
    for k in range(ncalls):
        fake, call = _run(monkeypatch, name, fail_at=k)
        with pytest.raises(capi.KrError):
            call()
        assert sorted(fake.frees) == list(range(len(fake.allocs))), f"call {k} ({fake.log[-1][0]}) failed: a buffer leaked"
        if fake.log[fake.failed][0] == "kr_post_return_map_batch_dev_f64":
            assert fake.log[fake.failed + 1][0] == "kr_trace_wait_many", "the tickets are retired whatever the pass said"


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--record"]:
        out = {}
        for case in CASES:
            lib = FakeLib(_real(), None, CASES[case][1])
            api._lib = lib
            res = _summary(CASES[case][0]())
            out[case] = {"log": lib.log, "frees": lib.frees, "result": res}
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=0, separators=(",", ":"))
            f.write("\n")
