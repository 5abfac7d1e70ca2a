"""CPU: the HEALPix point source's rules (tests/healpix_rules.py) against what they restate, and the library's host-side contract.

  geometry    the numpy rule against tests/golden/healpix_vectors.npz -- the reference's own healpix.h at all pixels of orders 0-3 and 512 pixels each of
              orders 8 and 12.  A component may differ by at most 4.5e-16 absolute: both libraries' sin / cos are within 1 ulp, the product rounds
              once more on each side, and the operands are <= 1.
  constants   the rule against the oracle's PointSource on the 354-ray grid of raytrace_rk4_test, basis 0, motion 0,
              v = (sin a cos b, sin a sin b, cos a).  The only inexact inputs are numpy's sin / cos / acos against the C library's; the bound is 16 x the
              worst relative difference measured when the rule was written (profiles/healpix_parity.json holds both numbers; a wrong tetrad entry
              shows as O(1)).
  refusals    everything kr_healpix_source refuses comes back as KR_EINVAL with the field named, before any device is asked for.
  ABI         the ctypes structs against a freshly compiled sizeof / offsetof print of include/kr_trace.h; the ABI version is still 16.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import healpix_rules as hr
import oracle_lib as ol
from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY_ATOL = 4.5e-16


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "healpix_vectors.npz"))
    return z["order"], z["pix"], z["bits"].view(np.float64)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def test_fixture_holds_what_it_should(fixture):
    order, pix, vec = fixture
    assert vec.shape == (2044, 15) and not np.isnan(vec).any()
    for o in range(4):
        assert np.array_equal(pix[order == o], np.arange(hr.npix_of(o)))
    for o in (8, 12):
        p = set(pix[order == o].tolist())
        nside = 1 << o
        npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
        assert len(p) == 512 and {0, ncap - 1, ncap, npix - ncap - 1, npix - ncap, npix - 1} <= p
    corners = vec[:, :12].reshape(-1, 4, 3)
    assert np.abs(np.sqrt((corners * corners).sum(axis=2)) - 1).max() < 1e-15
    centre0 = np.sqrt((vec[order == 0, 12:] ** 2).sum(axis=1))            # not normalised: 0.726-0.777 at order 0
    assert 0.726 < centre0.min() and centre0.max() < 0.778


def test_geometry_rule_matches_reference_vectors(fixture):
    order, pix, vec = fixture
    differ = 0
    for o in np.unique(order):
        m = order == o
        got = hr.pixel_vectors(int(o), pix[m])
        assert np.abs(got - vec[m]).max() <= GEOMETRY_ATOL, f"order {o}"
        differ += int((got.view(np.int64) != vec[m].view(np.int64)).sum())
    print(f"components not bit-identical to the reference's: {differ} of {vec.size}")
    assert differ < vec.size // 100


def test_unit_centre_is_unit(fixture):
    order, pix, _ = fixture
    c = hr.pixel_vectors(3, pix[order == 3], unit_center=True)[:, 12:]
    assert np.abs(np.sqrt((c * c).sum(axis=1)) - 1).max() <= 2.3e-16


def test_constants_rule_matches_oracle_pointsource():
    m = hr.constants_vs_oracle_pointsource()
    assert m["rays"] == 354
    recorded = json.load(open(os.path.join(ROOT, "profiles", "healpix_parity.json")))["constants_rule_vs_oracle_pointsource"]
    print(f"worst relative difference of k, h, Q over {m['live']} rays: {m['worst_rel']:.3e}; recorded {recorded['worst_rel']:.3e}, allowed {recorded['allowed']:.3e}"
          " (python tests/healpix_rules.py measures and records it anew)")
    assert recorded["allowed"] == 16 * recorded["worst_rel"]
    assert m["worst_rel"] <= recorded["allowed"]
    assert m["signs_agree"]


def _spec(**kw):
    a = dict(pos=(0.0, 5.0, 1e-3, 1.5707), V=0.0, spin=0.998, order=3, motion=0, basis=0, rays_per_pixel=5)
    a.update(kw)
    return api.healpix_spec(**a)


REFUSED = [
    ("order-low", dict(order=-1), b"order"),
    ("order-high", dict(order=14), b"order"),
    ("motion", dict(motion=2), b"motion"),
    ("basis", dict(basis=2), b"basis"),
    ("rays-per-pixel", dict(rays_per_pixel=4), b"rays_per_pixel"),
    ("basis-with-radial", dict(motion=1, basis=1, V=0.3), b"basis"),
    ("orbital-not-timelike", dict(pos=(0.0, 6.0, 1.2, 1.5707), V=0.5, spin=0.9), b"V"),
    ("orbital-keplerian-flag", dict(pos=(0.0, 6.0, 1.2, 1.5707), V=-1.0, spin=0.9), b"V"),
    ("orbital-nan", dict(V=float("nan")), b"V"),
    ("radial-not-timelike", dict(motion=1, V=0.9), b"V"),
    ("radial-nan", dict(motion=1, V=float("nan")), b"V"),
    ("energy-zero", dict(E=0.0), b"E must"),
    ("energy-negative", dict(E=-1.0), b"E must"),
    ("energy-nan", dict(E=float("nan")), b"E must"),
    ("disc-source", dict(disc_source=2), b"disc_source"),
]


@pytest.mark.parametrize("case,kw,field", REFUSED, ids=[c[0] for c in REFUSED])
def test_refusals_name_the_field(lib, case, kw, field):
    s = _spec(**kw)
    calls = [lambda: lib.kr_healpix_count(C.byref(s), None),
             lambda: lib.kr_healpix_init_dev_f64(C.byref(s), 0, 1, None, 0, None),
             lambda: lib.kr_healpix_init_emit_dev_f64(C.byref(s), 0, 1, 0, None, 0, None),
             lambda: lib.kr_healpix_init_f64(C.byref(s), None, 0)]
    for call in calls:
        assert call() == capi.KR_EINVAL
        assert field in lib.kr_last_error(), lib.kr_last_error()


def test_argument_checks_come_before_the_device(lib):
    s = _spec()
    npix = C.c_int64()
    assert lib.kr_healpix_count(C.byref(s), C.byref(npix)) == 5 * 768 and npix.value == 768
    assert lib.kr_healpix_count(C.byref(_spec(order=13, rays_per_pixel=1)), C.byref(npix)) == 12 * 4 ** 13 == npix.value
    assert lib.kr_healpix_count(None, None) == capi.KR_EINVAL
    buf = C.c_void_p(64)                                                  # never dereferenced: every call below is refused first
    assert lib.kr_healpix_init_dev_f64(C.byref(s), -1, 1, buf, 5, None) == capi.KR_EINVAL and b"first/stride" in lib.kr_last_error()
    assert lib.kr_healpix_init_dev_f64(C.byref(s), 0, 0, buf, 5, None) == capi.KR_EINVAL
    assert lib.kr_healpix_init_dev_f64(C.byref(s), 0, 1, buf, 5 * 768 + 1, None) == capi.KR_EINVAL and b"beyond the sphere" in lib.kr_last_error()
    assert lib.kr_healpix_init_emit_dev_f64(C.byref(s), 767, 2, 0, buf, 6, None) == capi.KR_EINVAL
    assert lib.kr_healpix_init_dev_f64(C.byref(s), 0, 1, buf, -1, None) == capi.KR_EINVAL
    assert lib.kr_healpix_init_f64(C.byref(s), buf, 5 * 768 - 1) == capi.KR_EINVAL
    assert lib.kr_healpix_vectors_dev_f64(14, 0, 0, 1, 1, buf, None) == capi.KR_EINVAL and b"order" in lib.kr_last_error()
    assert lib.kr_healpix_vectors_dev_f64(3, 0, 768, 1, 1, buf, None) == capi.KR_EINVAL
    assert lib.kr_healpix_vectors_dev_f64(3, 0, 0, 1, 769, buf, None) == capi.KR_EINVAL
    m = api.healpix_map_struct(768, 1.2, 500.0, 1000.0)
    assert lib.kr_post_healpix_map_dev_f64(0.9, -1.0, 0, 0, 0, -np.pi, np.pi, None, buf, 5, 0, 1, buf, None) == capi.KR_EINVAL
    assert lib.kr_reduce_healpix_map_dev_f64(C.byref(m), buf, 7, 0, 1, buf, None) == capi.KR_EINVAL and b"multiple" in lib.kr_last_error()
    assert lib.kr_reduce_healpix_map_dev_f64(C.byref(m), buf, 5 * 769, 0, 1, buf, None) == capi.KR_EINVAL
    assert lib.kr_reduce_healpix_map_dev_f64(C.byref(m), buf, 10, 767, 1, buf, None) == capi.KR_EINVAL
    m.rays_per_pixel = 2
    assert lib.kr_reduce_healpix_map_f64(C.byref(m), buf, 10, buf) == capi.KR_EINVAL and b"rays_per_pixel" in lib.kr_last_error()
    m.rays_per_pixel, m.npix = 1, 0
    assert lib.kr_reduce_healpix_map_f64(C.byref(m), buf, 10, buf) == capi.KR_EINVAL and b"npix" in lib.kr_last_error()


ABI_PRINT = r"""
#include <stddef.h>
#include <stdio.h>
#include "kr_trace.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void)
{
    printf("abi %d\n", KR_ABI_VERSION);
    printf("kr_healpix_source %zu\n", sizeof(kr_healpix_source));
    F(kr_healpix_source, pos); F(kr_healpix_source, V); F(kr_healpix_source, spin); F(kr_healpix_source, E); F(kr_healpix_source, order);
    F(kr_healpix_source, motion); F(kr_healpix_source, basis); F(kr_healpix_source, rays_per_pixel); F(kr_healpix_source, unit_center); F(kr_healpix_source, disc_source);
    printf("kr_healpix_map %zu\n", sizeof(kr_healpix_map));
    F(kr_healpix_map, r_isco); F(kr_healpix_map, r_disc); F(kr_healpix_map, r_esc); F(kr_healpix_map, theta_tol); F(kr_healpix_map, source_r);
    F(kr_healpix_map, source_phi); F(kr_healpix_map, q1); F(kr_healpix_map, rb1); F(kr_healpix_map, q2); F(kr_healpix_map, rb2); F(kr_healpix_map, q3);
    F(kr_healpix_map, npix); F(kr_healpix_map, rays_per_pixel); F(kr_healpix_map, self_zone);
    return 0;
}
"""


def test_struct_layouts_match_a_compiled_print(lib, tmp_path):
    src, exe = tmp_path / "abi_print.c", tmp_path / "abi_print"
    src.write_text(ABI_PRINT)
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    want = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(want.pop("abi")) == 16 == capi.ABI_VERSION == lib.kr_abi_version()
    got = {}
    for name, T in (("kr_healpix_source", capi.HealpixSource), ("kr_healpix_map", capi.HealpixMap)):
        got[name] = str(C.sizeof(T))
        got.update({f"{name}.{f}": str(getattr(T, f).offset) for f, _ in T._fields_})
    assert got == want
