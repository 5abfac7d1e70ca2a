"""CPU: the volume-map entry points (kr_trace_volume_*) are additive -- the ABI version and the pinned struct sizes stay -- and refuse every bad
argument before they touch a device; the numpy rule the GPU tests hold the kernel to (tests/volume_map_rules.py) bins hand-built rows into the
cells they were built for; api.cell_volume is the reference's sqrt(-g_rr g_thth g_phph) dr dtheta dphi."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import volume_map_rules as vr
from raytrace_cpu_amd import api, capi


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_abi_version_and_struct_sizes(lib):
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "kr_trace.h")).read()
    size = int(re.search(r"static_assert\(sizeof\(kr_volume_map\) == (\d+)", header).group(1))
    assert C.sizeof(capi.VolumeMap) == size == 72
    assert [capi.VolumeMap.__dict__[f].offset for f in ("r_min", "dr", "dtheta", "dphi", "V", "nr", "ntheta", "nphi", "logbin", "mode", "reverse", "projradius", "motion")] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64, 68]
    assert capi.ABI_VERSION == 16 and lib.kr_abi_version() == 16
    assert C.sizeof(capi.Params) == 128 and C.sizeof(capi.Stats) == 136


def _grid(**kw):
    m = api.volume_map_struct(1.2, 40.0, 24, 16, 1, False)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _calls(lib, p, m, n=4, null=()):
    """the host-pointer and the device-pointer form (with never-dereferenced non-null pointers); -> [(rc, message), (rc, message)]"""
    rays = np.zeros(max(n, 1), dtype=capi.RAY_F64)
    words = np.zeros(api.volume_words(m) if 0 < m.nr * m.ntheta * m.nphi < 1 << 20 else 16)
    fake = C.c_void_p(4096)
    pp = None if "p" in null else C.byref(p)
    mm = None if "m" in null else C.byref(m)
    rc1 = lib.kr_trace_volume_f64(pp, mm, None if "rays" in null else rays.ctypes.data_as(C.c_void_p), n, None if "map" in null else words.ctypes.data_as(C.c_void_p), None)
    e1 = lib.kr_last_error().decode()
    rc2 = lib.kr_trace_volume_dev_f64(pp, mm, None if "rays" in null else fake, n, None if "map" in null else fake, None, None)
    e2 = lib.kr_last_error().decode()
    assert (rays["r"] == 0).all() and (words == 0).all()
    return [(rc1, e1), (rc2, e2)]


REFUSALS = [
    ("nr 0", dict(), dict(nr=0), "at least 1"),
    ("ntheta 0", dict(), dict(ntheta=0), "at least 1"),
    ("nphi negative", dict(), dict(nphi=-2), "at least 1"),
    ("too many cells", dict(), dict(nr=1024, ntheta=1024, nphi=129), "more than 2^27 cells"),
    ("dr 0", dict(), dict(dr=0.0), "positive and finite"),
    ("dr negative", dict(), dict(dr=-1.0), "positive and finite"),
    ("dr NaN", dict(), dict(dr=float("nan")), "positive and finite"),
    ("dtheta inf", dict(), dict(dtheta=float("inf")), "positive and finite"),
    ("dtheta 0", dict(), dict(dtheta=0.0), "positive and finite"),
    ("dphi NaN", dict(), dict(dphi=float("nan")), "positive and finite"),
    ("dphi negative", dict(), dict(dphi=-0.1), "positive and finite"),
    ("log dr 1", dict(), dict(logbin=1, dr=1.0), "needs dr > 1"),
    ("log dr below 1", dict(), dict(logbin=1, dr=0.5), "needs dr > 1"),
    ("log r_min 0", dict(), dict(logbin=1, dr=1.1, r_min=0.0), "needs r_min > 0"),
    ("log r_min negative", dict(), dict(logbin=1, dr=1.1, r_min=-1.0), "needs r_min > 0"),
    ("mode 2", dict(), dict(mode=2), "unknown mode"),
    ("mode -1", dict(), dict(mode=-1), "unknown mode"),
    ("motion 2", dict(), dict(motion=2), "unknown motion"),
    ("fast math", dict(flags=capi.FLAG_FAST_MATH), dict(), "KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted"),
    ("hybrid", dict(flags=capi.FLAG_HYBRID), dict(), "KR_FLAG_FAST_MATH / KR_FLAG_HYBRID are not accepted"),
    ("rk45", dict(integrator=capi.RK45), dict(), "RK45"),
    ("euler + destination", dict(integrator=capi.EULER, stop_kind=capi.STOP_FLATDISC), dict(), "Integrator::Euler does not support RayDestination stopping conditions"),
]


@pytest.mark.parametrize("what,pkw,mkw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_device_work(lib, what, pkw, mkw, msg):
    p = capi.copy_params(capi.default_params(0.998), **pkw)
    m = _grid(**mkw)
    for rc, err in _calls(lib, p, m):
        assert rc == capi.KR_EINVAL and msg in err and err.startswith("kr_trace_volume:"), (rc, err)


def test_null_pointers_and_negative_n_are_refused(lib):
    p, m = capi.default_params(0.998), _grid()
    for null in ("p", "m", "rays", "map"):
        for rc, err in _calls(lib, p, m, null=(null,)):
            assert rc == capi.KR_EINVAL and "null argument" in err, (null, rc, err)
    for rc, err in _calls(lib, p, m, n=-1):
        assert rc == capi.KR_EINVAL and "negative n" in err, (rc, err)


def test_a_valid_call_needs_a_device(lib):
    """(the refusals above are not an artefact of a missing device: a valid call gets past them)"""
    if lib.kr_device_count() > 0:
        return
    p, m = capi.copy_params(capi.default_params(0.998), integrator=capi.RK4), _grid(mode=1, logbin=1, dr=1.2)
    for rc, err in _calls(lib, p, m):
        assert rc == capi.KR_ENODEVICE and "no HIP device" in err
    with pytest.raises(capi.KrError, match="no HIP device"):
        api.trace_volume(p, np.zeros(4, dtype=capi.RAY_F64), m)


def test_struct_has_the_mapper_constructors_bin_widths():
    m = api.volume_map_struct(1.5, 100.0, 11, 7, 9, True)
    assert m.dr == math.exp(math.log(100.0 / 1.5) / 10) and m.dtheta == (math.pi / 2) / 6 and m.dphi == (2 * math.pi) / 8
    assert (m.nr, m.ntheta, m.nphi, m.logbin, m.mode, m.V, m.projradius, m.motion, m.reverse) == (11, 7, 9, 1, 0, -1.0, 1, 0, 0)
    m = api.volume_map_struct(1.5, 100.0, 11, 7, 1, False, mode=1)
    assert m.dr == (100.0 - 1.5) / 10 and m.dphi == 2 * math.pi and m.mode == 1      # (one cell in phi: the whole circle)


# ---- the rule on hand-built rows: r in [1, 3) in 4 cells of 0.5, theta in [0, 1) in 4 cells of 0.25, phi in 4 cells of pi / 2 from -pi ------------
def _small(mode, nphi=4):
    m = capi.VolumeMap()
    m.r_min, m.dr, m.dtheta, m.dphi, m.V = 1.0, 0.5, 0.25, np.pi / 2, -1.0
    m.nr, m.ntheta, m.nphi, m.logbin, m.mode, m.reverse, m.projradius, m.motion = 4, 4, nphi, 0, mode, 0, 1, 0
    return m


def _cell(ir, ith, iph, m):
    return (ir * m.ntheta + ith) * m.nphi + iph


def _bin(m, per_ray_rows, g=None):
    """per_ray_rows: a list of lists of (t, r, theta, phi); g: per row (default 1.0 everywhere)"""
    rows = np.array([row for ray in per_ray_rows for row in ray], dtype=np.float64).reshape(-1, 4)
    offsets = np.concatenate([[0], np.cumsum([len(ray) for ray in per_ray_rows])])
    g = np.ones(len(rows)) if g is None else np.asarray(g, dtype=np.float64)
    return vr.bin_rows(m, offsets, rows, lambda due: g[due])


def test_rule_cells_at_the_edges():
    m = _small(mode=1)
    under = np.nextafter(3.0, 0.0)
    rows = [(1.0, 1.5, 0.3, 0.1),                 # exactly on a radial edge: q_r = 1 -> ir = 1;  ith = 1;  (0.1 + pi) / (pi / 2) = 2.06 -> iph = 2
            (2.0, 1.0, 0.0, -np.pi),              # q = 0 on every axis: cell 0 is a cell
            (3.0, under, 0.1, 0.0),               # just under n: ir = 3
            (4.0, 3.0, 0.1, 0.0),                 # q_r = n: outside
            (5.0, float("nan"), 0.1, 0.0),        # NaN: outside, and no error
            (6.0, 1.2, float("nan"), 0.0),
            (7.0, 1.2, 0.1, float("inf")),
            (8.0, 1.2, np.nextafter(1.0, 0.0), 0.0),   # theta just under ntheta dtheta: ith = 3
            (9.0, 1.2, 1.0, 0.0),                 # on it: outside
            (10.0, np.nextafter(1.0, 0.0), 0.1, 0.0),  # q_r just under 0: outside (no (-1, 0] band)
            (11.0, 1.2, 0.1, np.pi),              # phi = pi wraps to -pi: iph = 0
            (12.0, 1.2, 0.1, -np.pi),
            (13.0, 1.2, 0.1, 3 * np.pi)]
    cell = vr.cells_of(m, np.array(rows))
    assert cell.tolist() == [_cell(1, 1, 2, m), 0, _cell(3, 0, 2, m), -1, -1, -1, -1, _cell(0, 3, 2, m), -1, -1, _cell(0, 0, 0, m), _cell(0, 0, 0, m), _cell(0, 0, 0, m)]
    got = _bin(m, [rows])
    assert (got["rows"], got["in_grid"], got["deposits"], got["bad_g"]) == (13, 7, 7, 0)
    want = np.zeros(64)
    for c, t in zip(cell, [r[0] for r in rows]):
        if c >= 0:
            want[c] += 1
    assert np.array_equal(got["count"].ravel(), want) and got["count"].shape == (4, 4, 4)
    assert got["count"].ravel()[0] == 4 and got["time"].ravel()[0] == 2.0 + 11.0 + 12.0 + 13.0
    assert got["time"].sum() == 1.0 + 2.0 + 3.0 + 8.0 + 11.0 + 12.0 + 13.0


def test_rule_axisymmetric_map_makes_no_phi_test():
    m = _small(mode=1, nphi=1)
    rows = [(1.0, 1.2, 0.1, float("nan")), (2.0, 1.2, 0.1, 1e6), (3.0, 1.7, 0.6, -17.0)]
    assert vr.cells_of(m, np.array(rows)).tolist() == [0, 0, 1 * 4 + 2]


def test_rule_passage_and_every_row():
    a, b = (1.2, 0.1, 0.0), (1.7, 0.1, 0.0)           # cells A = (0, 0, 2) and B = (1, 0, 2)
    out = (5.0, 0.1, 0.0)
    ray1 = [(1.0, *a), (2.0, *a), (3.0, *a),           # held for three rows: once in passage mode
            (4.0, *b),                                 # a new cell
            (5.0, *out), (6.0, *b),                    # re-entry after leaving the grid: counted again
            (7.0, *a), (8.0, *b)]                      # and after another cell
    ray2 = [(9.0, *b), (10.0, *b)]                     # the next ray starts with last_cell = -1: B counts although ray 1 ended in B
    m0, m1 = _small(0), _small(1)
    A, B = _cell(0, 0, 2, m0), _cell(1, 0, 2, m0)
    p = _bin(m0, [ray1, [], ray2])
    assert p["count"].ravel()[A] == 2 and p["count"].ravel()[B] == 4 and p["count"].sum() == 6
    assert p["time"].ravel()[A] == 1.0 + 7.0 and p["time"].ravel()[B] == 4.0 + 6.0 + 8.0 + 9.0
    assert (p["rows"], p["in_grid"], p["deposits"], p["bad_g"]) == (10, 9, 6, 0)
    e = _bin(m1, [ray1, [], ray2])
    assert e["count"].ravel()[A] == 4 and e["count"].ravel()[B] == 5 and e["count"].sum() == 9
    assert (e["rows"], e["in_grid"], e["deposits"], e["bad_g"]) == (10, 9, 9, 0)


def test_rule_a_bad_g_consumes_the_passage():
    a, b = (1.2, 0.1, 0.0), (1.7, 0.1, 0.0)
    ray = [(1.0, *a), (2.0, *a), (3.0, *b), (4.0, *b), (5.0, *a)]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        g = [bad, 2.0, 3.0, bad, 0.5]
        m0 = _small(0)
        A, B = _cell(0, 0, 2, m0), _cell(1, 0, 2, m0)
        p = _bin(m0, [ray], g)
        # row 0 is the passage of A and its g is bad: nothing deposits, and row 1 (same cell) is no new passage
        assert p["count"].ravel()[A] == 1 and p["count"].ravel()[B] == 1 and (p["deposits"], p["bad_g"]) == (2, 1)
        assert p["redshift"].ravel()[A] == 0.5 and p["redshift"].ravel()[B] == 3.0 and p["time"].ravel()[A] == 5.0
        e = _bin(_small(1), [ray], g)
        assert e["count"].ravel()[A] == 2 and e["count"].ravel()[B] == 1 and (e["deposits"], e["bad_g"]) == (3, 2)
        assert e["redshift"].ravel()[A] == 2.5


def test_rule_radial_sign_is_the_direction_the_row_moved():
    m = _small(0)
    m.motion = 1
    init = np.zeros(2, dtype=capi.RAY_F64)
    init["r"] = [2.0, 1.0]
    rows = np.array([(0, 1.9, 0, 0), (0, 1.8, 0, 0), (0, 1.85, 0, 0), (0, 1.5, 0, 0)], dtype=np.float64)
    rd, td = vr.signs_for(m, init, np.array([0, 3, 4]), rows)
    assert rd.tolist() == [-1, -1, 1, 1] and td.tolist() == [1, 1, 1, 1]
    with pytest.raises(AssertionError, match="did not move"):
        vr.signs_for(m, init, np.array([0, 3, 4]), np.array([(0, 1.9, 0, 0), (0, 1.9, 0, 0), (0, 1.85, 0, 0), (0, 1.5, 0, 0)], dtype=np.float64))


def test_log_grid_cells():
    m = api.volume_map_struct(2.0, 2.0 * 1.5 ** 5, 6, 3, 1, True)
    assert abs(m.dr - 1.5) < 1e-15
    m.dr = 1.5
    r = 2.0 * 1.5 ** np.arange(6) * 1.2            # inside cell i by construction: 1 < 1.2 < 1.5
    rows = np.stack([np.zeros(6), r, np.full(6, 0.1), np.zeros(6)], axis=1)
    assert vr.cells_of(m, rows).tolist() == [i * 3 for i in range(6)]
    assert vr.cells_of(m, np.array([[0, 1.9, 0.1, 0], [0, 2.0 * 1.5 ** 6 * 1.01, 0.1, 0], [0, 0.0, 0.1, 0], [0, -1.0, 0.1, 0]], dtype=np.float64)).tolist() == [-1] * 4


def test_cell_volume_closed_form_at_zero_spin():
    """Mapper::calculate_volume at a = 0: sqrt(-g_rr g_thth g_phph) = sqrt((r^2 / (r^2 - 2 r)) r^2 r^2 sin^2 theta) = r^2 sin(theta) / sqrt(1 - 2 / r)
    at the cell's lower corner, times dr dtheta dphi -- the proper volume of the Schwarzschild slice, which tends to the flat r^2 sin(theta) dr dtheta dphi
    as 2 / r -> 0 (checked separately, at r >= 1e6, to the size of that factor)."""
    for logbin in (False, True):
        m = api.volume_map_struct(3.0, 60.0, 9, 7, 5, logbin)
        v = api.cell_volume(m, 0.0)
        assert v.shape == (9, 7, 5)
        i = np.arange(9.0)
        r = (3.0 * m.dr ** i if logbin else 3.0 + m.dr * i)[:, None, None]
        dr = r * (m.dr - 1) if logbin else m.dr
        th = (np.arange(7.0) * m.dtheta)[None, :, None]
        want = r * r * np.sin(th) / np.sqrt(1 - 2 / r) * dr * m.dtheta * m.dphi * np.ones((1, 1, 5))
        assert np.allclose(v, want, rtol=1e-13, atol=0) and (v[:, 0, :] == 0).all() and (v[:, 1:, :] > 0).all()
    far = api.volume_map_struct(1e6, 2e6, 5, 4, 3, False)
    v = api.cell_volume(far, 0.0)
    r = (1e6 + far.dr * np.arange(5.0))[:, None, None]
    flat = r * r * np.sin(np.arange(4.0) * far.dtheta)[None, :, None] * far.dr * far.dtheta * far.dphi * np.ones((1, 1, 3))
    assert np.allclose(v, flat, rtol=1.5e-6, atol=0)          # 1 / sqrt(1 - 2 / r) - 1 = 1e-6 at r = 1e6
    # and with spin it is the reference's expression, term for term
    m = api.volume_map_struct(2.0, 30.0, 6, 5, 1, False)
    a, r, th = 0.9, 2.0 + m.dr * 3, 2 * m.dtheta
    rhosq, delta = r * r + (a * math.cos(th)) ** 2, r * r - 2 * r + a * a
    sigmasq = (r * r + a * a) ** 2 - a * a * delta * math.sin(th) ** 2
    want = math.sqrt(-1 * (-rhosq / delta) * (-rhosq) * (-(sigmasq * math.sin(th) ** 2 / rhosq))) * m.dr * m.dtheta * m.dphi
    assert abs(api.cell_volume(m, a)[3, 2, 0] / want - 1) < 1e-14
