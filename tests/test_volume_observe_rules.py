"""CPU: the numpy rule the GPU tests hold kr_trace_observe_* to (tests/volume_observe_rules.py) on hand-built rows, against closed forms: the proper
length of a radial step at a = 0, the optically thin and the absorbed line integral, the dropped polar-reflection row, absorption without emission,
the order of the rule on a bad energy shift, and the bins."""
import math

import numpy as np

import volume_observe_rules as vo
from raytrace_cpu_amd import api, capi


def _grid(nr=4, ntheta=1, nphi=1, r_min=2.0, dr=10.0):
    """nr radial cells of dr from r_min, one polar cell [0, pi), one azimuthal cell"""
    m = capi.VolumeMap()
    m.r_min, m.dr, m.dtheta, m.dphi, m.V = r_min, dr, np.pi / ntheta, 2 * np.pi / nphi, 0.0
    m.nr, m.ntheta, m.nphi, m.logbin, m.mode, m.reverse, m.projradius, m.motion = nr, ntheta, nphi, 0, 0, 1, 0, 0
    return m


def _measure(m, spin, per_ray, starts, emis, kappa=None, delay=None, z=1.0):
    """per_ray: a list of lists of (t, r, theta, phi); starts: (r, theta, phi) per ray; z: a scalar or one value per row"""
    rows = np.array([row for ray in per_ray for row in ray], dtype=np.float64).reshape(-1, 4)
    offsets = np.concatenate([[0], np.cumsum([len(ray) for ray in per_ray])])
    zz = np.full(len(rows), z, dtype=np.float64) if np.isscalar(z) else np.asarray(z, dtype=np.float64)
    return vo.measure(m, spin, offsets, rows, np.asarray(starts, dtype=np.float64), lambda which: zz[which], emis, kappa, delay)


def test_radial_step_at_zero_spin_has_the_schwarzschild_length():
    """a = 0, a purely radial two-row ray: l = dr / sqrt(1 - 2 / r) at the row"""
    m = _grid()
    th = 1.0
    ray = [(1.0, 9.5, th, 0.3), (2.0, 9.0, th, 0.3)]
    got = _measure(m, 0.0, [ray], [(10.0, th, 0.3)], np.ones(4))
    want = [0.5 / math.sqrt(1 - 2 / 9.5), 0.5 / math.sqrt(1 - 2 / 9.0)]
    assert np.allclose(got["len"], want, rtol=1e-15, atol=0)
    assert (got["rows"], got["in_grid"], got["lit"], got["contributions"], got["bad_g"], got["degenerate"]) == (2, 2, 2, 2, 0, 0)
    # and the angular terms at a = 0: r dtheta and r sin(theta) dphi
    ang = _measure(m, 0.0, [[(1.0, 9.0, th + 0.01, 0.3), (2.0, 9.0, th + 0.01, 0.32)]], [(9.0, th, 0.3)], np.ones(4))
    assert np.allclose(ang["len"], [9.0 * 0.01, 9.0 * math.sin(th + 0.01) * 0.02], rtol=1e-12, atol=0)


def test_kerr_length_is_the_metric_term_for_term():
    a, r, th, dr, dth, dph = 0.9, 3.0, 0.7, -0.02, 0.01, 0.03
    sigma = r * r + a * a * math.cos(th) ** 2
    delta = r * r - 2 * r + a * a
    big_a = (r * r + a * a) ** 2 - a * a * delta * math.sin(th) ** 2
    want = math.sqrt(sigma / delta * dr * dr + sigma * dth * dth + big_a * math.sin(th) ** 2 / sigma * dph * dph)
    got = vo.proper_length(a, np.array([r]), np.array([th]), np.array([dr]), np.array([dth]), np.array([dph]))[0]
    assert abs(got / want - 1) < 1e-14 and vo.proper_length(-a, np.array([r]), np.array([th]), np.array([dr]), np.array([dth]), np.array([dph]))[0] == got


def _radial_ray(r_from, r_to, steps, th=1.2):
    r = np.linspace(r_from, r_to, steps + 1)
    return [(float(i), float(ri), th, 0.0) for i, ri in enumerate(r[1:], 1)], (r_from, th, 0.0)


def test_optically_thin_uniform_emissivity_is_the_line_integral():
    """total = j sum(l E^3), per ray; and the spectrum holds all of it when the bins cover E"""
    m = _grid(nr=4, r_min=2.0, dr=10.0)
    ray, start = _radial_ray(30.0, 5.0, 50)
    jj, z = 0.25, np.linspace(0.8, 1.6, 50)
    got = _measure(m, 0.0, [ray], [start], np.full(4, jj), z=z)
    r = np.array([row[1] for row in ray])
    length = (25.0 / 50) / np.sqrt(1 - 2 / r)
    want = jj * np.sum(length / z ** 3)
    assert abs(got["image"][0] / want - 1) < 1e-13 and got["contributions"] == 50 and (got["tau"] == 0).all()
    b = api.observe_bins_struct(0.5, 1.5, 10)
    out = vo.bin_rows(b, got)
    assert abs(out["spectrum"].sum() / want - 1) < 1e-13 and out["hits"].sum() == 50 and out["response"].shape == (10, 0)
    assert np.array_equal(out["hits"], np.bincount(((1 / z - 0.5) / 0.1).astype(int), minlength=10))


def test_uniform_absorption_tends_to_the_transfer_solution():
    """uniform j and kappa along a finely stepped ray, E = 1: total -> (j / kappa)(1 - exp(-kappa L)), L the proper length of the path; the sum is a
    left Riemann sum of j exp(-kappa s), so it lies above the integral by less than j dl_max"""
    m = _grid(nr=1, r_min=2.0, dr=100.0)
    steps = 20000
    ray, start = _radial_ray(60.0, 10.0, steps)
    jj, kk = 0.7, 0.08
    got = _measure(m, 0.0, [ray], [start], np.full(1, jj), kappa=np.full(1, kk))
    L = got["len"].sum()
    # the closed form of L: the integral of dr / sqrt(1 - 2 / r)
    F = lambda r: math.sqrt(r * (r - 2)) + 2 * math.log(math.sqrt(r) + math.sqrt(r - 2))      # noqa: E731
    assert abs(L / (F(60.0) - F(10.0)) - 1) < 1e-4
    want = jj / kk * (1 - math.exp(-kk * L))
    assert 0 <= got["image"][0] - want < jj * got["len"].max() and abs(got["image"][0] / want - 1) < 1e-3
    assert abs(got["tau"][-1] - kk * (L - got["len"][-1])) < 1e-9
    thin = _measure(m, 0.0, [ray], [start], np.full(1, jj))
    assert got["image"][0] < thin["image"][0] and abs(thin["image"][0] / (jj * L) - 1) < 1e-12


def test_polar_reflection_row_is_degenerate():
    """|dphi| >= pi / 2: the row counts as degenerate, adds nothing and does not absorb"""
    m = _grid()
    th = 0.01
    ray = [(1.0, 9.5, th, 0.0), (2.0, 9.4, th, np.pi), (3.0, 9.3, th + 0.01, np.pi + 0.001)]
    got = _measure(m, 0.0, [ray], [(9.6, th, 0.0)], np.ones(4), kappa=np.full(4, 0.5))
    assert (got["rows"], got["in_grid"], got["lit"], got["contributions"], got["degenerate"]) == (3, 3, 3, 2, 1)
    assert got["tau"][0] == 0 and got["tau"][1] == got["len"][0] * 0.5          # (the dropped row left tau alone)
    edge = _measure(m, 0.0, [[(1.0, 9.5, th, np.pi / 2)]], [(9.6, th, 0.0)], np.ones(4))
    assert edge["degenerate"] == 1 and edge["contributions"] == 0 and edge["image"][0] == 0
    # a row that did not move at all has l = 0: degenerate as well
    still = _measure(m, 0.0, [[(1.0, 9.5, th, 0.0)]], [(9.5, th, 0.0)], np.ones(4))
    assert still["degenerate"] == 1 and still["lit"] == 1


def test_absorption_without_emission():
    """tau grows in a cell with j = 0, kappa > 0; a cell with neither is not lit"""
    m = _grid(nr=3, r_min=2.0, dr=10.0)          # cells [2, 12), [12, 22), [22, 32)
    ray, start = _radial_ray(31.0, 3.0, 28)      # r = 30, 29, ..., 3
    emis, kappa = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.2, 0.0])
    got = _measure(m, 0.0, [ray], [start], emis, kappa=kappa)
    r = np.array([row[1] for row in ray])
    assert (got["rows"], got["in_grid"], got["lit"], got["contributions"]) == (28, 28, int(((r >= 12) & (r < 22)).sum() + (r < 12).sum()), int((r < 12).sum()))
    absorbed = np.sum(1.0 / np.sqrt(1 - 2 / r[(r >= 12) & (r < 22)])) * 0.2
    assert np.allclose(got["tau"], absorbed, rtol=1e-13) and absorbed > 1
    thin = _measure(m, 0.0, [ray], [start], emis)
    assert np.allclose(got["image"][0], thin["image"][0] * math.exp(-absorbed), rtol=1e-13) and thin["lit"] == int((r < 12).sum())


def test_bad_energy_shift_emits_nothing_and_still_absorbs():
    m = _grid(nr=1, r_min=2.0, dr=100.0)
    ray, start = _radial_ray(20.0, 16.0, 4)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        got = _measure(m, 0.0, [ray], [start], np.ones(1), kappa=np.full(1, 0.3), z=[1.0, bad, 1.0, 1.0])
        assert (got["contributions"], got["bad_g"], got["lit"], got["degenerate"]) == (3, 1, 4, 0)
        lens = 1.0 / np.sqrt(1 - 2 / np.array([19.0, 18.0, 17.0, 16.0]))
        assert np.allclose(got["tau"], [0.0, 0.3 * (lens[0] + lens[1]), 0.3 * lens[:3].sum()], rtol=1e-14)      # (the bad row's own l kappa is in)
        assert np.allclose(got["image"][0], np.sum(lens[[0, 2, 3]] * np.exp(-got["tau"])), rtol=1e-14)


def test_tau_and_the_total_are_per_ray():
    m = _grid(nr=1, r_min=2.0, dr=100.0)
    ray, start = _radial_ray(20.0, 16.0, 4)
    got = _measure(m, 0.0, [ray, [], ray], [start, start, start], np.ones(1), kappa=np.full(1, 0.3))
    assert got["image"][0] == got["image"][2] > 0 and got["image"][1] == 0 and np.array_equal(got["tau"][:4], got["tau"][4:]) and got["tau"][4] == 0


def test_bins_edges_delay_and_ranges():
    m = _grid(nr=2, r_min=2.0, dr=10.0)
    ray, start = _radial_ray(20.0, 4.0, 4)          # r = 16, 12 (cell 1), 8, 4 (cell 0); t = 1, 2, 3, 4
    z = [1.0, 0.5, 0.25, 2.0]                       # E = 1, 2, 4, 0.5: exact
    got = _measure(m, 0.0, [ray], [start], np.ones(2), delay=np.array([10.0, 100.0]), z=z)
    assert np.array_equal(got["T"], [101.0, 102.0, 13.0, 14.0]) and np.array_equal(got["E"], [1.0, 2.0, 4.0, 0.5])
    b = api.observe_bins_struct(1.0, 4.0, 3, t0=0.0, tmax=104.0, nt=2)          # E edges 1, 2, 3, 4;  t edges 0, 52, 104
    out = vo.bin_rows(b, got)
    # E = 1 sits on the first edge (q = 0: inside), 2 on an inner one (bin 1), 4 on the last (q = nen: outside), 0.5 below
    assert out["hits"].tolist() == [1, 1, 0] and out["contributions"] == 4
    assert out["response"][0].tolist() == [0, got["w"][0]] and out["response"][1].tolist() == [0, got["w"][1]] and out["spectrum"][1] == got["w"][1]
    assert out["response"].sum() == got["w"][0] + got["w"][1]
    assert vo.near_edge_e(got, bins=b) == 3 and vo.near_edge_e(np.array([0.5, 1.0 + 1e-12, np.nan, 2.3])) == 1
    log = api.observe_bins_struct(0.5, 4.0, 3, logbin_en=True)                   # edges 0.5, 1, 2, 4
    assert abs(log.den - 2.0) < 1e-15
    E = {"E": np.array([0.75, 1.5, 3.0, 0.4, 5.0]), "T": np.zeros(5), "w": np.ones(5), "image": np.zeros(1), **{k: 0 for k in vo.TALLIES}}
    assert vo.bin_rows(log, E)["hits"].tolist() == [1, 1, 1]


def test_volume_emissivity_is_the_mappers_expression():
    m = api.volume_map_struct(3.0, 30.0, 4, 3, 2, False)
    shape = (4, 3, 2)
    count = np.zeros(shape)
    count[1, 1, 0], count[2, 2, 1], count[0, 0, 0] = 4.0, 2.0, 5.0          # (the last one lies on the axis: no volume)
    vmap = {"count": count, "time": count * 7.0, "redshift": count * 0.5, "num_rays": 1000}
    emis, delay = api.volume_emissivity(vmap, m, 0.5, gamma=2.0)
    vol = api.cell_volume(m, 0.5)
    assert emis.shape == shape and abs(emis[1, 1, 0] / (4.0 / (1000 * vol[1, 1, 0]) * 0.5 ** -2) - 1) < 1e-15
    assert emis[0, 0, 0] == 0 and vol[0, 0, 0] == 0 and delay[0, 0, 0] == 7.0
    assert (emis[count == 0] == 0).all() and (delay[count == 0] == 0).all() and delay[2, 2, 1] == 7.0
    assert abs(api.volume_emissivity(vmap, m, 0.5, gamma=3.0)[0][2, 2, 1] / (2.0 / (1000 * vol[2, 2, 1]) * 0.5 ** -3) - 1) < 1e-15
