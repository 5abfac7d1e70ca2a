"""GPU: volume illumination maps (kr_trace_volume_*) against the numpy rule of tests/volume_map_rules.py applied to the path recorder's
write_step = 1 rows -- the recorder is pinned to the reference's own trajectory files and to the strict trace by tests/test_gpu_paths.py, the energy
shift comes from the CPU oracle.  Linear grids: every quotient is one IEEE operation on both sides, so count and the four tallies are EQUAL; time and
redshift are sums in another order, within parity.BIN_RTOL.

Measured on MI355X: every case below -- Euler, RK4, RK4 with a destination, both grids, both modes, motion = 1, the wave boundaries, 533 600 rays on
reused lanes -- equal in count and tallies, time / redshift within 3e-14 relative; the logarithmic grid: no cell differs (rows within 1e-9 of an
edge: 0)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import golden_cases as gc
import parity
import volume_map_rules as vr
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

R0, RMAX = 1.2, 40.0


def grid(nr, ntheta, nphi, mode, logbin=False, **kw):
    """nr cells over r in [1.2, 40), Mapper's widths in theta and phi; V = -1, projradius = 1: the mapper's own orbital velocity"""
    m = api.volume_map_struct(R0, RMAX, nr, ntheta, nphi, logbin, V=-1.0, mode=mode, projradius=1, motion=0)
    m.dr = float(np.exp(np.log(RMAX / R0) / nr)) if logbin else (RMAX - R0) / nr
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def marked_init(case, n=None):
    init = np.load(gc.golden_path(case))["init"].copy()
    if n is not None:
        init = init[:n].copy()
    return init


@functools.lru_cache(maxsize=None)
def recording(case, run):
    """(params, init, offsets, rows, the strict trace's records) of a golden init with every 17th ray unused and one at the step limit; computed once,
    read-only"""
    p = capi.copy_params(gc.cases()[case]["runs"][run], flags=0)
    init = marked_init(case)
    init["steps"][::17] = -1
    init["steps"][5] = capi.STEPLIM + 1
    offsets, rows, traced, out, _ = api.trace_paths(p, init, write_step=1)
    want, _ = api.trace(p, init)
    assert parity.same_records(out, want)
    assert (init["emit"][traced.astype(bool)] != 0).all()          # (redshift_start has been applied to the golden init)
    for a in (init, offsets, rows, want):
        a.setflags(write=False)
    return p, init, offsets, rows, want


def as_bins(v):
    return {"count": v["count"].ravel(), "flux": v["time"].ravel(), "emis": v["redshift"].ravel(), "sum_redshift": v["redshift"].ravel(), "sum_time": v["time"].ravel()}


def worst_rel(got, want):
    out = 0.0
    for k in ("time", "redshift"):
        g, w = got[k], want[k]
        rel = np.where(g == w, 0.0, np.abs(g - w) / np.maximum(np.abs(w), 1e-300))
        out = max(out, float(rel.max()))
    return out


RUNS = [("ps_h10", "euler"), ("ps_h10", "rk4"), ("ps_h5", "rk4_isco")]
GRIDS = {"24x16x1": (24, 16, 1), "12x8x12": (12, 8, 12)}


@pytest.mark.parametrize("mode", [0, 1], ids=["passage", "every_row"])
@pytest.mark.parametrize("shape", list(GRIDS))
@pytest.mark.parametrize("case,run", RUNS, ids=[f"{c}-{r}" for c, r in RUNS])
def test_map_is_the_rule_applied_to_the_recorded_rows(case, run, shape, mode):
    p, init, offsets, rows, want_records = recording(case, run)
    m = grid(*GRIDS[shape], mode)
    got = api.trace_volume(p, init, m)
    want = vr.rule(m, p.spin, init, offsets, rows)
    problems = vr.compare(got, want, parity.BIN_RTOL)
    print(f"volume map {case}/{run} {shape} mode {mode}: rows {got['rows']} (recorded {int(offsets[-1])}), in grid {got['in_grid']}, deposits {got['deposits']}, "
          f"bad g {got['bad_g']}, cells hit {int((got['count'] > 0).sum())} / {got['count'].size}, worst relative sum difference {worst_rel(got, want):.2e}, "
          f"kernel {got['stats']['kernel_ms']:.2f} ms; problems {problems}")
    assert got["rows"] == int(offsets[-1])
    assert got["deposits"] == int(got["count"].sum()) and got["deposits"] + got["bad_g"] <= got["in_grid"] <= got["rows"]
    assert not problems, problems
    assert parity.same_records(got["rays"], want_records)
    assert got["deposits"] > 1000 and (got["count"] > 0).sum() > got["count"].size // 8          # (not vacuous)
    if mode == 1:
        assert got["deposits"] + got["bad_g"] == got["in_grid"]


def test_logarithmic_grid():
    """The device's log may differ from numpy's in the last bit, so a row within rounding of an edge may land next door: parity.compare_bins with its
    stock count slack, at most 2 cells left out of the sum check."""
    p, init, offsets, rows, want_records = recording("ps_h10", "rk4")
    m = grid(24, 16, 1, 0, logbin=True)
    got = api.trace_volume(p, init, m)
    want = vr.rule(m, p.spin, init, offsets, rows)
    problems = parity.compare_bins(as_bins(got), as_bins(want), max_excluded=2, label="volume map, logarithmic grid")
    print(f"volume map log grid: rows within 1e-9 of a radial edge {vr.near_edge(m, rows)}, cells that differ in count {int((got['count'] != want['count']).sum())}, "
          f"in grid {got['in_grid']} vs {want['in_grid']}, deposits {got['deposits']} vs {want['deposits']}; problems {problems}")
    assert not problems, problems
    assert got["rows"] == want["rows"] == int(offsets[-1]) and abs(got["in_grid"] - want["in_grid"]) <= 2
    assert got["deposits"] == int(got["count"].sum()) and parity.same_records(got["rays"], want_records)


@pytest.mark.parametrize("mode", [0, 1], ids=["passage", "every_row"])
def test_radial_observers_on_euler(mode):
    """motion = 1: the observer moves radially, so g depends on rdot_sign at the row -- the sign the Euler update moved r with, which the rule reads off
    the rows themselves (volume_map_rules.signs_for refuses a ray that stood still in r: ps_h10 must have none)."""
    p, init, offsets, rows, _ = recording("ps_h10", "euler")
    m = grid(24, 16, 1, mode, motion=1, V=0.3)
    got = api.trace_volume(p, init, m)
    want = vr.rule(m, p.spin, init, offsets, rows)            # (raises on a zero radial difference)
    problems = vr.compare(got, want, parity.BIN_RTOL)
    print(f"volume map motion = 1 mode {mode}: deposits {got['deposits']}, bad g {got['bad_g']}, worst relative sum difference {worst_rel(got, want):.2e}; problems {problems}")
    assert not problems, problems
    assert got["deposits"] > 1000


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("run", ["euler", "rk4"])
def test_wave_boundaries_with_skipped_slots(run, n):
    """One wave exactly full, one slot short, one over, three waves; every third slot unused, one at the step limit: the map is the rule's and the
    skipped records keep their bytes."""
    p = capi.copy_params(gc.cases()["ps_h10"]["runs"][run], flags=0)
    steplim = p.steplim if p.steplim > 0 else capi.STEPLIM
    init = marked_init("ps_h10", n)
    init["steps"][1::3] = -1
    if n > 3:
        init["steps"][3] = steplim
    skipped = (init["steps"] < 0) | (init["steps"] >= steplim)
    offsets, rows, traced, out, _ = api.trace_paths(p, init, write_step=1)
    m = grid(12, 8, 12, 0)
    got = api.trace_volume(p, init, m)
    want = vr.rule(m, p.spin, init, offsets, rows)
    problems = vr.compare(got, want, parity.BIN_RTOL)
    assert not problems, problems
    assert got["rows"] == int(offsets[-1]) and got["stats"]["rays_traced"] == int((~skipped).sum())
    assert got["rays"][skipped].tobytes() == init[skipped].tobytes()
    assert parity.same_records(got["rays"], out)


def test_lanes_are_reused():
    """More rays than the launch has lanes, so every lane takes several rays in turn: the counts are exactly tiles x the single map's, which a
    last_cell or an emit that leaked from a lane's previous ray would break."""
    p, init, offsets, rows, want_records = recording("ps_h10", "rk4")
    tiles = 400
    info = api.device_info()
    assert tiles * len(init) > 2 * 64 * 16 * info["cu_count"], "the tiled input no longer exceeds the resident lanes of this device"
    m = grid(12, 8, 12, 0)
    one = api.trace_volume(p, init, m)
    many = api.trace_volume(p, np.tile(init, tiles), m)
    assert np.array_equal(many["count"], tiles * one["count"])
    for k in vr.TALLIES:
        assert many[k] == tiles * one[k], k
    scaled = {k: tiles * one[k] for k in vr.PLANES + vr.TALLIES}
    assert not vr.compare(many, scaled, parity.BIN_RTOL)
    assert parity.same_records(many["rays"], np.tile(want_records, tiles))
    print(f"volume map refill: rays {tiles * len(init)} on {info['cu_count']} CUs, deposits {many['deposits']}, map launch {many['stats']['kernel_ms']:.2f} ms")


def test_adds_and_does_not_overwrite():
    L = api.lib()
    p, init, offsets, rows, _ = recording("ps_h10", "rk4")
    init = init.copy()
    m = grid(12, 8, 12, 0)
    nw = api.volume_words(m)
    single = api.trace_volume(p, init, m)
    with DeviceScope(L) as dev:
        d_rays, d_map = dev.alloc(init.nbytes), dev.zeros(nw * 8)
        st = capi.Stats()
        for _ in range(2):
            capi.check(L, L.kr_memcpy_h2d(d_rays, init.ctypes.data_as(C.c_void_p), init.nbytes), "h2d")
            capi.check(L, L.kr_trace_volume_dev_f64(C.byref(p), C.byref(m), d_rays, len(init), d_map, None, C.byref(st)), "kr_trace_volume_dev")
        words = dev.fetch(d_map, nw)
        twice = api.volume_from_words(m, words)
        assert not vr.compare(twice, vr.add_maps(single, single), parity.BIN_RTOL)
        assert st.rays_traced == single["stats"]["rays_traced"] and st.steps_total == single["stats"]["steps_total"] and st.kernel_ms > 0
        # n = 0: the map is left untouched, whatever it holds
        capi.check(L, L.kr_trace_volume_dev_f64(C.byref(p), C.byref(m), None, 0, d_map, None, C.byref(st)), "kr_trace_volume_dev n = 0")
        assert dev.fetch(d_map, nw).tobytes() == words.tobytes() and st.rays_total == 0 and st.rays_traced == 0
    empty = api.trace_volume(p, np.zeros(0, dtype=capi.RAY_F64), m)
    assert empty["count"].sum() == 0 and empty["rows"] == 0


def two_sources():
    specs = []
    for h in (5.0, 8.0):
        s = capi.PointSourceSpec()
        for i, v in enumerate((0.0, h, 1e-3, 0.0)):
            s.pos[i] = v
        s.V, s.spin, s.tol, s.E = 0.0, 0.998, 100.0, 1.0
        s.cosalpha0, s.cosalphamax, s.dcosalpha = -0.995, 0.995, 0.05
        s.beta0, s.betamax, s.dbeta = -np.pi, np.pi, 0.2
        specs.append(s)
    return specs


def test_volume_map_sums_its_sources():
    p = capi.copy_params(capi.default_params(0.998), integrator=capi.RK4, r_max=100.0)
    m = grid(12, 8, 12, 0)
    s1, s2 = two_sources()
    a, b, both = api.volume_map([s1], p, m), api.volume_map([s2], p, m), api.volume_map([s1, s2], p, m)
    assert not vr.compare(both, vr.add_maps(a, b), parity.BIN_RTOL)
    assert both["num_rays"] == a["num_rays"] + b["num_rays"] > 1000 and a["deposits"] > 1000 and b["deposits"] > 1000
    hit = both["count"] > 0
    assert np.allclose(both["mean_time"][hit], both["time"][hit] / both["count"][hit], rtol=0, atol=0) and np.isnan(both["mean_time"][~hit]).all()
    assert np.array_equal(both["mean_redshift"][hit], both["redshift"][hit] / both["count"][hit])
    # and the host-pointer form on the same rays gives the same map
    rays = api.pointsource_init(s1)
    api.redshift_start(0.998, s1.V, 0, 0, rays)
    host = api.trace_volume(p, rays, m)
    assert not vr.compare(host, a, parity.BIN_RTOL)


# ---- the program -----------------------------------------------------------------------------------------------------------------------------
APPS = os.path.join(gc.ROOT, "tests", "golden", "apps")
EXE = os.path.join(gc.ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_volume_map")


def test_program_writes_the_map():
    """kr_volume_map on a small par file: NRAYS / TIME / REDSHIFT are api.volume_map of the same inputs (counts equal; the means, sums in another
    order divided by equal counts, within parity.BIN_RTOL), NaN where nothing crossed; VOLUME is api.cell_volume."""
    import tempfile

    import fits_lite
    assert os.path.exists(EXE), f"{EXE} not built (make -C raytrace_cpu_amd/apps)"
    with tempfile.TemporaryDirectory() as w:
        out = os.path.join(w, "map.fits")
        r = subprocess.run([EXE, f"--parfile={os.path.join(APPS, 'volume_map.par')}", f"--outfile={out}", "--timing"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "timing: rays" in r.stdout
        hdus = fits_lite.read(out)
    assert [h["name"] for h in hdus] == ["PRIMARY", "NRAYS", "TIME", "REDSHIFT", "VOLUME"]
    s = capi.PointSourceSpec()
    for i, v in enumerate((0.0, 5.0, 1e-3, 0.0)):
        s.pos[i] = v
    s.V, s.spin, s.tol, s.E = 0.0, 0.998, 100.0, 1.0
    s.cosalpha0, s.cosalphamax, s.dcosalpha = -0.995, 0.995, 0.05
    s.beta0, s.betamax, s.dbeta = -np.pi, np.pi, 0.2
    p = capi.copy_params(capi.default_params(0.998), integrator=capi.RK4, r_max=100.0)
    m = api.volume_map_struct(1.2, 30.0, 10, 6, 5, False)
    want = api.volume_map([s], p, m)
    head = hdus[0]["header"]
    num = {k: float(head[k]) for k in ("SPIN", "R0", "RMAX", "NR", "DR", "LOGBIN_R", "THETAMAX", "NTHETA", "DTHETA", "NPHI", "DPHI", "MODE", "NUM_RAYS", "ROWS",
                                       "IN_GRID", "DEPOSITS", "BAD_G")}
    assert (num["SPIN"], num["R0"], num["RMAX"], num["NR"], num["NTHETA"], num["NPHI"], num["LOGBIN_R"], num["MODE"]) == (0.998, 1.2, 30.0, 10, 6, 5, 0, 0)
    assert abs(num["DR"] - m.dr) <= 1e-14 * m.dr and abs(num["DTHETA"] - m.dtheta) <= 1e-14 and abs(num["DPHI"] - m.dphi) <= 1e-14 and abs(num["THETAMAX"] - np.pi / 2) <= 1e-14
    assert num["NUM_RAYS"] == want["num_rays"] > 1000
    assert [num[k] for k in ("ROWS", "IN_GRID", "DEPOSITS", "BAD_G")] == [want[k] for k in vr.TALLIES]
    planes = {h["name"]: np.asarray(h["data"], dtype=np.float64) for h in hdus[1:]}
    for name, plane in planes.items():
        assert plane.shape == (10, 6 * 5), name
        planes[name] = plane.reshape(10, 6, 5)
    hit = want["count"] > 0
    assert np.array_equal(planes["NRAYS"], want["count"]) and hit.sum() > 50 and not hit.all()
    for name, key in (("TIME", "mean_time"), ("REDSHIFT", "mean_redshift")):
        assert np.array_equal(np.isnan(planes[name]), ~hit), name
        np.testing.assert_allclose(planes[name][hit], want[key][hit], rtol=parity.BIN_RTOL, atol=0, err_msg=name)
    np.testing.assert_allclose(planes["VOLUME"], api.cell_volume(m, 0.998), rtol=1e-13, atol=0)
