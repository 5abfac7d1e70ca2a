"""GPU: observing a volume map (kr_trace_observe_*) against the numpy rule of tests/volume_observe_rules.py applied to the path recorder's
write_step = 1 rows -- the recorder is pinned to the reference's own trajectory files and to the strict trace by tests/test_gpu_paths.py, the cells come
from tests/volume_map_rules.py, the energy shift from the CPU oracle.  hits and the six tallies are EQUAL; spectrum, response and the per-ray image are
sums in another order (and one exp of another library), within parity.BIN_RTOL.

Inputs: synthetic fields from the cell index (emis = 1 / (1 + cell % 7), zero in every fifth cell; kappa = 0.05 (cell % 3); delay = 0.1 cell) on the
grids of test_gpu_volume_map.py; 32 linear energy bins across the 1st to 99th percentile of the E the rule finds, widened by a quarter of a bin at
either end (so that no edge is an E of the data; the rest of the rows fall outside and exercise the range test), 20 time bins across the t of the
in-grid rows.  Every case asserts its precondition, near_edge_e == 0: no contributing row has a q_e within 1e-9 of a bin edge, where the last bit of
the energy shift would decide the bin."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import golden_cases as gc
import parity
import volume_observe_rules as vo
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

R0, RMAX = 1.2, 40.0
GRIDS = {"24x16x1": (24, 16, 1), "12x8x12": (12, 8, 12)}


def grid(nr, ntheta, nphi, reverse=1, logbin=False, **kw):
    """nr cells over r in [1.2, 40), Mapper's widths in theta and phi; V = -1, projradius = 1: the mapper's own orbital velocity"""
    m = api.volume_map_struct(R0, RMAX, nr, ntheta, nphi, logbin, V=-1.0, mode=0, reverse=reverse, projradius=1, motion=0)
    m.dr = float(np.exp(np.log(RMAX / R0) / nr)) if logbin else (RMAX - R0) / nr
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def fields(m, absorbing=True, delayed=True):
    cell = np.arange(m.nr * m.ntheta * m.nphi)
    emis = 1.0 / (1 + cell % 7)
    emis[::5] = 0.0
    return emis, (0.05 * (cell % 3) if absorbing else None), (0.1 * cell if delayed else None)


@functools.lru_cache(maxsize=None)
def recording(case, run, mark=17):
    """(params, init, offsets, rows, the strict trace's records) of a golden init with every 17th ray unused and one at the step limit; computed once,
    read-only"""
    p = capi.copy_params(gc.cases()[case]["runs"][run], flags=0)
    init = np.load(gc.golden_path(case))["init"].copy()
    init["steps"][::mark] = -1
    init["steps"][5] = capi.STEPLIM + 1
    offsets, rows, traced, out, _ = api.trace_paths(p, init, write_step=1)
    want, _ = api.trace(p, init)
    assert parity.same_records(out, want)
    assert (init["emit"][traced.astype(bool)] != 0).all()          # (redshift_start has been applied to the golden init)
    for a in (init, offsets, rows, want):
        a.setflags(write=False)
    return p, init, offsets, rows, want


@functools.lru_cache(maxsize=None)
def measured(case, run, shape, absorbing, delayed, reverse=1, motion=0, V=-1.0):
    """the rule's per-row quantities for a recording on a grid with the synthetic fields; computed once per combination"""
    p, init, offsets, rows, _ = recording(case, run)
    m = grid(*GRIDS[shape], reverse=reverse, motion=motion, V=V)
    emis, kappa, delay = fields(m, absorbing, delayed)
    return vo.measure_recording(m, p.spin, init, offsets, rows, emis, kappa, delay)


def bins_for(meas, response, logbin_en=False):
    E = meas["E"]
    lo, hi = np.percentile(E, [1, 99])
    w = (hi - lo) / 32
    if logbin_en:
        return api.observe_bins_struct(lo * 0.99, hi * 1.01, 32, logbin_en=True)
    t = meas["t_in_grid"]
    return api.observe_bins_struct(lo - 0.25 * w, hi + 0.25 * w, 32, t0=float(t.min()), tmax=float(t.max()), nt=20 if response else 0)


def check(label, got, want, b, meas, offsets, want_records, n_rays):
    problems = vo.compare(got, want, parity.BIN_RTOL)
    print(f"observe {label}: rows {got['rows']}, in grid {got['in_grid']}, lit {got['lit']}, contributions {got['contributions']}, bad g {got['bad_g']}, degenerate "
          f"{got['degenerate']}, hits {int(got['hits'].sum())} in {int((got['hits'] > 0).sum())} / {b.nen} bins, response cells {int((got['response'] > 0).sum())}, "
          f"worst relative difference spectrum {vo.worst_rel(got['spectrum'], want['spectrum']):.2e} response {vo.worst_rel(got['response'], want['response']):.2e} "
          f"image {vo.worst_rel(got['image'], want['image']) if got['image'] is not None else -1:.2e}, kernel {got['stats']['kernel_ms']:.2f} ms; problems {problems}")
    assert vo.near_edge_e(meas, bins=b) == 0          # the precondition on the inputs
    assert not problems, problems
    assert got["rows"] == int(offsets[-1])
    assert got["contributions"] >= got["hits"].sum()
    assert parity.same_records(got["rays"], want_records)
    if n_rays >= 256:          # not vacuous
        assert got["contributions"] > 1000 and (got["hits"] > 0).sum() > b.nen // 4
        if b.nt > 0:
            assert (got["response"] > 0).sum() > b.nt // 4 and got["response"].sum() <= got["spectrum"].sum()


CAMERA_RUNS = [("ip15", "euler"), ("ip15", "rk4"), ("ip15", "rk4_isco")]


@pytest.mark.parametrize("response", [False, True], ids=["no_response", "response_with_delay"])
@pytest.mark.parametrize("absorbing", [False, True], ids=["thin", "absorbing"])
@pytest.mark.parametrize("shape", list(GRIDS))
@pytest.mark.parametrize("case,run", CAMERA_RUNS, ids=[f"{c}-{r}" for c, r in CAMERA_RUNS])
def test_observation_is_the_rule_applied_to_the_recorded_rows(case, run, shape, absorbing, response):
    p, init, offsets, rows, want_records = recording(case, run)
    m = grid(*GRIDS[shape])
    emis, kappa, delay = fields(m, absorbing, response)
    meas = measured(case, run, shape, absorbing, response)
    b = bins_for(meas, response)
    got = api.trace_observe(p, init, m, b, emis, kappa, delay)
    want = vo.bin_rows(b, meas)
    check(f"{case}/{run} {shape} {'absorbing' if absorbing else 'thin'} nt {b.nt}", got, want, b, meas, offsets, want_records, len(init))
    skipped = (init["steps"] < 0) | (init["steps"] >= capi.STEPLIM)
    assert (got["image"][skipped] == 0).all() and skipped.sum() > 10
    if absorbing:
        thin = measured(case, run, shape, False, response)
        assert got["image"].sum() < thin["image"].sum() and got["spectrum"].sum() < vo.bin_rows(b, thin)["spectrum"].sum()


def test_logarithmic_energy_grid():
    """The device's log may differ from numpy's in the last bit, so a row within rounding of an edge may land next door: parity.compare_bins with its
    stock count slack, at most 2 bins left out of the sum check."""
    p, init, offsets, rows, want_records = recording("ip15", "rk4")
    m = grid(*GRIDS["24x16x1"])
    emis, kappa, delay = fields(m, True, False)
    meas = measured("ip15", "rk4", "24x16x1", True, False)
    b = bins_for(meas, False, logbin_en=True)
    got = api.trace_observe(p, init, m, b, emis, kappa, delay)
    want = vo.bin_rows(b, meas)
    as_bins = lambda v: {"count": v["hits"], "flux": v["spectrum"], "emis": v["spectrum"], "sum_redshift": v["spectrum"], "sum_time": v["spectrum"]}      # noqa: E731
    problems = parity.compare_bins(as_bins(got), as_bins(want), max_excluded=2, label="volume observe, logarithmic energy grid")
    print(f"observe log energy grid: rows within 1e-9 of an edge {vo.near_edge_e(meas, bins=b)}, bins that differ in hits {int((got['hits'] != want['hits']).sum())}; "
          f"problems {problems}")
    assert not problems, problems
    for k in vo.TALLIES:
        assert got[k] == want[k], k
    assert vo.worst_rel(got["image"], want["image"]) <= parity.BIN_RTOL and parity.same_records(got["rays"], want_records)
    assert got["contributions"] > 1000 and (got["hits"] > 0).sum() > 8


@pytest.mark.parametrize("absorbing", [False, True], ids=["thin", "absorbing"])
def test_radial_emitters_on_euler(absorbing):
    """motion = 1: the emitter moves radially, so z depends on rdot_sign at the row -- the sign the Euler update moved r with, which the rule reads off
    the rows themselves (volume_map_rules.signs_for refuses a ray that stood still in r: ps_h10 must have none).  Source rays: reverse = 0."""
    p, init, offsets, rows, want_records = recording("ps_h10", "euler")
    m = grid(*GRIDS["24x16x1"], reverse=0, motion=1, V=0.3)
    emis, kappa, delay = fields(m, absorbing, True)
    meas = measured("ps_h10", "euler", "24x16x1", absorbing, True, reverse=0, motion=1, V=0.3)
    b = bins_for(meas, True)
    got = api.trace_observe(p, init, m, b, emis, kappa, delay)
    check(f"motion = 1 {'absorbing' if absorbing else 'thin'}", got, vo.bin_rows(b, meas), b, meas, offsets, want_records, len(init))
    if absorbing:
        assert got["image"].sum() < measured("ps_h10", "euler", "24x16x1", False, True, reverse=0, motion=1, V=0.3)["image"].sum()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("run", ["euler", "rk4"])
def test_wave_boundaries_with_skipped_slots(run, n):
    """One wave exactly full, one slot short, one over, three waves; every third slot unused, one at the step limit: the observation is the rule's, the
    skipped records keep their bytes and their image is 0."""
    p = capi.copy_params(gc.cases()["ip16"]["runs"][run], flags=0)
    steplim = p.steplim if p.steplim > 0 else capi.STEPLIM
    init = np.load(gc.golden_path("ip16"))["init"][:n].copy()
    init["steps"][1::3] = -1
    if n > 3:
        init["steps"][3] = steplim
    skipped = (init["steps"] < 0) | (init["steps"] >= steplim)
    offsets, rows, traced, out, _ = api.trace_paths(p, init, write_step=1)
    m = grid(*GRIDS["12x8x12"])
    emis, kappa, delay = fields(m)
    meas = vo.measure_recording(m, p.spin, init, offsets, rows, emis, kappa, delay)
    b = bins_for(meas, True) if len(meas["E"]) > 50 else api.observe_bins_struct(0.0413, 1.6413, 32, t0=9900.0, tmax=10150.0, nt=20)
    got = api.trace_observe(p, init, m, b, emis, kappa, delay)
    check(f"wave boundary {run} n {n}", got, vo.bin_rows(b, meas), b, meas, offsets, out, n)
    assert got["stats"]["rays_traced"] == int((~skipped).sum())
    assert got["rays"][skipped].tobytes() == init[skipped].tobytes() and (got["image"][skipped] == 0).all()
    if n >= 63:
        assert got["contributions"] > 100 and got["hits"].sum() > 50


def test_lanes_are_reused():
    """More rays than the launch has lanes, so every lane takes several rays in turn: hits and the tallies are exactly tiles x the single run's, and
    every copy of a ray has the same image to the bit (a ray's total is summed in its lane, in step order) -- which a tau, an image_ray or an emit that
    leaked from a lane's previous ray would break."""
    p, init, offsets, rows, want_records = recording("ps_h10", "rk4")
    tiles = 400
    info = api.device_info()
    assert tiles * len(init) > 2 * 64 * 16 * info["cu_count"], "the tiled input no longer exceeds the resident lanes of this device"
    m = grid(*GRIDS["12x8x12"], reverse=0)
    emis, kappa, delay = fields(m)
    b = bins_for(measured("ps_h10", "rk4", "12x8x12", True, True, reverse=0), True)
    one = api.trace_observe(p, init, m, b, emis, kappa, delay)
    many = api.trace_observe(p, np.tile(init, tiles), m, b, emis, kappa, delay)
    assert one["contributions"] > 1000 and (one["hits"] > 0).sum() > 8 and (one["response"] > 0).sum() > 8
    assert np.array_equal(many["hits"], tiles * one["hits"])
    for k in vo.TALLIES:
        assert many[k] == tiles * one[k], k
    assert vo.worst_rel(many["spectrum"], tiles * one["spectrum"]) <= parity.BIN_RTOL and vo.worst_rel(many["response"], tiles * one["response"]) <= parity.BIN_RTOL
    assert np.array_equal(many["image"], np.tile(one["image"], tiles))
    assert parity.same_records(many["rays"], np.tile(want_records, tiles))
    print(f"observe refill: rays {tiles * len(init)} on {info['cu_count']} CUs, contributions {many['contributions']}, launch {many['stats']['kernel_ms']:.2f} ms")


def test_adds_and_does_not_overwrite_and_image_is_optional():
    L = api.lib()
    p, init, offsets, rows, _ = recording("ip15", "rk4")
    init = init.copy()
    m = grid(*GRIDS["12x8x12"])
    emis, kappa, delay = fields(m)
    meas = measured("ip15", "rk4", "12x8x12", True, True)
    b = bins_for(meas, True)
    nw = api.observe_words(b)
    single = api.trace_observe(p, init, m, b, emis, kappa, delay)
    no_image = api.trace_observe(p, init, m, b, emis, kappa, delay, want_image=False)
    assert no_image["image"] is None and np.array_equal(no_image["hits"], single["hits"]) and not vo.compare(no_image, single, parity.BIN_RTOL)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    with DeviceScope(L) as dev:
        bufs = {"rays": dev.alloc(init.nbytes), "out": dev.zeros(nw * 8), "emis": dev.upload(emis), "kappa": dev.upload(kappa), "delay": dev.upload(delay)}
        st = capi.Stats()
        for _ in range(2):          # d_image = NULL
            capi.check(L, L.kr_memcpy_h2d(bufs["rays"], ptr(init), init.nbytes), "h2d")
            capi.check(L, L.kr_trace_observe_dev_f64(C.byref(p), C.byref(m), C.byref(b), bufs["emis"], bufs["kappa"], bufs["delay"], bufs["rays"], len(init), bufs["out"],
                                                     None, None, C.byref(st)), "kr_trace_observe_dev")
        words = dev.fetch(bufs["out"], nw)
        twice = api.observe_from_words(b, words)
        twice["image"] = None
        doubled = {k: 2 * single[k] for k in vo.TALLIES + ("hits", "spectrum", "response")}
        assert not vo.compare(twice, doubled, parity.BIN_RTOL) and twice["contributions"] > 2000
        assert st.rays_traced == single["stats"]["rays_traced"] and st.steps_total == single["stats"]["steps_total"] and st.kernel_ms > 0
        # n = 0: the output is left untouched, whatever it holds
        capi.check(L, L.kr_trace_observe_dev_f64(C.byref(p), C.byref(m), C.byref(b), bufs["emis"], None, None, None, 0, bufs["out"], None, None, C.byref(st)), "n = 0")
        assert dev.fetch(bufs["out"], nw).tobytes() == words.tobytes() and st.rays_total == 0 and st.rays_traced == 0
    empty = api.trace_observe(p, np.zeros(0, dtype=capi.RAY_F64), m, b, emis)
    assert empty["spectrum"].sum() == 0 and empty["rows"] == 0 and len(empty["image"]) == 0


# ---- the pipeline and the program --------------------------------------------------------------------------------------------------------------
SPIN = 0.998


def two_sources():
    specs = []
    for h in (5.0, 8.0):
        s = capi.PointSourceSpec()
        for i, v in enumerate((0.0, h, 1e-3, 0.0)):
            s.pos[i] = v
        s.V, s.spin, s.tol, s.E = 0.0, SPIN, 100.0, 1.0
        s.cosalpha0, s.cosalphamax, s.dcosalpha = -0.995, 0.995, 0.05
        s.beta0, s.betamax, s.dbeta = -np.pi, np.pi, 0.2
        specs.append(s)
    return specs


def small_plane(nx=21):
    s = capi.ImagePlaneSpec()
    s.dist, s.inc_deg, s.x0, s.xmax, s.y0, s.ymax, s.spin, s.phi0, s.precision = 10000.0, 60.0, -20.0, 20.0, -20.0, 20.0, SPIN, 0.0, 100.0
    s.dx = s.dy = 40.0 / (nx - 1)
    return s


def pipeline_params():
    p_source = capi.copy_params(capi.default_params(SPIN), integrator=capi.RK4, r_max=100.0)
    p_plane = capi.copy_params(capi.default_params(-SPIN), integrator=capi.RK4, r_max=15000.0)
    return p_source, p_plane


def test_volume_spectrum_of_two_sources_is_the_observation_of_the_summed_map():
    p_source, p_plane = pipeline_params()
    m = api.volume_map_struct(1.2, 30.0, 10, 6, 5, False)
    s1, s2 = two_sources()
    plane = small_plane()
    b = api.observe_bins_struct(0.0513, 1.6513, 32, t0=9950.0, tmax=10250.0, nt=20)
    res = api.volume_spectrum([s1, s2], plane, p_source, p_plane, m, b)
    a, c = api.volume_map([s1], p_source, m), api.volume_map([s2], p_source, m)
    summed = {k: a[k] + c[k] for k in ("count", "time", "redshift", "num_rays")}
    emis, delay = api.volume_emissivity(summed, m, SPIN)
    assert np.array_equal(res["map"]["count"], summed["count"]) and np.allclose(res["emis"], emis, rtol=1e-12, atol=0) and (emis > 0).sum() > 50
    rays = api.imageplane_init(plane)
    api.redshift_start(-SPIN, 0.0, 1, 0, rays)
    mo = capi.VolumeMap.from_buffer_copy(m)
    mo.reverse = 1
    want = api.trace_observe(p_plane, rays, mo, b, emis, None, delay)
    got = dict(res, image=res["image"].ravel())
    problems = vo.compare(got, want, parity.BIN_RTOL)
    print(f"volume_spectrum: contributions {res['contributions']}, hits {int(res['hits'].sum())} in {int((res['hits'] > 0).sum())} bins, response cells "
          f"{int((res['response'] > 0).sum())}; problems {problems}")
    assert not problems, problems
    assert res["contributions"] > 1000 and (res["hits"] > 0).sum() > 8 and (res["response"] > 0).sum() > 5 and res["image"].shape == (21, 21)
    # and with absorption the total drops
    kappa = np.full(m.nr * m.ntheta * m.nphi, 0.05)
    absorbed = api.volume_spectrum([s1, s2], plane, p_source, p_plane, m, b, kappa=kappa)
    assert absorbed["image"].sum() < res["image"].sum() and np.array_equal(absorbed["hits"], res["hits"])


APPS = os.path.join(gc.ROOT, "tests", "golden", "apps")
EXE = os.path.join(gc.ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_volume_spectrum")


def test_program_writes_what_volume_spectrum_computes():
    """kr_volume_spectrum on a small par file: SPECTRUM / RESPONSE / IMAGE are api.volume_spectrum of the same inputs within parity.BIN_RTOL, HITS and
    the tallies in the header are equal."""
    import tempfile

    import fits_lite
    assert os.path.exists(EXE), f"{EXE} not built (make -C raytrace_cpu_amd/apps)"
    with tempfile.TemporaryDirectory() as w:
        out = os.path.join(w, "spectrum.fits")
        r = subprocess.run([EXE, f"--parfile={os.path.join(APPS, 'volume_spectrum.par')}", f"--outfile={out}", "--timing"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "timing: source rays" in r.stdout
        hdus = fits_lite.read(out)
    assert [h["name"] for h in hdus] == ["PRIMARY", "ENERGY", "SPECTRUM", "HITS", "RESPONSE", "IMAGE"]
    s = two_sources()[0]
    p_source, p_plane = pipeline_params()
    p_plane.r_max = 1.5 * 10000.0
    m = api.volume_map_struct(1.2, 30.0, 10, 6, 5, False)
    plane = small_plane(17)
    b = api.observe_bins_struct(0.05, 1.65, 32, t0=9950.0, tmax=10250.0, nt=20)
    want = api.volume_spectrum([s], plane, p_source, p_plane, m, b)
    head = hdus[0]["header"]
    num = {k: float(head[k]) for k in ("SPIN", "DIST", "INCL", "X0", "XMAX", "NX", "Y0", "YMAX", "NY", "EN0", "ENMAX", "NEN", "LOGBIN_E", "T0", "TMAX", "NT", "R0", "RMAX",
                                       "NR", "NTHETA", "NPHI", "GAMMA", "KAPPA", "NUM_RAYS", "ROWS", "IN_GRID", "LIT", "CONTRIB", "BAD_G", "DEGENER")}
    assert (num["SPIN"], num["DIST"], num["INCL"], num["NX"], num["NY"], num["NEN"], num["NT"], num["NR"], num["NTHETA"], num["NPHI"], num["GAMMA"], num["KAPPA"]) == \
        (SPIN, 10000.0, 60.0, 17, 17, 32, 20, 10, 6, 5, 2.0, 0.0)
    assert (num["EN0"], num["ENMAX"], num["T0"], num["TMAX"], num["X0"], num["XMAX"], num["LOGBIN_E"]) == (0.05, 1.65, 9950.0, 10250.0, -20.0, 20.0, 0)
    assert num["NUM_RAYS"] == want["map"]["num_rays"] > 1000
    assert [num[k] for k in ("ROWS", "IN_GRID", "LIT", "CONTRIB", "BAD_G", "DEGENER")] == [want[k] for k in vo.TALLIES]
    data = {h["name"]: np.asarray(h["data"], dtype=np.float64) for h in hdus[1:]}
    assert np.allclose(data["ENERGY"].ravel(), 0.5 * (want["energy"][:-1] + want["energy"][1:]), rtol=1e-14, atol=0)
    assert np.array_equal(data["HITS"].ravel(), want["hits"]) and want["contributions"] > 1000 and (want["hits"] > 0).sum() > 8
    assert data["RESPONSE"].shape == (32, 20) and data["IMAGE"].shape == (17, 17)
    for name, key in (("SPECTRUM", "spectrum"), ("RESPONSE", "response"), ("IMAGE", "image")):
        assert vo.worst_rel(data[name].ravel(), want[key].ravel()) <= parity.BIN_RTOL, name
    assert (data["RESPONSE"] > 0).sum() > 5 and (data["IMAGE"] > 0).sum() > 20
