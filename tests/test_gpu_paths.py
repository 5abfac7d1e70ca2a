"""GPU: per-step ray paths recorded on the device (kr_trace_paths_*), (a) against the trajectory files the reference's own code wrote
(tests/golden/paths/, block rule in tests/paths_rules.py) and (b) against the trace itself, at full precision.

Measured on MI355X (profiles/ray_paths.txt): all six fixture files reproduced byte for byte (every block identical, 0 bad rays)."""
import ctypes as C

import numpy as np
import pytest

import golden_cases as gc
import parity
import paths_rules as pr
import step_control_cases as sc
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", pr.CASES)
def test_paths_match_the_reference_file(name):
    params, rays, kw = pr.case_inputs(name)
    offsets, rows, traced, out, st = api.trace_paths(params, rays, **kw)
    assert offsets[0] == 0 and offsets[-1] == len(rows) and (np.diff(offsets) >= 0).all()
    text = api.paths_text(offsets, rows, traced)
    want = pr.reference_text(name)
    res = pr.compare_texts(text, want)                     # (asserts the two blank lines after every block of either file)
    allowed = parity.allowed_bad_frac_strict(params, res["n_traced"])
    print(f"paths {name}: blocks {res['n_blocks_got']} / {res['n_traced']}, rows {len(rows)}, byte-identical blocks {res['frac_blocks_identical']:.4f}, "
          f"bad rays {res['n_bad']} {res['bad_index'][:16]} (allowed share {allowed:.4f}), whole file identical: {text == want}")
    parity.record_margin("test_paths_match_the_reference_file", name, res, allowed=allowed, frac_blocks_identical=res["frac_blocks_identical"],
                         rows=int(len(rows)), file_identical=bool(text == want))
    assert res["n_blocks_got"] == res["n_traced"] == int(traced.sum())
    assert res["frac_bad"] <= allowed, res


def test_windowed_ray_ends_with_the_reference_record():
    """A ray that leaves the radial window after it has written a row stops there (raytracer.cpp:938-941), and its final record is what the
    reference's epilogue makes of that state: compared with the records the reference itself left (tests/golden/paths/rk4_window.records.txt.gz) under
    the bar of the strict RK4 trace (parity.compare_rays at RAY_RTOL, step counts equal, parity.allowed_bad_frac_strict)."""
    params, rays, kw = pr.case_inputs("rk4_window")
    offsets, rows, traced, out, st = api.trace_paths(params, rays, **kw)
    want = pr.reference_records("rk4_window")
    assert len(want) == len(out)
    res = parity.compare_rays(out, want, rtol=parity.RAY_RTOL, steps_slack=parity.steps_slack_for(params))
    allowed = parity.allowed_bad_frac_strict(params, res["n_traced"])
    # the early stop is what the case is for: rays that ended inside r_max, above the disc, off the horizon and below the step limit
    stopped = (want["steps"] > 0) & ((want["status"] & (capi.STATUS_DEST | capi.STATUS_HORIZON | capi.STATUS_RLIM | capi.STATUS_STEPLIM)) == 0)      # (steps = -1: the allocation's unused tail)
    print(f"paths rk4_window records: traced {res['n_traced']}, stopped by the window {int(stopped.sum())}, bad {res['n_bad']}, bit-identical share {res['frac_bit_identical']:.4f}, "
          f"worst accepted {res['worst_ok']:.3e}")
    parity.record_margin("test_windowed_ray_ends_with_the_reference_record", "rk4_window", res, allowed=allowed, stopped_by_window=int(stopped.sum()))
    assert stopped.sum() >= 10
    assert res["frac_bad"] <= allowed, res
    # and a trace without recording does NOT stop those rays: the window is what ended them
    plain, _ = api.trace(params, rays)
    assert (np.abs(plain["steps"][stopped]) > np.abs(out["steps"][stopped])).all()


def test_lanes_are_refilled_from_the_queue():
    """More rays than the launch has lanes (persistent waves: at most 16 per compute unit), so that every lane takes several rays in turn: the ps_h10
    init tiled 400 times (533 600 rays), recorded coarsely inside a window.  Every copy must get the row count, the rows and the final record of
    its original -- which a small launch, where no lane is ever reused, recorded -- and the records must be those of api.trace(flags = 0)."""
    L = api.lib()
    p = capi.copy_params(gc.cases()["ps_h10"]["runs"]["rk4"], flags=0)
    one = np.load(gc.golden_path("ps_h10"))["init"].copy()
    one["steps"][::17] = -1                     # skipped rays among them
    tiles = 400
    info = api.device_info()
    assert tiles * len(one) > 2 * 64 * 16 * info["cu_count"], "the tiled input no longer exceeds the resident lanes of this device"
    kw = dict(write_step=40, write_rmin=1.5, write_rmax=30.0)
    off1, rows1, traced1, out1, _ = api.trace_paths(p, one, **kw)
    many = np.tile(one, tiles)
    off, rows, traced, out, st = api.trace_paths(p, many, **kw)
    n1 = len(one)
    counts1 = np.diff(off1)
    assert (np.diff(off).reshape(tiles, n1) == counts1).all()
    assert (traced.reshape(tiles, n1) == traced1).all()
    assert counts1.sum() > 0 and off[-1] == tiles * off1[-1] == len(rows)
    assert (rows.view(np.uint64).reshape(tiles, -1) == rows1.view(np.uint64).reshape(1, -1)).all()
    assert parity.same_records(out, np.tile(out1, tiles))
    # (the window stops rays early, so the yardstick trace is compared on a recording without one)
    offw, rowsw, _, outw, stw = api.trace_paths(p, many, write_step=1000)
    want, st_trace = api.trace(capi.copy_params(p), many)
    assert parity.same_records(outw, want)
    assert stw["steps_total"] == st_trace["steps_total"] and stw["rays_traced"] == st_trace["rays_traced"] == tiles * int(traced1.sum())
    print(f"paths refill: rays {len(many)} on {info['cu_count']} CUs, rows {len(rows)}, record kernel {st['kernel_ms']:.2f} ms; no window: rows {len(rowsw)}, "
          f"record kernel {stw['kernel_ms']:.2f} ms, plain trace kernel {st_trace['kernel_ms']:.2f} ms")


CONSISTENCY = [("ps_h10", "euler"), ("ps_h10", "rk4"), ("ip15", "rk4"), ("ip15", "rk4_isco"), ("ip15", "rk4_plane"), ("ps_h5", "rk4_flatdisc"), ("ps_h5", "rk4_steplim300")]


# ... and off the default step-control parameters (the recorder reuses the strict step): kr_params overrides on top of a golden run
CONSISTENCY_OVERRIDES = {("ps_h10", "rk4", "tight_caps"): sc.REGIMES["tight_caps"], ("ps_h10", "rk4", "boundary"): sc.REGIMES["boundary"]}
CONSISTENCY_RUNS = [(c, r, None) for c, r in CONSISTENCY] + list(CONSISTENCY_OVERRIDES)


@pytest.mark.parametrize("case,run,regime", CONSISTENCY_RUNS, ids=[f"{c}-{r}" + (f"-{g}" if g else "") for c, r, g in CONSISTENCY_RUNS])
def test_recording_is_the_strict_trace_with_rows(case, run, regime):
    """No window, on an existing golden init: a recording ends with the records of api.trace(flags = 0), its write_step = 7 rows are every seventh
    write_step = 1 row, and a ray that ended by the loop condition has its final (t, r, theta, phi) as its last row -- all bit for bit."""
    p = capi.copy_params(gc.cases()[case]["runs"][run], flags=0, **(CONSISTENCY_OVERRIDES[case, run, regime] if regime else {}))
    init = np.load(gc.golden_path(case))["init"].copy()
    init["steps"][::17] = -1                       # rays the skip rule leaves out (raytracer.cpp:91-92) ...
    init["steps"][5] = capi.STEPLIM + 1            # ... on either side of it
    skipped = (init["steps"] < 0) | (init["steps"] >= (p.steplim if p.steplim > 0 else capi.STEPLIM))
    want, st_trace = api.trace(p, init)
    off1, rows1, traced1, out1, st1 = api.trace_paths(p, init, write_step=1)
    off7, rows7, traced7, out7, st7 = api.trace_paths(p, init, write_step=7)
    assert parity.same_records(out1, want) and parity.same_records(out7, want)
    assert st1["rays_traced"] == st_trace["rays_traced"] and st1["steps_total"] == st_trace["steps_total"]
    # the skip rule
    assert (traced1 == (~skipped).astype(np.uint8)).all() and (traced7 == traced1).all()
    assert (np.diff(off1)[skipped] == 0).all() and (np.diff(off7)[skipped] == 0).all()
    assert skipped.sum() >= 2 and (~skipped).sum() > 100
    # a second recording of the same input gives identical bytes
    off1b, rows1b, traced1b, out1b, _ = api.trace_paths(p, init, write_step=1)
    assert off1b.tobytes() == off1.tobytes() and rows1b.tobytes() == rows1.tobytes() and traced1b.tobytes() == traced1.tobytes() and out1b.tobytes() == out1.tobytes()
    u1, u7 = rows1.view(np.uint64), rows7.view(np.uint64)
    steps = np.abs(out1["steps"].astype(np.int64)) - np.where(skipped, 0, init["steps"])      # this call's own step count
    by_loop_condition = ~skipped & ((out1["status"] & (capi.STATUS_HORIZON | capi.STATUS_STEPLIM)) == 0)
    if p.stop_kind != capi.STOP_THETA:
        by_loop_condition &= (out1["status"] & capi.STATUS_DEST) == 0        # dest->reached() breaks before the write
    n_checked_last = 0
    for i in np.flatnonzero(~skipped):
        a, b = u1[off1[i]:off1[i + 1]], u7[off7[i]:off7[i + 1]]
        silent = steps[i] - len(a)                 # iterations that wrote nothing: theta flips, and the one that broke on the horizon / destination
        assert 0 <= silent and steps[i] // 7 - silent <= len(b) <= steps[i] // 7, (i, steps[i], len(a), len(b))
        # every coarse row appears in the fine recording, in order, bit for bit
        fine = iter(r.tobytes() for r in a)
        assert all(any(f == r.tobytes() for f in fine) for r in b), i
        if by_loop_condition[i] and steps[i] > 0:
            last = np.array([out1[f][i] for f in ("t", "r", "theta", "phi")]).view(np.uint64)
            assert len(a) and (a[-1] == last).all(), i
            n_checked_last += 1
    # (not vacuous: under the theta-limit overloads with the default step limit most rays end by the loop condition -- disc or r_max; a destination
    # that catches every ray, or a step limit below the rays' lengths, may leave none, and then the other checks are what the case is for)
    if p.stop_kind == capi.STOP_THETA and p.steplim <= 0:
        assert n_checked_last > (~skipped).sum() // 2
    print(f"paths consistency {case}/{run}{'/' + regime if regime else ''}: rays {int((~skipped).sum())}, rows ws=1 {len(rows1)}, ws=7 {len(rows7)}, steps {st1['steps_total']}, last-row checks {n_checked_last}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("run", ["euler", "rk4"])
def test_wave_boundaries_with_skipped_slots(run, n):
    """The recorder rides the trace's own loop (kr_trace_loop.hpp): what the 35-ray fixtures do not reach is a launch of one wave exactly full,
    one slot short, one slot over and three waves, with slots among them that the skip rule leaves out -- every third one unused (steps = -1;
    at n = 65 the second wave's only slot), one at the step limit.  The first n ps_h10 records: the traced slots end with the golden file's
    records under test_trace_vs_golden's bar for the strict fixed-step kernels (and with those of api.trace, bit for bit), the skipped slots keep
    their bytes, and traced[] / offsets / the last rows say the same."""
    case = gc.cases()["ps_h10"]
    p = capi.copy_params(case["runs"][run], flags=0)
    g = np.load(gc.golden_path("ps_h10"))
    steplim = p.steplim if p.steplim > 0 else capi.STEPLIM
    init = g["init"][:n].copy()
    init["steps"][1::3] = -1
    if n > 3:
        init["steps"][3] = steplim
    skipped = (init["steps"] < 0) | (init["steps"] >= steplim)
    offsets, rows, traced, out, st = api.trace_paths(p, init, write_step=1)
    # the skip rule: traced[], zero-width slabs, untouched records
    assert (traced == (~skipped).astype(np.uint8)).all() and st["rays_traced"] == int((~skipped).sum())
    assert offsets[0] == 0 and (np.diff(offsets) >= 0).all() and (np.diff(offsets)[skipped] == 0).all()
    assert offsets[n] == len(rows)
    assert out[skipped].tobytes() == init[skipped].tobytes()
    # the last row of a ray that ended by the loop condition is its final record
    by_loop_condition = ~skipped & ((out["status"] & (capi.STATUS_HORIZON | capi.STATUS_STEPLIM)) == 0) & (np.abs(out["steps"]) > 0)
    u = rows.view(np.uint64)
    for i in np.flatnonzero(by_loop_condition):
        last = np.array([out[f][i] for f in ("t", "r", "theta", "phi")]).view(np.uint64)
        assert offsets[i + 1] > offsets[i] and (u[offsets[i + 1] - 1] == last).all(), i
    want_trace, st_trace = api.trace(p, init)
    assert parity.same_records(out, want_trace) and st["steps_total"] == st_trace["steps_total"]
    # the traced slots against the reference's records, as test_gpu_parity.test_trace_vs_golden holds the strict Euler / RK4 trace to them
    got = out[~skipped]
    api.range_phi(got)
    V, rev, proj = case["post"]
    api.redshift(p.spin, V, rev, proj, got)
    res = parity.compare_rays(got, g[f"final__{run}"][:n][~skipped], rtol=parity.rtol_for(p), check_redshift=True, steps_slack=parity.steps_slack_for(p, 0))
    allowed = parity.allowed_bad_frac_strict(p, res["n_traced"])
    print(f"paths wave boundaries {run} n={n}: traced {res['n_traced']}, rows {len(rows)}, bad {res['n_bad']} (allowed share {allowed:.4f}), "
          f"bit-identical share {res['frac_bit_identical']:.4f}, last-row checks {int(by_loop_condition.sum())}")
    assert res["n_traced"] == int((~skipped).sum()) and res["frac_bad"] <= allowed, res


def test_count_pass_leaves_the_rays_alone_and_record_checks_its_slabs():
    """Device-pointer forms: the count pass does not modify d_rays; the record pass refuses a rows buffer smaller than offsets[n], and reports rays whose
    row count differs from the slab the offsets give them (here: offsets counted with another write_step) without writing outside the buffer."""
    L = api.lib()
    p = capi.copy_params(gc.cases()["ps_h10"]["runs"]["rk4"], flags=0)
    init = np.load(gc.golden_path("ps_h10"))["init"].copy()
    n = len(init)
    w = api.path_spec(write_step=3)
    with DeviceScope(L) as dev:
        d_rays, d_off, d_traced = dev.upload(init), dev.alloc((n + 1) * 8), dev.alloc(n)
        total = C.c_int64()
        capi.check(L, L.kr_trace_paths_count_dev_f64(C.byref(p), C.byref(w), d_rays, n, d_off, d_traced, C.byref(total), None), "count")
        assert dev.fetch(d_rays, n, init.dtype).tobytes() == init.tobytes()
        offsets = dev.fetch(d_off, n + 1, np.int64)
        assert offsets[0] == 0 and offsets[-1] == total.value > 0
        guard = 64                                                # rows beyond the buffer's nominal end, filled with a pattern
        d_rows = dev.alloc((total.value + guard) * 32)
        capi.check(L, L.kr_memset(d_rows, 0xA5, (total.value + guard) * 32), "memset")
        # too small a buffer: refused, nothing written
        rc = L.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w), d_rays, n, d_off, d_rows, total.value - 1, None, None)
        assert rc == capi.KR_EINVAL and b"total_rows is smaller than offsets[n]" in L.kr_last_error()
        # other parameters than the count pass had: every row stays inside its ray's slab, and the call says so
        w2 = api.path_spec(write_step=1)
        rc = L.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w2), d_rays, n, d_off, d_rows, total.value, None, None)
        assert rc == capi.KR_EINVAL and b"different number of rows" in L.kr_last_error()
        tail = dev.fetch(C.c_void_p(d_rows.value + total.value * 32), guard * 4, np.uint64)
        assert (tail == 0xA5A5A5A5A5A5A5A5).all()
        # the matching call on fresh rays succeeds and agrees with the host-pointer form
        capi.check(L, L.kr_memcpy_h2d(d_rays, init.ctypes.data_as(C.c_void_p), init.nbytes), "h2d")
        st = capi.Stats()
        capi.check(L, L.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w), d_rays, n, d_off, d_rows, total.value, None, C.byref(st)), "record")
        rows = dev.fetch(d_rows, total.value * 4).reshape(-1, 4)
        off_h, rows_h, _, out_h, st_h = api.trace_paths(p, init, write_step=3)
        assert off_h.tobytes() == offsets.tobytes() and rows_h.tobytes() == rows.tobytes()
        assert st.rays_traced == st_h["rays_traced"] and st.steps_total == st_h["steps_total"] and st.kernel_ms > 0


def test_empty_input():
    p = capi.copy_params(capi.default_params(0.998), integrator=capi.RK4)
    offsets, rows, traced, out, st = api.trace_paths(p, np.zeros(0, dtype=capi.RAY_F64))
    assert offsets.tolist() == [0] and rows.shape == (0, 4) and len(traced) == 0 and api.paths_text(offsets, rows, traced) == ""
