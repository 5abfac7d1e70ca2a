"""GPU: the two places where the recorders' shared wave-aggregated add (for_lane_groups, csrc/kr_recorder.hpp) can go wrong: more distinct keys in
one wave step than it has rounds (the lanes left over must add for themselves, exactly once), and a group that splits on a second key (the observer's
(energy, time) bin inside an energy bin).

The yardstick is the numpy rule (tests/volume_map_rules.py, tests/volume_observe_rules.py) on the path recorder's write_step = 1 rows, never the code
under test.  Every case runs ONE wave: 64 rays, none skipped, so all of them are claimed together and wave step k + 1 is iteration k + 1 of every ray.
A ray that never took a theta flip leaves a row at every iteration but a last one that ended on the horizon, so its row k is the product of wave step
k + 1 -- such rays are recognised on the CPU (rows == steps - ended_on_horizon), and each case asserts from the recording, over those rays alone, that
the situation it is about occurs (a ray that did flip only adds lanes to a step).  Linear axes only: counts and tallies are EQUAL by the argument of
volume_map_rules.py."""
import functools

import numpy as np
import pytest

import golden_cases as gc
import parity
import volume_map_rules as vr
import volume_observe_rules as vo
from raytrace_cpu_amd import api, capi
from test_gpu_volume_observe import fields
from test_gpu_volume_observe import grid as observe_grid
from test_gpu_volume_map import grid as map_grid

pytestmark = pytest.mark.gpu

ROUNDS = 8          # kAggRounds, csrc/kr_recorder.hpp
WAVE = 64


def spread(n_all):
    """64 indices spread evenly over n_all"""
    return np.linspace(0, n_all - 1, WAVE).astype(np.int64)


@functools.lru_cache(maxsize=None)
def one_wave(case, run, pick=spread):
    """(params, init, offsets, rows, the strict trace's records, aligned) of 64 traceable rays of a golden init, recorded once, read-only.
    aligned[ray]: the ray never flipped, so its row k belongs to wave step k + 1."""
    p = capi.copy_params(gc.cases()[case]["runs"][run], flags=0)
    full = np.load(gc.golden_path(case))["init"]
    usable = np.flatnonzero((full["steps"] >= 0) & (full["emit"] != 0))
    init = full[usable[pick(len(usable))]].copy()
    assert len(init) == WAVE
    offsets, rows, traced, out, _ = api.trace_paths(p, init, write_step=1)
    want, _ = api.trace(p, init)
    assert traced.all() and parity.same_records(out, want)
    ended_without_row = (want["status"] & (capi.STATUS_HORIZON | capi.STATUS_DEST)) != 0
    aligned = np.diff(np.asarray(offsets, dtype=np.int64)) == want["steps"].astype(np.int64) - ended_without_row
    for a in (init, offsets, rows, want, aligned):
        a.setflags(write=False)
    return p, init, np.asarray(offsets, dtype=np.int64), np.asarray(rows, dtype=np.float64).reshape(-1, 4), want, aligned


def per_step_groups(step, key):
    """For adds (step, key): per step that has any, (distinct keys, whether a key is shared by >= 2 adds, whether a key has exactly 1)."""
    if len(step) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)
    width = int(key.max()) + 1
    pair, count = np.unique(step.astype(np.int64) * width + key.astype(np.int64), return_counts=True)
    _, at = np.unique(pair // width, return_inverse=True)
    return np.bincount(at), np.bincount(at, weights=count >= 2) > 0, np.bincount(at, weights=count == 1) > 0


def step_of_rows(offsets):
    ray = vr.ray_of_rows(offsets)
    return ray, np.arange(offsets[-1]) - offsets[ray]


def map_deposits(m, spin, init, offsets, rows, aligned):
    """(wave step, cell) of the deposits of the aligned rays under the rule"""
    cell = vr.cells_of(m, rows)
    due = vr.due_rows(m, offsets, cell)
    g = vr.oracle_g(m, spin, init, offsets, rows, due, vr.signs_for(m, init, offsets, rows))
    with np.errstate(invalid="ignore"):
        deposit = np.flatnonzero(due)[(g > 0) & np.isfinite(g)]
    ray, step = step_of_rows(offsets)
    deposit = deposit[aligned[ray[deposit]]]
    return step[deposit], cell[deposit]


@pytest.mark.parametrize("run", ["euler", "rk4"])
def test_more_cells_in_a_wave_step_than_rounds(run):
    p, init, offsets, rows, want_records, aligned = one_wave("ps_h10", run)
    m = map_grid(12, 8, 12, 1)
    step, cell = map_deposits(m, p.spin, init, offsets, rows, aligned)
    distinct, shared, single = per_step_groups(step, cell)
    print(f"recorder groups, map {run}: aligned rays {int(aligned.sum())} / {WAVE}, steps with deposits {len(distinct)}, most distinct cells in a step "
          f"{int(distinct.max()) if len(distinct) else 0}, steps with more than {ROUNDS}: {int((distinct > ROUNDS).sum())}, steps with a shared and a lone cell "
          f"{int((shared & single).sum())}")
    assert (distinct > ROUNDS).any(), "no wave step deposits into more cells than the aggregation has rounds"
    assert (shared & single).any(), "no wave step has a cell that lanes share beside a cell of one lane"
    got = api.trace_volume(p, init, m)
    problems = vr.compare(got, vr.rule(m, p.spin, init, offsets, rows), parity.BIN_RTOL)
    assert not problems, problems
    assert parity.same_records(got["rays"], want_records)


def camera_wave(run, shape=(12, 8, 12)):
    p, init, offsets, rows, want_records, aligned = one_wave("ip15", run)
    m = observe_grid(*shape)
    emis, kappa, delay = fields(m)
    meas = vo.measure_recording(m, p.spin, init, offsets, rows, emis, kappa, delay)
    ray, step = step_of_rows(offsets)
    contributes = aligned[ray[meas["row"]]]
    return p, init, offsets, want_records, m, (emis, kappa, delay), meas, step[meas["row"]], contributes


def energy_bins(meas, nen, **time_bins):
    """nen linear bins across the 1st to 99th percentile of the E the rule finds, widened by a quarter of a bin at either end (as test_gpu_volume_observe.py)"""
    lo, hi = np.percentile(meas["E"], [1, 99])
    w = (hi - lo) / nen
    return api.observe_bins_struct(lo - 0.25 * w, hi + 0.25 * w, nen, **time_bins)


def observe_and_compare(p, init, m, b, cells, meas, offsets, want_records):
    assert vo.near_edge_e(meas, bins=b) == 0          # the precondition on the inputs
    got = api.trace_observe(p, init, m, b, *cells)
    problems = vo.compare(got, vo.bin_rows(b, meas), parity.BIN_RTOL)
    assert not problems, problems
    assert got["rows"] == int(offsets[-1]) and got["contributions"] > 100 and parity.same_records(got["rays"], want_records)
    return got


@pytest.mark.parametrize("run", ["euler", "rk4"])
def test_more_energy_bins_in_a_wave_step_than_rounds(run):
    p, init, offsets, want_records, m, cells, meas, step, contributes = camera_wave(run)
    chosen = None
    for nen in (32, 64, 128, 256, 512, 1024, 2048, 4096):          # the coarsest bins that spread a step's rays over more than ROUNDS of them
        b = energy_bins(meas, nen)
        q_e = vo.quotients(b, meas)[0]
        with np.errstate(invalid="ignore"):
            binned = contributes & (q_e >= 0) & (q_e < nen)
        distinct, shared, single = per_step_groups(step[binned], q_e[binned].astype(np.int64))
        if (distinct > ROUNDS).any() and vo.near_edge_e(meas, bins=b) == 0:
            chosen = (b, int(distinct.max()), int((distinct > ROUNDS).sum()), int((shared & single).sum()))
            break
    assert chosen is not None, "no number of energy bins spreads a wave step's contributions over more bins than the aggregation has rounds"
    b, most, steps_over, mixed = chosen
    print(f"recorder groups, observer {run}: {int(contributes.sum())} of {len(contributes)} contributions come from aligned rays, nen {b.nen}, most distinct bins in a step "
          f"{most}, steps with more than {ROUNDS}: {steps_over}, steps with a shared and a lone bin {mixed}")
    observe_and_compare(p, init, m, b, cells, meas, offsets, want_records)


@pytest.mark.parametrize("run", ["euler", "rk4"])
def test_energy_bin_shared_time_bin_split(run):
    p, init, offsets, want_records, m, cells, meas, step, contributes = camera_wave(run)
    assert len(np.unique(cells[2])) > 100          # the delay varies from cell to cell
    nen, nt = 2, 256
    b = energy_bins(meas, nen, t0=float(meas["T"].min()), tmax=float(np.nextafter(meas["T"].max(), np.inf)), nt=nt)
    q_e, q_t = vo.quotients(b, meas)
    with np.errstate(invalid="ignore"):
        binned = contributes & (q_e >= 0) & (q_e < nen) & (q_t >= 0) & (q_t < nt)
    e, t = q_e[binned].astype(np.int64), q_t[binned].astype(np.int64)
    # groups are (step, energy bin); inside each, the (energy, time) bins
    distinct, shared, _ = per_step_groups(step[binned] * nen + e, t)
    print(f"recorder groups, observer {run} nen {nen} nt {nt}: (step, energy bin) groups {len(distinct)}, that split over time bins {int((distinct >= 2).sum())}, "
          f"that also share one {int(((distinct >= 2) & shared).sum())}")
    assert ((distinct >= 2) & shared).any(), "no wave step has lanes of one energy bin in different time bins beside lanes that share one"
    got = observe_and_compare(p, init, m, b, cells, meas, offsets, want_records)
    assert (got["response"] > 0).sum() > 8
