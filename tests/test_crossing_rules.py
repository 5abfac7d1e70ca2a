"""CPU: the numpy crossing rule (tests/crossing_rules.py) on hand-made state sequences, before tests/test_gpu_crossings.py lets it judge the device
recorder: a zig-zag in theta with known crossing fractions, theta exactly on pi/2, a break iteration that crosses, more crossings than M in both stop
modes, skipped rays, and the choice an image of one order makes."""
import math

import numpy as np
import pytest

import crossing_rules as cr
import golden_cases as gc
from raytrace_cpu_amd import api, capi

H = cr.HALF_PI


def make(sequences, break_status=None, stop_kind=capi.STOP_THETA):
    """(params, init, offsets, rows, traced, final) of rays whose states are `sequences` (lists of (t, r, theta, phi)); break_status[i] != 0: the last
    state of ray i is that of a break iteration which added these status bits (it has no row); a sequence of None is a skipped ray."""
    n = len(sequences)
    p = capi.copy_params(capi.default_params(0.5), integrator=capi.RK4, stop_kind=stop_kind)
    init, final = np.zeros(n, dtype=capi.RAY_F64), np.zeros(n, dtype=capi.RAY_F64)
    init["k"], init["h"], init["Q"], init["emit"], init["rdot_sign"], init["thetadot_sign"] = 1.0, 0.7, 9.0, 1.1, -1, 1
    offsets, rows, traced = [0], [], np.zeros(n, dtype=np.uint8)
    for i, seq in enumerate(sequences):
        if seq is None:
            init["steps"][i] = -1
            final[i] = init[i]
            offsets.append(offsets[-1])
            continue
        traced[i] = 1
        seq = np.asarray(seq, dtype=np.float64)
        broke = int(break_status[i]) if break_status is not None else 0
        body = seq[1:-1] if broke else seq[1:]
        rows.extend(body.tolist())
        offsets.append(offsets[-1] + len(body))
        final[i] = init[i]
        for q, c in enumerate(cr.COLS):
            init[c][i] = seq[0][q]
            final[c][i] = seq[-1][q]
        final["status"][i] = broke
        final["steps"][i] = len(seq) - 1
    return p, init, np.asarray(offsets, dtype=np.int64), np.asarray(rows, dtype=np.float64).reshape(-1, 4), traced, final


def zigzag(thetas, r0=10.0, dr=-0.5, dphi=0.25, dt=2.0):
    return [(dt * k, r0 + dr * k, th, dphi * k) for k, th in enumerate(thetas)]


def test_crossed_is_the_traces_own_test():
    below, above = np.nextafter(H, 0), np.nextafter(H, 4)
    cases = [(1.0, 2.0, True), (2.0, 1.0, True), (1.0, 1.5, False), (2.0, 1.6, False), (below, H, True), (above, H, True), (H, above, False), (H, below, False),
             (H, H, False), (np.nan, 2.0, False), (1.0, np.nan, False)]
    for before, after, want in cases:
        assert bool(cr.crossed(before, after)) is want, (before, after)


def test_zigzag_with_known_fractions():
    thetas = [H - 0.3, H + 0.1, H + 0.2, H - 0.2, H - 0.1, H + 0.3]
    args = make([zigzag(thetas)])
    got = cr.rule(args[0], api.crossing_spec(4, False), *args[1:])
    assert got["seen"].tolist() == [3] and not got["ended"][0]
    # crossings in the iterations 0 -> 1 (f = 3/4), 2 -> 3 (f = 1/2), 4 -> 5 (f = 1/4)
    for m, (k, f) in enumerate(((0, 0.75), (2, 0.5), (4, 0.25))):
        r_c, phi_c, t_c, g = got["rows"][0, m]
        assert r_c == pytest.approx(10.0 - 0.5 * (k + f), abs=1e-13) and phi_c == pytest.approx(0.25 * (k + f), abs=1e-13) and t_c == pytest.approx(2.0 * (k + f), abs=1e-13)
        # and bit for bit the rule's own expressions in Python floats (IEEE doubles, one operation each)
        th0, th1 = thetas[k], thetas[k + 1]
        fq = (H - th0) / (th1 - th0)
        r0, r1 = 10.0 - 0.5 * k, 10.0 - 0.5 * (k + 1)
        assert r_c == r0 + fq * (r1 - r0)
        assert t_c == 2.0 * k + fq * (2.0 * (k + 1) - 2.0 * k)
        assert np.isfinite(g) and g > 0
    assert np.isnan(got["rows"][0, 3]).all()


def test_theta_exactly_on_the_plane():
    """Landing ON pi/2 is a crossing with f = 1; leaving it is none, in either direction (before is neither below nor above)."""
    args = make([zigzag([H - 0.2, H, H + 0.2]), zigzag([H + 0.2, H, H + 0.1]), zigzag([H, H - 0.1, H - 0.2])])
    got = cr.rule(args[0], api.crossing_spec(4, False), *args[1:])
    assert got["seen"].tolist() == [1, 1, 0]
    assert got["rows"][0, 0, 0] == 10.0 + 1.0 * (9.5 - 10.0) and got["rows"][0, 0, 2] == 2.0
    assert np.isnan(got["rows"][2]).all()


@pytest.mark.parametrize("status,kind", [(capi.STATUS_HORIZON, capi.STOP_THETA), (capi.STATUS_DEST, capi.STOP_DISC_ISCO)])
def test_a_break_iteration_that_crosses_counts(status, kind):
    seq = zigzag([H - 0.3, H - 0.1, H + 0.1])
    args = make([seq], break_status=[status], stop_kind=kind)
    assert args[2].tolist() == [0, 1]                       # (the break iteration left no row)
    found = cr.all_crossings(*args)
    assert found["ray"].tolist() == [0] and found["in_break"].tolist() == [True] and found["after"].tolist() == [2]
    got = cr.rule(args[0], api.crossing_spec(2, True), *args[1:])
    assert got["seen"].tolist() == [1] and not got["ended"][0]
    assert got["rows"][0, 0, 0] == pytest.approx(9.5 - 0.25, abs=1e-13)


def test_theta_limit_dest_is_not_a_break_iteration():
    """Without a destination the DEST bit comes from the epilogue: the last iteration has a row, and the final record repeats it."""
    seq = zigzag([H - 0.3, H - 0.1, H + 0.1])
    p, init, offsets, rows, traced, final = make([seq])
    final["status"][0] = capi.STATUS_DEST
    found = cr.all_crossings(p, init, offsets, rows, traced, final)
    assert found["n_states"].tolist() == [3] and found["in_break"].tolist() == [False]


@pytest.mark.parametrize("stop", [False, True], ids=["run_on", "stop_when_full"])
@pytest.mark.parametrize("M", [1, 2, 4])
def test_more_crossings_than_stored(M, stop):
    thetas = [H - 0.1, H + 0.1, H - 0.1, H + 0.1, H - 0.1]       # four crossings
    args = make([zigzag(thetas), None, zigzag(thetas[:2])])
    got = cr.rule(args[0], api.crossing_spec(M, stop), *args[1:])
    full = stop and M <= 4
    assert got["seen"].tolist() == [M if full else 4, 0, 1]
    assert got["ended"].tolist() == [full, False, stop and M == 1]
    stored = min(M, 4)
    assert np.isfinite(got["rows"][0, :stored]).all() and np.isnan(got["rows"][0, stored:]).all()
    assert np.isnan(got["rows"][1]).all()                          # (the skipped ray)
    if full:
        # the ray ends with the state of the iteration that made crossing M - 1: state M of the zig-zag
        assert got["end_state"][0].tolist() == [2.0 * M, 10.0 - 0.5 * M, thetas[M], 0.25 * M]
    else:
        assert np.isnan(got["end_state"][0]).all()
    # the stored crossings do not depend on the stop mode or on M
    ref = cr.rule(args[0], api.crossing_spec(4, False), *args[1:])
    assert got["rows"][0, :stored].tobytes() == ref["rows"][0, :stored].tobytes()


def test_which_crossing_an_order_takes():
    ip = gc.cases()["ip16"]["source"]
    bins = gc.image_bins(ip)                      # r_isco ~ 1.24, r_disc = 30
    rows = np.full((5, 3, 4), np.nan)
    rows[0, :, 0] = (50.0, 5.0, 3.0)              # first crossing outside the disc: the opaque disc takes the second
    rows[1, :, 0] = (0.5, np.nan, 7.0)            # inside the ISCO, NaN, in range
    rows[2, :, 0] = (50.0, 40.0, 31.0)            # never in range
    rows[3, :, 0] = (2.0, 3.0, 4.0)
    rows[4, :, 0] = (2.0, 3.0, 4.0)               # seen = 0: nothing stored, whatever the slab holds
    seen = np.array([3, 3, 5, 1, 0], dtype=np.int32)
    assert cr.pick(bins, rows, seen, -1).tolist() == [1, 2, -1, 0, -1]
    assert cr.pick(bins, rows, seen, 0).tolist() == [0, 0, 0, 0, -1]
    assert cr.pick(bins, rows, seen, 1).tolist() == [1, 1, 1, -1, -1]
    assert cr.pick(bins, rows, seen, 2).tolist() == [2, 2, 2, -1, -1]


def test_image_rule_is_the_image_rule_on_synthetic_records():
    import reducer_rules as rr
    ip = gc.cases()["ip16"]["source"]
    bins = gc.image_bins(ip)
    rays = np.zeros(3, dtype=capi.RAY_F64)
    rays["alpha"], rays["beta"] = (-10.0, 3.0, 3.0), (5.0, -7.0, -7.0)
    rows = np.full((3, 2, 4), np.nan)
    rows[0, 0] = (6.0, 7.0, 100.0, 0.8)           # phi = 7 wraps to 7 - 2 pi
    rows[1, 0] = (8.0, -1.0, 110.0, -0.5)         # g <= 0: filtered
    rows[1, 1] = (9.0, 1.0, 120.0, 1.2)
    rows[2, 0] = (12.0, 0.5, 130.0, 0.9)
    seen = np.array([1, 2, 1], dtype=np.int32)
    img0, img1 = cr.image_rule(bins, rays, rows, seen, 0), cr.image_rule(bins, rays, rows, seen, 1)
    assert img0["disc_count"] == 2 and img0["nrays"].sum() == 2 and img1["disc_count"] == 1
    ok, _, _, px = rr.image_pixel(bins, rays["alpha"], rays["beta"])
    assert ok.all() and img0["nrays"][px[0]] == 1 and img0["nrays"][px[2]] == 1 and img1["nrays"][px[1]] == 1
    assert img0["phi"][px[0]] == 7.0 - 2 * math.pi and img0["r"][px[0]] == 6.0 and img0["time"][px[2]] == 130.0
    assert img0["enshift"][px[0]] == 1.0 / 0.8 and img1["r"][px[1]] == 9.0
