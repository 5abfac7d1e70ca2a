"""GPU: the wave-uniform guards of the fast Euler / RK4 step (kr_device.hpp::step_fixed: the quiet-step guard at the end of the step, the guard in front
of the shared time / azimuth cap; profiles/uniform_guards_ab.txt).  A shortcut that a WAVE takes must not show in a RAY's record:

(A) company invariance.  The refill grid of tests/test_gpu_fast_ray_consts.py (a) in index order, (b) dealt round-robin by traced step count, so that every
    block of 64 consecutive slots spans all ray lengths -- mixed waves, in which some lane ends, is reflected or has its cap bind on most steps: the code
    behind the guards runs -- and (c) 256 rays as one batch of 256 single-ray traces: one live lane per wave, so every shortcut is taken whenever that one ray
    qualifies.  All three field by field (parity.same_records).
(B) restarts.  An interrupted trace picks the ray up with fresh lanes in fresh company; the rule of tests/test_gpu_fast_step_diet.py::restart_rule says
    for which rays that is the identity.  Cuts at 8 and 150 steps and at the two steps of a ladder between which most of this grid's rays pass theta = pi/4
    (read off interrupted traces of the grid, not written down here).
(C) the guards one lane at a time, through the probe kernel (include/kr_trace.h, ops 26-28): what a lane gets that leaves through the guard against what
    the code behind the guard gives for the same operands, bit for bit."""
import functools
import math

import numpy as np
import pytest

import parity
import step_control_cases as sc
import test_gpu_fast_ray_consts as frc
import test_gpu_fast_step_diet as diet
from raytrace_cpu_amd import api, capi
from test_gpu_primitives import probe

pytestmark = pytest.mark.gpu

MODES, METHODS = frc.MODES, frc.METHODS


# ---- (A) a record does not depend on its wave-mates -----------------------------------------------------------------------------------------------------
def round_robin_by_length(steps):
    """A permutation that deals the rays, sorted by length, round-robin into the slots: slot p takes the (p // 64)-th ray of the (p % 64)-th of 64 equal
    strata of the sorted list, so that 64 consecutive slots hold one ray of every stratum."""
    order = np.argsort(np.abs(steps.astype(np.int64)), kind="stable")
    m = -(-len(order) // 64)
    table = np.full(64 * m, -1, dtype=np.int64)
    table[:len(order)] = order
    dealt = table.reshape(64, m).T.ravel()
    return dealt[dealt >= 0]


def kinds(out, init, p):
    """The kinds of ray the single-ray batch has to contain, as masks over the index-order trace."""
    live = init["steps"] != -1
    with np.errstate(invalid="ignore"):
        return {
            "radial turning point": live & (out["rdot_flips"] > 0),
            "thetadot_sign changed": live & (out["thetadot_sign"] != init["thetadot_sign"]),
            "near-axis ray": live & (np.abs(init["h"]) < 1e-3),
            "ends on the horizon": live & ((out["status"] & capi.STATUS_HORIZON) != 0),
            "ends at r_max": live & (out["r"] >= p.r_max),
            "ends on the disc": live & (out["theta"] >= p.theta_max) & (out["r"] < p.r_max),
            "ends in quadrant 0": live & (out["theta"] < math.pi / 4),
            "ends in quadrant 1": live & (out["theta"] > math.pi / 4) & (out["theta"] < 3 * math.pi / 4),
        }


def picks_of(out, init, p, n=256):
    """n ray indices: up to n // 16 of every kind, spread evenly over that kind's rays, the rest spread evenly over the live rays."""
    chosen = []
    for mask in kinds(out, init, p).values():
        idx = np.flatnonzero(mask)
        chosen.extend(idx[np.linspace(0, len(idx) - 1, min(len(idx), n // 16)).astype(int)] if len(idx) else [])
    chosen = list(dict.fromkeys(int(i) for i in chosen))
    live = np.flatnonzero(init["steps"] != -1)
    for i in live[np.linspace(0, len(live) - 1, 4 * n).astype(int)]:
        if len(chosen) >= n:
            break
        if int(i) not in chosen:
            chosen.append(int(i))
    return np.array(chosen[:n])


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_mixed_waves_give_the_index_order_records(krlib, integrator, flags):
    grid = frc.refill_grid()
    rays = sc.init(grid)
    want, st_want = frc.single_trace(integrator, flags)
    perm = round_robin_by_length(want["steps"])
    assert sorted(perm.tolist()) == list(range(len(rays)))
    # every block of 64 slots spans the lengths: its shortest ray is among the shortest 5 % of all, its longest among the longest 5 %
    length = np.abs(want["steps"].astype(np.int64))[perm][:len(perm) // 64 * 64].reshape(-1, 64)
    lo, hi = np.quantile(np.abs(want["steps"].astype(np.int64)), [0.05, 0.95])
    assert (length.min(axis=1) <= lo).all() and (length.max(axis=1) >= hi).all()
    got, st = api.trace(frc.params(integrator, flags, grid), np.ascontiguousarray(rays[perm]))
    assert st["rays_traced"] == st_want["rays_traced"] > frc.RESIDENT_LANES
    assert st["steps_total"] == st_want["steps_total"] == sc.steps_total(want)
    assert parity.same_records(got, want[perm])


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_lone_lanes_give_the_index_order_records(krlib, integrator, flags):
    grid = frc.refill_grid()
    rays = sc.init(grid)
    p = frc.params(integrator, flags, grid)
    want, _ = frc.single_trace(integrator, flags)
    picks = picks_of(want, rays, p)
    assert len(picks) == 256 == len(set(picks.tolist()))
    present = {name: int(mask[picks].sum()) for name, mask in kinds(want, rays, p).items()}
    print(f"single-ray batch {frc.METHOD_NAME[integrator]}-{frc.MODE_NAME[flags]}: {present}")
    assert all(present.values()), present
    outs, stats = diet.batch_of(p, [np.ascontiguousarray(rays[i:i + 1]) for i in picks])
    assert all(st["rays_traced"] == 1 for st in stats)
    assert parity.same_records(np.concatenate(outs), want[picks])


# ---- (B) restarts ---------------------------------------------------------------------------------------------------------------------------------------
LADDER = (64, 128, 192, 256, 320, 384, 448, 512)


@functools.lru_cache(maxsize=None)
def cuts_round_pi_4(integrator, flags):
    """The two neighbouring steps of LADDER between which the share of in-flight rays beyond theta = pi/4 grows most, from interrupted traces of the grid."""
    share = []
    for cut in LADDER:
        part, was_cut = diet.interrupted(integrator, flags, cut)
        share.append(float((part["theta"][was_cut] > math.pi / 4).mean()) if was_cut.any() else 1.0)
    k = int(np.argmax(np.diff(share)))
    print(f"share of in-flight rays beyond pi/4 after {LADDER} steps: {[round(s, 3) for s in share]}")
    return LADDER[k], LADDER[k + 1]


@pytest.mark.parametrize("cut", ["8", "150", "before pi/4", "after pi/4"])
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_restart_reproduces_the_uninterrupted_trace(krlib, integrator, flags, cut):
    cut = int(cut) if cut.isdigit() else cuts_round_pi_4(integrator, flags)[cut.startswith("after")]
    init = sc.init(frc.refill_grid())
    want, _ = frc.single_trace(integrator, flags)
    part, was_cut = diet.interrupted(integrator, flags, cut)
    got = diet.resumed(integrator, flags, part, was_cut)
    must = diet.restart_rule(init, part, was_cut, flags)
    assert must.sum() > 0.9 * was_cut.sum() and was_cut.sum() > 1000
    equal = np.ones(len(want), dtype=bool)
    for f in want.dtype.names:
        x, y = got[f], want[f]
        equal &= (x.view(f"u{x.dtype.itemsize}") == y.view(f"u{y.dtype.itemsize}")) | ((x != x) & (y != y)) if x.dtype.kind == "f" else (x == y)
    print(f"restart {frc.METHOD_NAME[integrator]}-{frc.MODE_NAME[flags]} cut {cut}: cut {int(was_cut.sum())}, under the rule {int(must.sum())}, "
          f"equal among them {int((equal & must).sum())}")
    assert equal[must].all(), np.flatnonzero(must & ~equal)[:10]
    assert parity.same_records(got[~was_cut], want[~was_cut])


# ---- (C) the guards, one lane at a time -------------------------------------------------------------------------------------------------------------------
def same_bits(x, y):
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


def ulp_steps(x, ks):
    """x moved by k ulps for every k of ks (x finite, non-zero)."""
    return (np.array([x]).view(np.int64)[0] + np.asarray(ks, dtype=np.int64) * (1 if x > 0 else -1)).view(np.float64)


def test_cap_guard_lets_through_only_lanes_the_cap_leaves_alone(krlib):
    rng = np.random.default_rng(20261020)
    inf, nan, tiny = np.inf, np.nan, 5e-324
    triples = []                                                        # (step, m, num)
    # the cap a few ulps above, at and below the step: num = step m (1 + k ulp), over the magnitudes the step meets and far beyond them
    for e_step, e_m in [(-3, 0), (0, 0), (2, -4), (-12, 8), (5, 3), (-150, -150), (-160, 160), (100, 100), (-300, 10), (-300, -10), (10, 300), (-5, 307)]:
        for _ in range(40):
            step, m = rng.uniform(1, 2) * 10.0 ** e_step, rng.uniform(1, 2) * 10.0 ** e_m
            with np.errstate(all="ignore"):
                exact = step * m
            if not (np.isfinite(exact) and exact > 0):
                continue
            for num in np.concatenate([ulp_steps(exact, range(-6, 7)), exact * (1 + np.array([-1e-10, 1e-10, -2.0 ** -40, 2.0 ** -40, -2.0 ** -41, 2.0 ** -39, -2.0 ** -44, 2.0 ** -44]))]):
                triples.append((step, m, num))
    specials = [0.0, tiny, 1e-310, 2.3e-308, 1e-300, 1.0, 1e300, 1.7e308, inf, nan]
    for step in [0.0, tiny, 1e-310, 1e-3, 1.0, 1e300, inf, nan]:
        for m in specials:
            for num in specials:
                triples.append((step, m, num))
    t = np.array(triples)
    a = np.ascontiguousarray(t[:, [0, 2]]).ravel()                     # step, num
    b = np.ascontiguousarray(np.repeat(t[:, 1], 2))                    # m, m
    out = probe(26, a, b).reshape(-1, 2)
    same = same_bits(out[:, 0].copy(), out[:, 1].copy())
    guard_passed = same_bits(out[:, 0].copy(), t[:, 0].copy())
    print(f"cap guard: {len(t)} triples, of them with the step left alone {int(guard_passed.sum())}, changed by the cap {int((~same_bits(out[:, 1].copy(), t[:, 0].copy())).sum())}")
    assert same.all(), t[~same][:10]
    # the probe is not vacuous: the cap binds on some triples and leaves others alone
    assert (~same_bits(out[:, 1].copy(), t[:, 0].copy())).sum() > 1000 and guard_passed.sum() > 1000


def test_quiet_step_guard_lets_through_only_lanes_nothing_happens_to(krlib):
    horizon, r_max, pi, nan, inf = 1.0625, 1000.0, math.pi, np.nan, np.inf          # (the probe's launch: include/kr_trace.h)
    near = lambda x: list(ulp_steps(x, range(-4, 5)))
    rs = near(horizon) + near(r_max) + [1.5, 10.0, 999.0, 0.5, 2000.0, nan, inf, -1.0]
    cases = []                                                          # (r, theta, theta_max, theta_prev)
    for theta_max in [pi / 2, 1.0, 2.0, -1.0, -2.0, 0.0, pi, -pi / 2, 4.0, nan]:
        lo, hi = (-inf, theta_max) if theta_max > 0 else (-theta_max, inf) if theta_max < 0 else (-inf, inf)
        edges = [x for x in (abs(theta_max), pi / 2, pi) if x > 0] + [0.0]
        thetas = [0.0, -0.0, 5e-324, -5e-324, 1e-3, 0.7, 1.2, 1.7, 2.5, 3.1, -0.3, 3.3, 7.0, nan, inf, -inf]
        for e in edges:
            thetas += near(e) if e != 0.0 else []
        # theta_prev passed the loop condition (lo < theta_prev < hi), on either side of the equator where the interval has both
        prevs = [x for x in (0.3, 1.0 - 1e-9, 1.3, 1.9, 2.9, -0.2, 3.5) if lo < x < hi] or [1.0]
        for r in rs:
            for theta in thetas:
                for prev in prevs:
                    cases.append((r, theta, theta_max, prev))
    t = np.array(cases)
    a = np.ascontiguousarray(t[:, [0, 1]]).ravel()
    b = np.ascontiguousarray(t[:, [2, 3]]).ravel()
    for op, what in ((27, "outcome"), (28, "theta")):
        out = probe(op, a, b).reshape(-1, 2)
        same = same_bits(out[:, 0].copy(), out[:, 1].copy())
        assert same.all(), (what, t[~same][:10], out[~same][:10])
    outcome = probe(27, a, b).reshape(-1, 2)[:, 1]
    print(f"quiet-step guard: {len(t)} cases; nothing happens in {int((outcome == 0).sum())}, finished {int((outcome.astype(int) & 1 > 0).sum())}, "
          f"horizon {int((outcome.astype(int) & 2 > 0).sum())}, crossings {int((outcome.astype(int) & 4 > 0).sum())}, reflections {int((outcome.astype(int) & 8 > 0).sum())}")
    assert all(((outcome.astype(int) & bit) > 0).sum() > 100 for bit in (1, 2, 4, 8)) and (outcome == 0).sum() > 100
