"""GPU: the fast Euler / RK4 step without its non-arithmetic instructions (profiles/fast_step_diet_ab.txt).  Three things the change can get wrong:

(1) The theta-limit kernels keep a ray's two velocity signs as DOUBLES beside the integers of the record (kr_fast.hpp::FastRaySigns): set where a lane
    takes its ray, converted again wherever an integer flips -- the polar and the radial turning point of k1_with_flips_fast, reflect_poles.  Stale doubles
    (a lane's second ray stepping with its first ray's) need a launch whose lanes refill, so the grid, the one-wave-per-SIMD flag and the cached
    index-order traces are those of tests/test_gpu_fast_ray_consts.py: a record must not depend on which lane had which ray before -- a fixed permutation
    through kr_trace, and a merged batch of the rays and their permutation, against the index-order trace, field by field (NaN = NaN).
(2) A double that misses one of the three flip sites is wrong the same way in every order; it shows against a trace that was INTERRUPTED after the flip,
    because a lane that takes a stored ray converts the record's integers afresh.  Rays are cut with a small steplim, traced on to the end, and compared
    with the uninterrupted trace wherever the library before this change gives equality.  That set was established with that library
    (profiles/fast_step_diet_ab.txt) and is stated here as a rule, not as bits; see restart_rule().
(3) kr_sincos_fast_core_f64's quadrant fix-up forms the two sign bits with one three-input bit operation each.  The routine is shared by the float
    kernels and O(N) passes, so its values are pinned: the probe kernel's sine and cosine of 2e5 arguments -- all four quadrants, both signs, the
    neighbourhood of the multiples of pi/2 down to single ulps -- against a digest taken from the library before the change
    (tests/golden/fast_sincos_digest.json), against the strict routine (2 ulp: kr_sincos.hpp's "<= ~1.5 ulp", the 2 ulp tests/test_sincos_accuracy.py holds the
    routine to on the host), and with the exact sign in every quadrant."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import golden_cases as gc
import parity
import step_control_cases as sc
import test_gpu_fast_ray_consts as frc
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope
from test_gpu_primitives import probe, ulps

pytestmark = pytest.mark.gpu

MODES, METHODS = frc.MODES, frc.METHODS
DIGEST_FILE = os.path.join(gc.ROOT, "tests", "golden", "fast_sincos_digest.json")


# ---- (1) a lane's sign doubles belong to the ray it holds ---------------------------------------------------------------------------------------------
def permutation(n):
    return np.random.default_rng(20261019).permutation(n)


def kinds_present(out, init):
    """Which of the three flip sites the traced set visits, read off the records."""
    live = init["steps"] != -1
    return {
        "radial turning points": bool((out["rdot_flips"][live] > 0).any()),
        "equator crossings (polar motion through the plane)": bool((out["equatorial_crossings"][live] > 0).any()),
        # a polar turning point or a pole reflection: the only two ways a ray's thetadot_sign changes
        "polar sign flips": bool((out["thetadot_sign"][live] != init["thetadot_sign"][live]).any()),
        # a pole reflection proper: reflect_poles adds pi to phi each time, and only rays next to the axis (the source sits at theta = 1e-3) meet it; a ray
        # that starts towards the near pole (thetadot_sign < 0 at theta = 1e-3 with h != 0 turns before it, with h ~ 0 it crosses) ends with its sign changed
        "near-axis rays": bool((live & (np.abs(init["h"]) < 1e-3)).any()),
    }


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_every_flip_site_is_visited(krlib, integrator, flags):
    init = sc.init(frc.refill_grid())
    out, st = frc.single_trace(integrator, flags)
    assert st["rays_traced"] > frc.RESIDENT_LANES          # lanes are reused
    present = kinds_present(out, init)
    assert all(present.values()), present


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_permuted_trace_equals_the_index_order_trace(krlib, integrator, flags):
    grid = frc.refill_grid()
    rays = sc.init(grid)
    want, st_want = frc.single_trace(integrator, flags)
    perm = permutation(len(rays))
    got, st = api.trace(frc.params(integrator, flags, grid), np.ascontiguousarray(rays[perm]))
    assert st["rays_traced"] == st_want["rays_traced"] > frc.RESIDENT_LANES
    assert st["steps_total"] == st_want["steps_total"] == sc.steps_total(want)
    assert parity.same_records(got, want[perm])


def batch_of(p, inputs):
    """One kr_trace_batch_async_f64 batch over `inputs` (host arrays): the traced arrays and the stats."""
    krlib = api.lib()
    with DeviceScope(krlib) as dev:
        bufs = [dev.upload(h) for h in inputs]
        stats = [api.trace_wait(t) for t in api.trace_batch_async([p] * len(inputs), [d.value for d in bufs], [len(h) for h in inputs])]
        outs = [dev.fetch(d, len(h), h.dtype) for d, h in zip(bufs, inputs)]
    return outs, stats


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_merged_batch_of_two_equals_the_index_order_trace(krlib, integrator, flags):
    """The rays and their permutation as one batch: with KR_FLAG_HYBRID one trace_multi_kernel main launch over both (its instances carry the signs too)."""
    grid = frc.refill_grid()
    rays = sc.init(grid)
    want, st_want = frc.single_trace(integrator, flags)
    perm = permutation(len(rays))
    outs, stats = batch_of(frc.params(integrator, flags, grid), [np.ascontiguousarray(rays), np.ascontiguousarray(rays[perm])])
    for st in stats:
        assert st["rays_traced"] == st_want["rays_traced"] and st["steps_total"] == st_want["steps_total"]
    assert parity.same_records(outs[0], want)
    assert parity.same_records(outs[1], want[perm])


# ---- (2) a mid-flight restart keeps the signs ---------------------------------------------------------------------------------------------------------
# steps before the interruption.  Most rays are still in flight at any of them (median ~450 steps).  The source sits next to the pole, so a ray moves towards
# the pole only in its first steps: the records stored after 8 steps are the ones that carry thetadot_sign = -1; by 150 most turning points lie behind a ray.
CUTS = (8, 40, 150)


def interrupted(integrator, flags, cut):
    """The refill grid traced for `cut` steps: (records, mask of the rays that were cut)."""
    grid = frc.refill_grid()
    part, _ = api.trace(sc.grid_params(sc.DEFAULT, integrator, grid, flags=flags | frc.ONE_WAVE_PER_SIMD, steplim=cut), sc.init(grid))
    was_cut = (part["steps"] == -cut) & ((part["status"] & capi.STATUS_STEPLIM) != 0)
    return part, was_cut


def resumed(integrator, flags, part, was_cut):
    """The cut rays traced on to the end (everything else is an unused slot for that call), put back among the rays that had ended before the cut."""
    stored = part.copy()
    stored["steps"][was_cut] = -stored["steps"][was_cut]
    stored["status"][was_cut] &= ~capi.STATUS_STEPLIM
    stored["steps"][~was_cut] = -1
    cont, _ = api.trace(frc.params(integrator, flags, frc.refill_grid()), stored)
    out = part.copy()
    out[was_cut] = cont[was_cut]
    return out


def restart_rule(init, part, was_cut, flags):
    """The rays for which an interrupted trace must reproduce the uninterrupted one, bit for bit.

    A call's two turning-point latches are locals of the call (raytracer.cpp:767-768: r_was_positive = false, theta_was_positive = true at entry), so a
    restart is NOT the identity for a ray that is stored
      * on the step of a polar turning point: thetadot^2 < 0 at the stored point.  The uninterrupted trace has just flipped there and does not flip again;
        the restarted call sees a negative thetadot^2 with a fresh latch and does;
      * on the step of a radial turning point, rdot^2 <= 0 at the stored point: the uninterrupted trace flips, the restarted call (latch false) does not.
    Both are read off the stored record -- the potentials N and R of kr_fast.hpp::potentials_fast, in numpy, with a guard band of 1e-9 of their terms
    for the last bits in which numpy and the kernel differ.  With KR_FLAG_HYBRID the launch also decides per ray, from the state it is handed, which
    arithmetic traces it (kr_trace.hip::ill_conditioned): a stored ray can be classified otherwise than it was at emission, so the knife-edge column
    (parity.knife_edge_mask) and the rays within the classifier's own 1e-9 band at either point are left out as well."""
    a = 0.998
    k, h, Q, r, th = part["k"], part["h"], part["Q"], part["r"], part["theta"]
    with np.errstate(all="ignore"):
        s2, c2 = np.sin(th) ** 2, np.cos(th) ** 2
        ak = a * k
        n_terms = np.abs(Q) + c2 * (ak * ak + h * h / s2)
        N = Q + c2 * (ak * ak - h * h / s2)
        delta = r * r - 2.0 * r + a * a
        P = (r * r + a * a) * k - a * h
        r_terms = P * P + np.abs(delta) * (np.abs(Q) + (h - ak) ** 2)
        R = P * P - delta * (Q + (h - ak) ** 2) - delta * (np.abs(N) - N)
    ok = was_cut & (N > 1e-9 * n_terms) & (R > 1e-9 * r_terms)
    if flags & capi.FLAG_HYBRID:
        def near_classifier(rec):
            with np.errstate(all="ignore"):
                cs, sn = np.cos(rec["theta"]), np.sin(rec["theta"])
                kac, hcs = rec["k"] * a * cs, rec["h"] * cs / sn
                prod = (kac + hcs) * (kac - hcs)
                return ~(np.abs(rec["Q"] + prod) > 1e-8 * (np.abs(rec["Q"]) + np.abs(prod))) | ~(np.abs(rec["h"]) >= 1e-12)
        ok &= ~parity.knife_edge_mask(init, False) & ~near_classifier(init) & ~near_classifier(part)
    return ok


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_restart_mid_flight_reproduces_the_uninterrupted_trace(krlib, integrator, flags, cut):
    init = sc.init(frc.refill_grid())
    want, _ = frc.single_trace(integrator, flags)
    part, was_cut = interrupted(integrator, flags, cut)
    got = resumed(integrator, flags, part, was_cut)
    must = restart_rule(init, part, was_cut, flags)
    # the stored records carry what the restart has to pick up: a negative rdot_sign on many of them at every cut, a negative thetadot_sign at the first
    n_r, n_th = int((part["rdot_sign"][must] == -1).sum()), int((part["thetadot_sign"][must] == -1).sum())
    print(f"restart {frc.METHOD_NAME[integrator]}-{frc.MODE_NAME[flags]} cut {cut}: stored with rdot_sign = -1: {n_r}, with thetadot_sign = -1: {n_th}")
    assert n_r > 1000 and (n_th > 1000 or cut != CUTS[0])
    assert must.sum() > 0.9 * was_cut.sum() > 0.5 * (init["steps"] != -1).sum()
    equal = np.ones(len(want), dtype=bool)
    for f in want.dtype.names:
        x, y = got[f], want[f]
        equal &= (x.view(f"u{x.dtype.itemsize}") == y.view(f"u{y.dtype.itemsize}")) | ((x != x) & (y != y)) if x.dtype.kind == "f" else (x == y)
    print(f"restart {frc.METHOD_NAME[integrator]}-{frc.MODE_NAME[flags]} cut {cut}: cut {int(was_cut.sum())}, under the rule {int(must.sum())}, "
          f"equal among them {int((equal & must).sum())}, equal among the other cut rays {int((equal & was_cut & ~must).sum())} of {int((was_cut & ~must).sum())}")
    assert equal[must].all(), np.flatnonzero(must & ~equal)[:10]
    # the rays that had ended before the cut are the uninterrupted trace's already
    assert parity.same_records(got[~was_cut], want[~was_cut])


# ---- (3) the sine / cosine fix-up gives the same values -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sincos_arguments():
    """~2e5 arguments, built from exact operations only (the same bits under any numpy): the dyadic grid k / 8192 over [-12, 12] -- every quadrant, both
    signs, +-0 -- and, round each multiple m pi/2 (|m| <= 7) as the routine's own reduction sees it, the 64 doubles on either side, then offsets of
    2^-10 ... 2^-50 either way."""
    grid = np.arange(-98304, 98305, dtype=np.float64) / 8192.0
    near = [np.array([-0.0])]
    for m in range(-7, 8):
        base = np.float64(m) * np.float64(1.5707963267948966)
        bits = np.array([base]).view(np.int64)[0]
        if m != 0:
            near.append((bits + np.arange(-64, 65, dtype=np.int64)).view(np.float64))
        off = 2.0 ** -np.arange(10, 51, dtype=np.float64)
        near.append(base + off)
        near.append(base - off)
    x = np.concatenate([grid] + near)
    x.setflags(write=False)
    return x


def sincos_digest(x, s, c):
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).view(np.uint64).tobytes()).hexdigest()
    return {"n": int(len(x)), "arguments": sha(x), "sin": sha(s), "cos": sha(c)}


def test_fast_sincos_values_are_those_of_the_old_fix_up(krlib):
    x = sincos_arguments()
    assert 1.9e5 < len(x) < 2.1e5
    s, c = probe(15, x), probe(16, x)
    # every quadrant, on both sides of zero
    quadrant = np.rint(x * (2 / np.pi)).astype(np.int64)
    assert {(int(q) & 3, bool(neg)) for q, neg in zip(quadrant[::97], (x < 0)[::97])} >= {(q, neg) for q in range(4) for neg in (False, True)}
    # the strict routine (correctly rounded in practice): the exact sign everywhere, and the fast routine's 2 ulp -- plus, for the arguments next to a
    # multiple of pi/2, what its two-piece pi/2 leaves of the reduced argument: |n| <= 8 times half an ulp of the second piece, 8 x 2^-54 x 6.2e-17 < 3e-32
    want_s, want_c = probe(4, x), probe(5, x)
    assert np.array_equal(np.signbit(s), np.signbit(want_s)) and np.array_equal(np.signbit(c), np.signbit(want_c))
    for got, want, name in ((s, want_s, "sin"), (c, want_c, "cos")):
        err = np.abs(got - want)
        worst = float((err / np.spacing(np.abs(want))).max())
        print(f"fast {name}: {worst:.3f} ulp from the strict routine at worst over {len(x)} arguments")
        assert (err <= 2.0 * np.spacing(np.abs(want)) + 3e-32).all(), (name, worst)
    # and bit for bit what the library before the change gave
    want = json.load(open(DIGEST_FILE))
    got = sincos_digest(x, s, c)
    assert got["arguments"] == want["arguments"] and got["n"] == want["n"], "the arguments are not the ones the digest was taken over"
    assert got == want
