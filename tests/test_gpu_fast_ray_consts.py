"""GPU: the fast Euler / RK4 kernels keep a ray's constant terms (kr_fast.hpp::FastRayConsts: a k, a h, a^2 k, h^2, (a k)^2, Q + (h - a k)^2) beside the
lane state, filled where a lane takes the ray (kr_trace.hip::trace_body) instead of once per step.

What that can get wrong is STALE terms: a lane that takes a second ray and still steps with the first ray's.  It needs a lane that refills, i.e. a launch
with more rays than resident lanes: a lamp post at h = 10, a = 0.998 on a 317 x 317 grid (~1e5 rays) with KR_FLAG_BLOCKS_PER_CU(1) -- one wave per
SIMD, 65 536 lanes on 256 compute units.  A ray's record must then not depend on which lane had which ray before it: (a) the trace of a permuted copy
equals the trace, record for record and bit for bit; (b) the merged batch (trace_multi_kernel, which goes through the same trace_body) equals the single
trace; (c) the first claim alone -- a 5040-ray grid, no refills -- against the oracle under tests/parity.py's bars, nothing wider.

The fast RK45 kernels do not carry the terms (their stages form them per evaluation, as before) and are not part of this file."""
import functools
import math

import numpy as np
import pytest

import parity
import step_control_cases as sc
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

ONE_WAVE_PER_SIMD = 1 << 8          # KR_FLAG_BLOCKS_PER_CU(1), include/kr_trace.h
RESIDENT_LANES = 65536              # 256 compute units x 4 SIMDs x 1 wave x 64 lanes
MODES = [pytest.param(capi.FLAG_FAST_MATH, id="fastmath"), pytest.param(capi.FLAG_HYBRID, id="hybrid")]
MODE_NAME = {capi.FLAG_FAST_MATH: "fastmath", capi.FLAG_HYBRID: "hybrid"}
METHODS = [pytest.param(capi.EULER, id="euler"), pytest.param(capi.RK4, id="rk4")]
METHOD_NAME = {capi.EULER: "euler", capi.RK4: "rk4"}


def refill_grid():
    d = 1.99 / 316
    return sc.lamp(spin=0.998, h=10.0, d=d, dbeta=d * math.pi / 0.995)


def parity_grid():
    return sc.lamp(spin=0.998, h=10.0)          # 0.05 x 0.05: 5040 live rays


def params(integrator, flags, grid):
    return sc.grid_params(sc.DEFAULT, integrator, grid, flags=flags | ONE_WAVE_PER_SIMD)


@functools.lru_cache(maxsize=None)
def single_trace(integrator, flags):
    """The refill grid traced in emission order: computed once per (integrator, mode), read-only."""
    grid = refill_grid()
    out, st = api.trace(params(integrator, flags, grid), sc.init(grid))
    out.setflags(write=False)
    return out, st


def orders(n):
    return {"shuffled": np.random.default_rng(20240607).permutation(n), "reversed": np.arange(n)[::-1]}


def test_the_grid_forces_refills(krlib):
    rays = sc.init(refill_grid())
    live = int((rays["steps"] != -1).sum())
    assert api.device_info()["cu_count"] * 4 * 64 <= RESIDENT_LANES
    assert len(rays) >= live > RESIDENT_LANES + RESIDENT_LANES // 2


@pytest.mark.parametrize("order", ["shuffled", "reversed"])
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_a_record_does_not_depend_on_the_lane_history(krlib, integrator, flags, order):
    """(a) The buffer and a copy whose records were permuted BEFORE the trace: after undoing the permutation every record is bit-identical."""
    grid = refill_grid()
    rays = sc.init(grid)
    want, st_want = single_trace(integrator, flags)
    perm = orders(len(rays))[order]
    got, st = api.trace(params(integrator, flags, grid), np.ascontiguousarray(rays[perm]))
    assert st["rays_traced"] == st_want["rays_traced"] > RESIDENT_LANES
    assert st["steps_total"] == st_want["steps_total"] == sc.steps_total(want)
    assert parity.same_records(got, want[perm])
    if flags & capi.FLAG_HYBRID:
        assert st["rays_strict_side"] == st_want["rays_strict_side"] > 0


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_merged_batch_equals_the_single_trace(krlib, integrator, flags):
    """(b) One kr_trace_batch_async_f64 batch of two traces -- the rays, and the rays in reverse order -- against the single trace.  With KR_FLAG_HYBRID the
    batch is merged (one trace_multi_kernel main launch over both); KR_FLAG_FAST_MATH traces are not mergeable and run as two launches of a batch."""
    grid = refill_grid()
    rays = sc.init(grid)
    want, st_want = single_trace(integrator, flags)
    inputs = [np.ascontiguousarray(rays), np.ascontiguousarray(rays[::-1])]
    p = params(integrator, flags, grid)
    with DeviceScope(krlib) as dev:
        bufs = [dev.upload(h) for h in inputs]
        stats = [api.trace_wait(t) for t in api.trace_batch_async([p, p], [d.value for d in bufs], [len(h) for h in inputs])]
        outs = [dev.fetch(d, len(h), h.dtype) for d, h in zip(bufs, inputs)]
    for st in stats:
        assert st["rays_traced"] == st_want["rays_traced"] and st["steps_total"] == st_want["steps_total"]
    assert parity.same_records(outs[0], want)
    assert parity.same_records(outs[1], want[::-1])


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", METHODS)
def test_first_claim_against_the_oracle(krlib, integrator, flags):
    """(c) 5040 rays: every lane takes one ray.  Per-ray parity at parity.rtol_for / steps_slack_for under 1 % + 3 x the oracle's own 1-ulp envelope (capped
    at 5 %), the fast arithmetic without the knife-edge column -- test_gpu_step_control.test_trace_vs_oracle's bars; the oracle alone stays inside them."""
    grid = parity_grid()
    init, want = sc.init(grid), sc.oracle_run(sc.DEFAULT, integrator, grid)
    p = params(integrator, flags, grid)
    out, st = api.trace(p, init)
    rtol, slack = parity.rtol_for(p), parity.steps_slack_for(p, flags)
    envelope = sc.envelope(sc.DEFAULT, integrator, grid)
    n_live = 5040
    if flags & capi.FLAG_FAST_MATH:
        ke = parity.knife_edge_mask(init, False)
        n_live -= int((ke & (init["steps"] != -1)).sum())
        res = parity.compare_rays(parity.drop_rays(out, ke), parity.drop_rays(want, ke), rtol=rtol, steps_slack=slack)
    else:
        res = parity.compare_rays(out, want, rtol=rtol, steps_slack=slack)
    allowed = parity.allowed_bad_frac(p, init, rtol, envelope=envelope)
    case = f"h10-{METHOD_NAME[integrator]}-{MODE_NAME[flags]}"
    parity.record_margin("test_first_claim_against_the_oracle", case, res, allowed, envelope, steps_total=st["steps_total"])
    print(f"fast ray consts {case}: bad {res['n_bad']} / {res['n_traced']} (allowed {allowed:.4f}, envelope {envelope:.4f}), worst accepted {res['worst_ok']:.3e}")
    assert envelope <= allowed
    assert res["n_traced"] == n_live
    assert res["frac_bad"] <= allowed, res
    assert st["rays_traced"] == 5040 and st["steps_total"] == sc.steps_total(out)
