"""GPU: the radial waves of the strict side launch (kr_device.hpp::step_radial, kr_trace.hip::trace_side_kernel).

A flagged ray whose polar numerator is exactly zero never leaves its theta; the side launch integrates it with a radial-only step.  That changes
which instructions run, never what is computed: every record must equal, field for field (parity.same_records), what the general strict step gives --
the same trace with KR_NO_RADIAL=1 (all flagged rays on the general waves) and the single strict launch (KR_NO_ISOLATE=1, flags = 0)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import bench
import golden_cases as gc
import parity
import radial_cases as rc
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

METHODS = [pytest.param(capi.RK4, id="rk4"), pytest.param(capi.EULER, id="euler")]
same = parity.same_records


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def hybrid(p, rays):
    return api.trace(capi.copy_params(p, flags=capi.FLAG_HYBRID), rays)


def hybrid_general(p, rays):
    """The same trace with every flagged ray on the general waves."""
    with env(KR_NO_RADIAL="1"):
        return hybrid(p, rays)


def single_strict(p, rays):
    with env(KR_NO_ISOLATE="1"):
        out, st = api.trace(capi.copy_params(p, flags=0), rays)
    assert st["rays_strict_side"] == 0
    return out, st


@functools.lru_cache(maxsize=None)
def reference(integrator):
    """The test grid through the single strict launch and through the hybrid trace without radial waves: computed once, shared, read-only."""
    p, rays = rc.params(integrator), rc.init()
    want, _ = single_strict(p, rays)
    general, st = hybrid_general(p, rays)
    want.setflags(write=False)
    general.setflags(write=False)
    return want, general, st


def check_three_ways(p, rays, column):
    """hybrid with radial waves == hybrid without them (every ray, and the counters); flagged rays == the single strict launch.  Returns the records."""
    got, st = hybrid(p, rays)
    general, st_general = hybrid_general(p, rays)
    want, _ = single_strict(p, rays)
    assert st["rays_strict_side"] == st_general["rays_strict_side"] >= int(column.sum()) > 0
    for k in ("rays_traced", "steps_total", "steps_strict_side", "longest_ray_steps_strict_side", "longest_ray_steps"):
        assert st[k] == st_general[k], k
    assert same(got, general)
    assert same(got[column], want[column])
    return got, st


@pytest.mark.parametrize("integrator", METHODS)
def test_hybrid_and_strict_split_equal_the_single_strict_launch(krlib, integrator):
    p, rays = rc.params(integrator), rc.init()
    column = rc.flagged(rays)
    want, general, st_general = reference(integrator)
    got, st = hybrid(p, rays)
    assert st["rays_strict_side"] == int(column.sum())
    assert same(got[column], want[column])
    assert same(got, general)
    # the counters keep meaning "all flagged rays", radial or not
    steps = np.abs(want["steps"].astype(np.int64))
    assert st["steps_strict_side"] == st_general["steps_strict_side"] == int(steps[column].sum())
    assert st["longest_ray_steps_strict_side"] == st_general["longest_ray_steps_strict_side"] == int(steps[column].max())
    assert st["steps_total"] == st_general["steps_total"]
    # the all-strict trace with a side launch (flags = 0): traces of a batch split from 4096 rays on, so the grid goes in seven times over
    tiled = np.tile(rays, 7)
    with DeviceScope(krlib) as dev:
        d = dev.upload(tiled)
        st_split = api.trace_wait(api.trace_batch_async([capi.copy_params(p, flags=0)], [d.value], [len(tiled)])[0])
        out = dev.fetch(d, len(tiled), tiled.dtype)
    assert st_split["rays_strict_side"] == 7 * int(column.sum())
    assert st_split["steps_strict_side"] == 7 * int(steps[column].sum()) and st_split["steps_total"] == 7 * int(steps[rays["steps"] >= 0].sum())
    assert same(out, np.tile(want, 7))


@pytest.mark.parametrize("integrator", METHODS)
def test_integer_fields_and_step_totals_equal_the_oracle(krlib, integrator):
    rays, cpu = rc.init(), rc.oracle(integrator)
    column, held = rc.flagged(rays), rc.held(rays, rc.oracle(integrator))
    got, st = hybrid(rc.params(integrator), rays)
    for f in parity.INT_FIELDS + ("steps",):
        assert np.array_equal(got[f][column], cpu[f][column]), f
    steps = np.abs(cpu["steps"].astype(np.int64))
    assert st["steps_strict_side"] == int(steps[column].sum()) and st["longest_ray_steps_strict_side"] == int(steps[column].max())
    # the rays the oracle holds at theta_0 are held here, with the oracle's signed zero for a polar velocity
    assert np.array_equal(got["theta"][held].view(np.uint64), rays["theta"][held].view(np.uint64))
    assert np.array_equal(got["ptheta"][held].view(np.uint64), cpu["ptheta"][held].view(np.uint64))


@pytest.mark.parametrize("integrator", METHODS)
def test_step_limit_and_resume(krlib, integrator):
    """1000 steps, then the rest: a ray taken up again mid-flight is radial on the strength of the state it is stored in."""
    rays = rc.init()
    column = rc.flagged(rays)
    first, rest = rc.params(integrator, steplim=1000), rc.params(integrator)

    def two_calls(trace):
        a, st_a = trace(first, rays)
        cut = (a["status"] & capi.STATUS_STEPLIM) != 0
        assert (a["steps"][cut] == -1000).all()
        b = a.copy()
        b["steps"][cut] = 1000                               # what a caller does to go on: the ray counts as unfinished again
        b["status"][cut] &= ~capi.STATUS_STEPLIM
        c, st_c = trace(rest, b)
        return a, c, cut, (st_a, st_c)

    a, c, cut, sts = two_calls(hybrid)
    a_g, c_g, _, sts_g = two_calls(hybrid_general)
    a_s, c_s, _, _ = two_calls(single_strict)
    held = rc.held(rays, rc.oracle(integrator))
    assert (cut & held).sum() >= 50                          # the long rays are the radial ones
    assert same(a, a_g) and same(c, c_g)
    assert same(a[column], a_s[column]) and same(c[column], c_s[column])
    for st, st_g in zip(sts, sts_g):
        for k in ("steps_total", "steps_strict_side", "longest_ray_steps_strict_side"):
            assert st[k] == st_g[k], k
    assert not (c["status"][column] & capi.STATUS_STEPLIM).any()
    assert np.array_equal(c["theta"][held].view(np.uint64), rays["theta"][held].view(np.uint64))


@pytest.mark.parametrize("integrator", METHODS)
def test_one_ulp_off_in_Q_is_not_radial_and_equals_the_general_path(krlib, integrator):
    rays = rc.init()
    held = rc.held(rays, rc.oracle(integrator))
    rays["Q"][held] = np.nextafter(rays["Q"][held], np.inf)
    check_three_ways(rc.params(integrator), rays, rc.flagged(rays))
    rays["Q"][held] = np.nextafter(np.nextafter(rays["Q"][held], -np.inf), -np.inf)          # ... and one ulp below
    check_three_ways(rc.params(integrator), rays, rc.flagged(rays))


@pytest.mark.parametrize("integrator", METHODS)
def test_rays_that_start_off_the_healthy_range(krlib, integrator):
    """Radial constants with a radius that is not a number, on r_max (no step at all), infinite, and on the horizon (Delta = 0: the first
    evaluation divides by zero): whatever the general path makes of them."""
    rays = rc.init()
    p = rc.params(integrator)
    pick = np.flatnonzero(rc.held(rays, rc.oracle(integrator)))[[3, 20, 40, 60, 80]]
    rays["r"][pick] = [np.nan, p.r_max, np.inf, p.horizon, np.nextafter(p.horizon, np.inf)]
    got, _ = check_three_ways(p, rays, rc.flagged(rays))
    assert np.isnan(got["r"][pick[0]]) and got["steps"][pick[1]] == 0 and got["status"][pick[1]] & capi.STATUS_RLIM


OTHER_SHAPES = [("ps_h10_a0_landing", "rk4"), ("ps_h10_a0_landing", "euler"), ("ip16", "rk4"), ("ip16", "euler")]


@pytest.mark.parametrize("case,run", OTHER_SHAPES, ids=[f"{c}-{r}" for c, r in OTHER_SHAPES])
def test_shapes_with_few_or_no_radial_rays(krlib, case, run):
    """A Schwarzschild lamp post (a = 0) and an image plane far off the axis (with its NaN pixel): the flagged rays move in theta."""
    spec = gc.cases()[case]
    rays = np.load(gc.golden_path(case))["init"]
    column = parity.knife_edge_mask(rays, gc.is_imageplane(spec)) & (rays["steps"] >= 0)
    nan = np.isnan(rays["h"]) & (rays["steps"] >= 0)
    check_three_ways(spec["runs"][run], rays, column | nan)
