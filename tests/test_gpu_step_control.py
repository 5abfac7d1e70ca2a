"""GPU: the trace kernels away from the default step-control parameters (tests/step_control_cases.py has the regimes and what each reaches).

Every kernel reads precision, theta_precision, max_tstep, maxtstep_rlim, max_phistep and horizon through launch constants that kr_ray_io.hpp::make_consts
derives from kr_params -- host-made reciprocals and the switch to IEEE division when one does not qualify, -inf / +inf for a cap that is off, the words
of max_tstep for the fast path's select -- and the step heuristic that uses them exists in five hand-written copies (kr_device.hpp::step_fixed fast
and strict, step_radial, kr_rk45.hpp's first step and outer cap).  The oracle these tests trust is held to the compiled reference in the same
regimes, bit for bit, by tests/test_oracle_vs_ref.py.  Bars are tests/parity.py's own; nothing here introduces a tolerance."""
import ctypes as C
import math

import numpy as np
import pytest

import golden_cases as gc
import oracle_lib as ol
import parity
import radial_cases as rc
import step_control_cases as sc
from raytrace_cpu_amd import api, capi
from test_gpu_radial import check_three_ways

pytestmark = pytest.mark.gpu

MODES = [pytest.param(0, id="strict"), pytest.param(capi.FLAG_HYBRID, id="hybrid"), pytest.param(capi.FLAG_FAST_MATH, id="fastmath")]
MODE_NAME = {0: "strict", capi.FLAG_HYBRID: "hybrid", capi.FLAG_FAST_MATH: "fastmath"}
REGIMES = [pytest.param(r, id=r) for r in sc.NAMES]
ALL_METHODS = [pytest.param(m, id=n) for n, m in sc.INTEGRATORS.items()]
FIXED_STEP = [pytest.param(capi.RK4, id="rk4"), pytest.param(capi.EULER, id="euler")]
METHOD_NAME = {m: n for n, m in sc.INTEGRATORS.items()}
BIT_IDENTICAL_FLOOR = 0.99          # test_trace_vs_golden's bar for strict Euler / RK4 from a PointSource


# ---- (a) per-ray parity, (b) bit-identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("integrator", ALL_METHODS)
@pytest.mark.parametrize("regime", REGIMES)
def test_trace_vs_oracle(krlib, regime, integrator, flags):
    """Written like test_gpu_parity.test_trace_vs_golden, on the 5040-ray lamp post at h = 5: per-ray parity at rtol_for / steps_slack_for; the strict
    fixed-step runs under allowed_bad_frac_strict, every other run under 1 % + 3 x the oracle's own 1-ulp envelope for this regime; the fast arithmetic
    without the knife-edge column.  The kernel's step counters must agree with the records it wrote.

    Bit-identity of the strict fixed-step runs: the share of rays that carry the oracle's bits in every output is recorded for every regime and held to
    the point-source floor (0.99) where the regime takes no more steps on this grid than the default parameters do -- a condition computed from the
    oracle alone.  More steps are more sin / cos calls at which glibc itself is not correctly rounded, so for the other regimes the share is a
    measurement (profiles/step_control_parity_margins.json) and no floor is fixed in advance."""
    grid = sc.lamp()
    init = sc.init(grid)
    want = sc.oracle_run(regime, integrator, grid)
    p = sc.grid_params(regime, integrator, grid)
    out, st = api.trace(capi.copy_params(p, flags=flags), init)
    rtol, slack = parity.rtol_for(p), parity.steps_slack_for(p, flags)
    envelope = sc.envelope(regime, integrator, grid)
    strict_fixed = flags == 0 and integrator != capi.RK45
    case = f"{regime}-{METHOD_NAME[integrator]}-{MODE_NAME[flags]}"
    if flags & capi.FLAG_FAST_MATH:
        ke = parity.knife_edge_mask(init, False)
        res = parity.compare_rays(parity.drop_rays(out, ke), parity.drop_rays(want, ke), rtol=rtol, steps_slack=slack)
    else:
        res = parity.compare_rays(out, want, rtol=rtol, steps_slack=slack)
    allowed = parity.allowed_bad_frac_strict(p, res["n_traced"]) if strict_fixed else parity.allowed_bad_frac(p, init, rtol, envelope=envelope)
    steps_oracle, steps_default = sc.steps_total(want), sc.steps_total(sc.oracle_run(sc.DEFAULT, integrator, grid))
    floor_applies = strict_fixed and steps_oracle <= steps_default
    parity.record_margin("test_trace_vs_oracle", case, res, allowed, envelope, steps_total_oracle=steps_oracle, steps_total_oracle_default_regime=steps_default,
                         bit_identical_floor=BIT_IDENTICAL_FLOOR if floor_applies else None, steps_total=st["steps_total"])
    print(f"step control {case}: bad {res['n_bad']} / {res['n_traced']} (allowed {allowed:.4f}, envelope {envelope:.4f}), bit-identical {res['frac_bit_identical']:.4f}, "
          f"worst accepted {res['worst_ok']:.3e}, steps {st['steps_total']} (oracle {steps_oracle}, default regime {steps_default})")
    assert res["n_traced"] == (5040 if not flags & capi.FLAG_FAST_MATH else 5040 - int((ke & (init["steps"] != -1)).sum()))
    assert res["frac_bad"] <= allowed, res
    # the kernel's own counters agree with the records it wrote (every ray starts at steps = 0)
    assert st["steps_total"] == sc.steps_total(out)
    assert st["longest_ray_steps"] == sc.longest(out)
    assert st["rays_traced"] == 5040
    if floor_applies:
        assert res["frac_bit_identical"] >= BIT_IDENTICAL_FLOOR, res["frac_bit_identical"]


# ---- (c) a ray-destination run -----------------------------------------------------------------------------------------------------------------------
def _isco_case(regime, integrator):
    grid = sc.lamp(spin=0.5, h=5.0)
    return grid, sc.grid_params(regime, integrator, grid, stop_kind=capi.STOP_DISC_ISCO, stop_params=(gc.r_isco(0.5), 400.0, math.pi / 2))


@pytest.mark.parametrize("regime", ["coarse", "tight_caps"])
def test_destination_run_reproduces_every_integer_outcome(krlib, regime):
    """run_raytrace(DiscWithISCO) from a lamp post at a = 0.5, where rays whirl inside the ISCO and the reference's outcome is decided at the 1-ulp level,
    on the strict arithmetic the class mirror uses for it: the integer outcome and the step count of every ray are the reference's."""
    grid, p = _isco_case(regime, capi.RK4)
    init = sc.init(grid)
    want, _ = ol.oracle_trace(p, init)
    out, st = api.trace(capi.copy_params(p, flags=0), init)
    res = parity.compare_rays(out, want, rtol=parity.rtol_for(p), steps_slack=parity.steps_slack_for(p))
    allowed = parity.allowed_bad_frac_strict(p, res["n_traced"])
    parity.record_margin("test_destination_run_reproduces_every_integer_outcome", f"{regime}-rk4_isco-strict", res, allowed)
    assert res["n_traced"] == 5040 and (want["status"] & capi.STATUS_DEST).sum() > 1000
    assert res["n_int_fields_differ"] == 0 and res["n_steps_differ"] == 0, res
    assert res["frac_bad"] <= allowed, res
    assert st["steps_total"] == sc.steps_total(out)


@pytest.mark.parametrize("regime", ["coarse", "tight_caps"])
def test_destination_run_has_no_euler_form(krlib, regime):
    """The reference's Euler integrator has no RayDestination overload (it asserts, raytracer.cpp:983): off the defaults too, the oracle and the
    library both refuse the combination instead of tracing something."""
    grid, p = _isco_case(regime, capi.EULER)
    rays = sc.init(grid).copy()
    assert ol.oracle().kro_trace_f64(C.byref(p), ol.ptr(rays), len(rays), 1, None) == capi.KR_EINVAL
    assert krlib.kr_trace_f64(C.byref(p), ol.ptr(rays), len(rays), None) == capi.KR_EINVAL
    assert b"Euler does not support RayDestination" in krlib.kr_last_error()
    assert parity.same_records(rays, sc.init(grid))


# ---- (d) radial waves --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", FIXED_STEP)
@pytest.mark.parametrize("regime", REGIMES)
def test_radial_waves(krlib, regime, integrator):
    """kr_device.hpp::step_radial carries its own copy of the step heuristic.  On tests/radial_cases.py's 200 x 3 grid, under every regime: the hybrid
    trace with radial waves == the same without them == the single strict launch, field for field (test_gpu_radial.check_three_ways); the flagged
    column's integer fields and step counts, and the side launch's counters, are the oracle's.  The oracle holds exactly 93 of the 199 flagged rays at
    their theta in every regime (no NaN, no step-limit ray), so the radial step is never vacuously skipped."""
    p, rays = rc.params(integrator, **sc.overrides(regime)), rc.init()
    cpu, _ = ol.oracle_trace(p, rays)
    column, held = rc.flagged(rays), rc.held(rays, cpu)
    assert column.sum() == 199 and held.sum() == 93
    assert not np.isnan(cpu["r"][column]).any() and not (cpu["steps"] < -1).any()
    got, st = check_three_ways(p, rays, column)
    for f in parity.INT_FIELDS + ("steps",):
        assert np.array_equal(got[f][column], cpu[f][column]), f
    steps = np.abs(cpu["steps"].astype(np.int64))
    assert st["rays_strict_side"] == 199
    assert st["steps_strict_side"] == int(steps[column].sum())
    assert st["longest_ray_steps_strict_side"] == int(steps[column].max())
    # the rays the oracle holds at theta_0 are held here, with the oracle's signed zero for a polar velocity
    assert np.array_equal(got["theta"][held].view(np.uint64), rays["theta"][held].view(np.uint64))
    assert np.array_equal(got["ptheta"][held].view(np.uint64), cpu["ptheta"][held].view(np.uint64))


# ---- (e) RK45 at a boundary --------------------------------------------------------------------------------------------------------------------------
EXTRAPOLATION_RTOL = 1e-11          # include/kr_trace.h, kr_stats.rk45_extrapolated_steps: "t, phi, momenta to ~1e-11"


def test_rk45_creep_above_a_boundary(krlib):
    """RK45 rays that cannot pass set_boundary(3.0) creep above r = 3 to the step limit, as captured rays do above the event horizon -- which is what the
    fixed-point replay and the extrapolation of kr_rk45.hpp were reasoned for.  The default (extrapolating) strict trace against the same trace with
    KR_FLAG_RK45_ITERATE_ALL: every record that did not reach the step limit is identical; one that did has the same r, theta, step count and integer
    fields, and t and phi within the figure include/kr_trace.h documents for extrapolated steps."""
    grid = sc.lamp()
    init, want = sc.init(grid), sc.oracle_run("boundary", capi.RK45, grid)
    p = sc.grid_params("boundary", capi.RK45, grid)
    fast, st = api.trace(capi.copy_params(p, flags=0), init)
    slow, st_slow = api.trace(capi.copy_params(p, flags=capi.FLAG_RK45_ITERATE_ALL), init)
    cut = want["steps"] < -1
    assert cut.sum() == 875
    assert ((fast["steps"] < -1).sum(), (slow["steps"] < -1).sum()) == (875, 875)
    cut = slow["steps"] < -1
    assert np.array_equal(fast["steps"], slow["steps"]) and (slow["steps"][cut] == -capi.RK45_STEPLIM).all()
    assert parity.same_records(fast[~cut], slow[~cut])
    for f in ("r", "theta"):
        assert np.array_equal(fast[f].view(np.uint64), slow[f].view(np.uint64)), f
    for f in parity.INT_FIELDS:
        assert np.array_equal(fast[f], slow[f]), f
    worst = {}
    for f in ("t", "phi", "pt", "pr", "ptheta", "pphi"):
        g, w = fast[f][cut], slow[f][cut]
        assert f not in ("t", "phi") or np.isfinite(g).all() and np.isfinite(w).all(), f
        with np.errstate(invalid="ignore"):
            worst[f] = float(np.nanmax(np.where(g == w, 0.0, np.abs(g - w) / np.maximum(np.abs(w), 1.0))))
    res = parity.compare_rays(fast, slow, rtol=EXTRAPOLATION_RTOL, steps_slack=0)
    parity.record_margin("test_rk45_creep_above_a_boundary", "boundary-rk45-strict-extrapolated_vs_iterated", res, None, step_limit_rays=875,
                         rk45_extrapolated_steps=st["rk45_extrapolated_steps"], rk45_stationary_steps=st["rk45_stationary_steps"],
                         rk45_extrapolated_steps_iterate_all=st_slow["rk45_extrapolated_steps"], **{f"worst_rel_{f}_step_limit_rays": v for f, v in worst.items()})
    print(f"rk45 at boundary 3.0: step-limit rays 875, extrapolated steps {st['rk45_extrapolated_steps']}, stationary (replayed) steps {st['rk45_stationary_steps']}, "
          f"worst relative difference on the step-limit rays {worst}")
    assert st_slow["rk45_extrapolated_steps"] == 0
    assert worst["t"] <= EXTRAPOLATION_RTOL and worst["phi"] <= EXTRAPOLATION_RTOL, worst
    assert st["steps_total"] == st_slow["steps_total"] == sc.steps_total(slow)


# ---- (f) integer outcomes at scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["caps_off", "tight_caps"])
def test_integer_outcomes_at_scale(krlib, regime):
    """One reduced sweep in the style of tests/test_gpu_geometry_sweep.py: a lamp post at h = 3, a = 0.998 on 520 x 520 rays (>= 2^18, so the flags = 0
    launch splits off a strict side launch too), RK4.  status, steps, rdot_flips and equatorial_crossings of every ray are the oracle's: no differing
    ray on the strict arithmetic, at most 2 on the hybrid (the existing sweep's allowance)."""
    d = 1.99 / 519
    grid = sc.lamp(spin=0.998, h=3.0, d=d, dbeta=d * math.pi / 0.995)
    init, want = sc.init(grid), sc.oracle_run(regime, capi.RK4, grid)
    p = sc.grid_params(regime, capi.RK4, grid)
    valid = want["steps"] != -1
    assert valid.sum() >= 2 ** 18
    for flags, mode, allowed in ((capi.FLAG_HYBRID, "hybrid", 2), (0, "strict", 0)):
        got, st = api.trace(capi.copy_params(p, flags=flags), init)
        differ = np.zeros(len(init), dtype=bool)
        for k in ("status", "steps", "rdot_flips", "equatorial_crossings"):
            differ |= got[k] != want[k]
        n_bad = int((valid & differ).sum())
        print(f"step control sweep {regime} {mode}: {n_bad} of {int(valid.sum())} rays with another integer outcome, rays on the strict side {st['rays_strict_side']}")
        assert st["rays_strict_side"] > 0
        assert n_bad <= allowed, (regime, mode, n_bad, np.flatnonzero(valid & differ)[:10].tolist())
        assert st["steps_total"] == sc.steps_total(got)
