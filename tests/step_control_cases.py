"""The step-control regimes (TEST INFRASTRUCTURE; shared by tests/test_oracle_vs_ref.py and tests/test_gpu_step_control.py).

Every trace kernel reads six step-control inputs from kr_params: precision, theta_precision, max_tstep, maxtstep_rlim, max_phistep and horizon (the
set_boundary() radius).  Each regime below is a dict of kr_params overrides that moves some of them off the constructor defaults
(100, 50, 1, 100, 0.1, kerr_horizon(a)) to where the kernels' launch constants (kr_ray_io.hpp::make_consts) take another value or another path:

  coarse      reciprocals that are not powers of ten; long steps
  fine        ~6 x the steps per ray
  allones     both divisors have an all-ones significand: inv_ok == false, the IEEE-division fallback of div_by_uniform
  caps_off    tstep_rlim_eff = -inf, phistep_eff = +inf, the "off" high word of the fast path's time cap on every step
  tight_caps  a non-zero low word of max_tstep; rays cross maxtstep_rlim mid-flight; the azimuth cap binds on most steps
  boundary    set_boundary(3.0): RK45 rays creep above r = 3 instead of above the Kerr horizon
  time_cap    the time cap binds on most steps inside maxtstep_rlim = 50, which rays cross mid-flight.  (Under tight_caps the azimuth cap is always the
              tighter one for Euler / RK4: the oracle's records there are bit for bit those of max_tstep = 1.  Here max_tstep decides the step, down to
              its low word: with that word zeroed -- 0.03 (1 - 4.6e-7) -- 44-70 % of the oracle's rays move by more than the parity band.)

Grids are small named tuples (hashable: the oracle's trace and its 1-ulp noise envelope are computed once per (regime, integrator, grid) and shared)."""
import collections
import functools

import numpy as np

import oracle_lib as ol
import parity
from raytrace_cpu_amd import capi

REGIMES = {
    "coarse": dict(precision=7.0, theta_precision=3.0),
    "fine": dict(precision=1000.0, theta_precision=400.0),
    "allones": dict(precision=float(np.nextafter(128.0, 0.0)), theta_precision=float(np.nextafter(64.0, 0.0))),
    "caps_off": dict(max_tstep=-1.0, max_phistep=0.0),
    "tight_caps": dict(max_tstep=0.3, maxtstep_rlim=20.0, max_phistep=0.01),
    "boundary": dict(horizon=3.0),
    "time_cap": dict(max_tstep=0.03, maxtstep_rlim=50.0),
}
DEFAULT = "default"            # the constructor's values: the yardstick of "more steps than the default regime"
NAMES = list(REGIMES)
INTEGRATORS = {"euler": capi.EULER, "rk4": capi.RK4, "rk45": capi.RK45}

# kind "lamp": a lamp post on the axis (theta_0 = 1e-3) at height h, full angular range, spacing d in cos(alpha) and dbeta in beta
# kind "plane": an n x n image plane at 80 degrees, 10 000 r_g away
Grid = collections.namedtuple("Grid", "kind spin h d dbeta")


def lamp(spin=0.998, h=5.0, d=0.05, dbeta=None):
    """The point-source grid of the reference's integrator_perf_test (h = 5, a = 0.998, 0.05 x 0.05: 5040 live rays), emitted energy set, r_max 1000."""
    return Grid("lamp", float(spin), float(h), float(d), float(d if dbeta is None else dbeta))


def plane33():
    """The 33 x 33 image plane of test_oracle_vs_ref._imageplane_case (trace spin -a: rays run backwards from the observer), r_max 11000."""
    return Grid("plane", 0.998, 0.0, 60.0 / 32, 60.0 / 32)


def source_spec(grid, precision=100.0):
    """The source's constructor arguments; `precision` is the constructor's tol / precision, the only way the reference takes it."""
    if grid.kind == "lamp":
        return ol.pointsource_spec([0.0, grid.h, 1e-3, 0.0], 0.0, grid.spin, grid.d, grid.dbeta, cosalpha0=-0.995, cosalphamax=0.995, beta0=-np.pi,
                                   betamax=np.pi, tol=precision)
    return ol.imageplane_spec(10000.0, 80.0, -30.0, 30.0, grid.d, -30.0, 30.0, grid.dbeta, grid.spin, precision=precision)


def trace_spin(grid):
    return grid.spin if grid.kind == "lamp" else -grid.spin


def redshift_start_args(grid):
    """(V, reverse, projradius) of the redshift_start call that precedes the trace."""
    return (0.0, 0, 0) if grid.kind == "lamp" else (0.0, 1, 0)


def overrides(regime):
    return {} if regime == DEFAULT else REGIMES[regime]


def params(regime, integrator, spin, **kw):
    """kr_params of `regime` (a name of REGIMES, or DEFAULT); kw: further fields (r_max, stop_kind, stop_params, flags, ...), applied last."""
    p = capi.default_params(spin)
    p.integrator, p.r_max = integrator, 1000.0
    return capi.copy_params(p, **dict(overrides(regime), **kw))


def grid_params(regime, integrator, grid, **kw):
    if grid.kind == "plane":
        kw.setdefault("r_max", 11000.0)
    return params(regime, integrator, trace_spin(grid), **kw)


@functools.lru_cache(maxsize=None)
def _init(grid):
    spec = source_spec(grid)
    rays = ol.oracle_pointsource(spec) if grid.kind == "lamp" else ol.oracle_imageplane(spec)
    ol.oracle().kro_redshift_start_f64(trace_spin(grid), *redshift_start_args(grid), ol.ptr(rays), len(rays))
    rays.setflags(write=False)
    return rays


def init(grid):
    """The rays as the source emits them (the precision is no input of the constructor's records), read-only; computed once per grid."""
    return _init(grid)


@functools.lru_cache(maxsize=None)
def oracle_run(regime, integrator, grid):
    """The CPU oracle's trace of init(grid) under `regime`: computed once per process, read-only."""
    out, _ = ol.oracle_trace(grid_params(regime, integrator, grid), _init(grid))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def envelope(regime, integrator, grid):
    """parity.noise_envelope_frac of this case -- the share of rays that move by more than rtol, or change an integer output, when Q is perturbed by one
    ulp on the oracle -- with oracle_run as its base trace, so that the three arithmetic modes of one case share one CPU computation."""
    p = grid_params(regime, integrator, grid)
    pert = _init(grid).copy()
    pert["Q"] = np.nextafter(pert["Q"], np.inf)
    out, _ = ol.oracle_trace(p, pert)
    return parity.compare_rays(out, oracle_run(regime, integrator, grid), rtol=parity.rtol_for(p))["frac_bad"]


def steps_total(rays):
    """Steps of a trace that started at steps = 0, summed over the records it wrote (a ray cut at the step limit carries its count negated)."""
    live = rays["steps"] != -1
    return int(np.abs(rays["steps"][live].astype(np.int64)).sum())


def longest(rays):
    live = rays["steps"] != -1
    return int(np.abs(rays["steps"][live].astype(np.int64)).max()) if live.any() else 0
