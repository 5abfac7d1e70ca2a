"""The ray grid of the radial-ray tests (TEST INFRASTRUCTURE; shared by tests/test_radial_precondition.py and tests/test_gpu_radial.py).

bench.py's lamp post (h = 10 at theta_0 = 1e-3, a = 0.998) on 200 rows of cos(alpha) and 3 columns of beta starting at -pi: the beta = -pi column is
the one the hybrid classifier flags; about half of it is RADIAL (raytrace_cpu_amd/csrc/kr_device.hpp: the polar numerator of thetadot^2 rounds to
exactly zero, the ray never leaves theta_0), with the column's longest rays among them, the other half leaves theta_0 after one turning-point flip;
the two other columns are ordinary rays."""
import functools
import math

import numpy as np

import bench
import oracle_lib as ol
from raytrace_cpu_amd import capi

ROWS, COLUMNS = 200, 3


def spec():
    s = bench.make_spec(capi, 1.99 / (ROWS - 1))
    s.dbeta = 0.01
    s.betamax = -math.pi + (COLUMNS - 0.5) * s.dbeta
    return s


def params(integrator, **kw):
    p = capi.default_params(bench.SPIN)
    p.integrator, p.r_max = integrator, bench.R_MAX
    return capi.copy_params(p, **kw) if kw else p


@functools.lru_cache(maxsize=None)
def _init():
    rays = ol.oracle_pointsource(spec())
    ol.oracle().kro_redshift_start_f64(bench.SPIN, 0.0, 0, 0, ol.ptr(rays), len(rays))
    rays.setflags(write=False)
    return rays


def init():
    """The rays as the source emits them (a fresh copy)."""
    return _init().copy()


@functools.lru_cache(maxsize=None)
def _oracle(integrator):
    out, _ = ol.oracle_trace(params(integrator), _init())
    out.setflags(write=False)
    return out


def oracle(integrator):
    """The CPU oracle's trace of init() (computed once per process; read-only)."""
    return _oracle(integrator)


def flagged(rays):
    """The column the classifier flags: beta = -pi."""
    return (np.abs(np.sin(rays["beta"])) < 1e-9) & (rays["steps"] >= 0)


def held(before, after):
    """Rays whose theta has the same bits after the trace as before it."""
    return flagged(before) & (before["theta"].view(np.uint64) == after["theta"].view(np.uint64))
