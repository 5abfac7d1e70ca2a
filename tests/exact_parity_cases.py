"""The cases of the exact-parity tests (TEST INFRASTRUCTURE; shared by tests/test_oracle_cr.py, tests/test_gpu_exact_parity.py and
tests/tool_gpu_first_diff.py).

The strict arithmetic (flags = 0) documents: + - * IEEE, division and square root correctly rounded, no contraction, sin / cos correctly rounded
(kr_sincos_f64), the device image-plane constructor's acos / asin / atan2 / tan correctly rounded (kr_crmath.hpp).  oracle/libkr_oracle_cr.so is the
CPU oracle with those same routines at the same call sites (the table at the top of oracle/kr_oracle.c), so for Euler / RK4 that sentence is an
equality: every ray, every field, every bit.  The traces of both oracles are computed once per process and handed out read-only.

No exemption is defined: for |x| >= 1024 kr_sincos_f64 hands its argument to the library's sincos() -- glibc's in the oracle, the device library's on the
device -- but no fixture ray evaluates one there (the azimuth of ip15 / rk4_plane's captured ray passes 1024 only in the step that ends it on the
horizon, and the horizon test comes before the FlatPlane stop test's cos(phi - phi0))."""
import functools
import math

import numpy as np

import golden_cases as gc
import oracle_lib as ol
from raytrace_cpu_amd import capi


@functools.lru_cache(maxsize=None)
def cases():
    return gc.cases()


def fixed_step_runs():
    """Every Euler / RK4 run of the golden cases: (case name, run name)."""
    return [(c, r) for c, case in cases().items() for r, p in case["runs"].items() if p.integrator != capi.RK45]


# the runs of the measurement that motivated the correctly rounded oracle (plain against correctly rounded oracle, on the CPU alone), with the shares
# of bit-identical rays it gave with glibc 2.35 -- a record of what was seen, not a bar -- and the RayDestination runs away from a = 0.998
CPU_RUNS = [("ps_h10", "rk4"), ("ps_h10", "euler"), ("ps_h5", "rk4"), ("ps_kep5k", "rk4"), ("ip15", "rk4"), ("ip15", "rk4_isco"), ("ip15", "rk4_plane"),
            ("ip16", "rk4"), ("ps_h10_a0", "rk4_isco"), ("ps_h10_a0", "rk4_flatdisc"), ("ps_h5_a05", "rk4_isco"), ("ps_h5_a05", "rk4_flatdisc")]


@functools.lru_cache(maxsize=None)
def init(case_name):
    """The rays as the compiled reference's source emitted them (tests/golden/), read-only."""
    rays = np.load(gc.golden_path(case_name))["init"]
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def oracle_run(case_name, run, cr):
    """(records, stats) of the plain (cr = False) or the correctly rounded (cr = True) oracle's trace of init(case_name); read-only."""
    out, st = ol.oracle_trace(cases()[case_name]["runs"][run], init(case_name), cr=cr)
    out.setflags(write=False)
    return out, st


def steps_total(before, after):
    """Steps one call took, summed over the rays it traced, from the records (a ray cut at the step limit carries its count negated)."""
    live = before["steps"] >= 0
    return int((np.abs(after["steps"][live].astype(np.int64)) - before["steps"][live].astype(np.int64)).sum())


def longest(before, after):
    live = before["steps"] >= 0
    return int((np.abs(after["steps"][live].astype(np.int64)) - before["steps"][live].astype(np.int64)).max()) if live.any() else 0


def bit_identical_share(got, want):
    """(share of the traced rays that carry want's bits in EVERY field, NaN = NaN; mask of the traced rays that do not)."""
    live = want["steps"] != -1
    same = np.ones(len(want), dtype=bool)
    for f in want.dtype.names:
        x, y = got[f], want[f]
        if x.dtype.kind == "f":
            u = f"u{x.dtype.itemsize}"
            same &= (x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))
        else:
            same &= x == y
    return float(same[live].mean()) if live.any() else 1.0, live & ~same


def first_difference(got, want):
    """For an assertion message: the first differing ray and the fields that differ there, with both values."""
    _, differ = bit_identical_share(got, want)
    if not differ.any():
        return None
    i = int(np.flatnonzero(differ)[0])
    fields = {f: (got[f][i].item(), want[f][i].item()) for f in want.dtype.names if not (got[f][i] == want[f][i] or (got[f][i] != got[f][i] and want[f][i] != want[f][i]))}
    return {"rays_differing": int(differ.sum()), "first_ray": i, "fields (got, want)": fields}


@functools.lru_cache(maxsize=None)
def awkward_sets():
    """The argument sets of tests/crmath_check.cpp's generators, 2e4 each, from a fixed seed -- uniform, |x| -> 1, next to pi/2, tiny -- and the
    arguments each routine hands to the C library's case table (+-0, +-1, out of range, |x| >= 1024, inf, NaN): name -> (a, b or None)."""
    rng = np.random.default_rng(20261020)
    n = 20000
    sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    unit = np.concatenate([rng.uniform(-1, 1, n), sign() * (1 - rng.uniform(0, 1e-6, n)), rng.uniform(-1, 1, n) * 1e-5, [1.0, -1.0, 0.0, -0.0, 1.5, np.nan]])
    tan = np.concatenate([rng.uniform(-7, 7, n), rng.uniform(-1e-3, 1e-3, n), 1.5707963267948966 + rng.uniform(-1e-6, 1e-6, n),
                          -1.5707963267948966 + rng.uniform(-1e-6, 1e-6, n), [0.0, -0.0, 1023.9, 1024.0, -2000.0, np.inf, np.nan]])
    ay = np.concatenate([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n) * 1e-6, rng.uniform(-40, 40, n), [0.0, -0.0, 1.0, 1.0, np.inf, np.nan]])
    ax = np.concatenate([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-1e4, 1e4, n), [1.0, -1.0, 0.0, -0.0, 1.0, 1.0]])
    return {"acos": (unit, None), "asin": (unit, None), "tan": (tan, None), "atan2": (ay, ax)}


# the five planes of tests/test_gpu_geometry_sweep.py::test_device_imageplane_constructor_carries_the_reference_bits: (incl, spin, dist, half, phi0)
PLANES = [(5.0, 0.9, 10000.0, 30.0, 0.0), (45.0, 0.5, 10000.0, 60.0, 0.3), (80.0, 0.998, 10000.0, 30.0, 0.0), (89.5, 0.998, 1000.0, 20.0, -1.0), (120.0, 0.0, 5000.0, 15.0, 2.0)]
PLANE_RAYS = 2.5e5


def plane_spec(incl, spin, dist, half, phi0, rays=PLANE_RAYS):
    n = int(math.sqrt(rays)) | 1
    return ol.imageplane_spec(dist, incl, -half, half, 2 * half / n, -half, half, 2 * half / n, spin, phi0=phi0)
