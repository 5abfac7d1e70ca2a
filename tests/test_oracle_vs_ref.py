"""CPU: the oracle restatement against the compiled reference (oracle/_ref/libkr_ref.so) on the reference tests' full grids
(SURVEY.md section 4).  The reference's output of every case is on file as one SHA-256 digest per ray field
(tests/golden/oracle_vs_ref_digests.json; a NaN counts as any NaN, as in oracle_lib.rays_equal_bitwise), so the oracle is held to it
bit for bit everywhere.  Where the compiled reference is available it is also run live: its rays must equal the oracle's bit for bit and
match the recorded digests.  `python tests/test_oracle_vs_ref.py --record` rewrites the file from the live reference."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import golden_cases as gc
import oracle_lib as ol
import step_control_cases as sc
from raytrace_cpu_amd import capi

DIGESTS = os.path.join(gc.GOLDEN_DIR, "oracle_vs_ref_digests.json")
CANONICAL_NAN = np.float64(np.nan).view(np.int64)


def field_digests(rays):
    """SHA-256 of every field's little-endian bytes, every NaN replaced by the one canonical quiet NaN."""
    out = {}
    for f in rays.dtype.names:
        x = np.ascontiguousarray(rays[f])
        if x.dtype.kind == "f":
            bits = x.astype("<f8").view("<i8").copy()
            bits[np.isnan(x)] = CANONICAL_NAN
            data = bits.tobytes()
        else:
            data = x.astype(x.dtype.newbyteorder("<")).tobytes()
        out[f] = hashlib.sha256(data).hexdigest()
    return out


def recorded():
    with open(DIGESTS) as fh:
        return json.load(fh)["cases"]


def _ref_run(spec, params, start):
    src = ol.RefSource(spec)
    src.lib.ref_redshift_start(src.h, *start)
    src.run(params)
    ref_out = src.snapshot()
    src.close()
    return ref_out


def _oracle_run(spec, params, start):
    rays = ol.oracle_imageplane(spec) if isinstance(spec, capi.ImagePlaneSpec) else ol.oracle_pointsource(spec)
    ol.oracle().kro_redshift_start_f64(params.spin, *start, ol.ptr(rays), len(rays))
    out, _ = ol.oracle_trace(params, rays)
    return out


def _check(case, spec, params, start):
    out = _oracle_run(spec, params, start)
    want = recorded()[case]
    got = field_digests(out)
    assert sorted(got) == sorted(want)
    assert [f for f in want if got[f] != want[f]] == []
    if ol.ref() is not None:
        ref_out = _ref_run(spec, params, start)
        assert ol.rays_equal_bitwise(ref_out, out) == []
        assert field_digests(ref_out) == want
    return out


def _perf_case(method, h):
    # integrator_perf_test.cpp:35-45 grid (5167 allocated rays), at the reference's h=5 and BASELINE's h=10
    spec = ol.pointsource_spec([0.0, h, 1e-3, 0.0], 0.0, gc.SPIN, 0.05, 0.05, cosalpha0=-0.995, cosalphamax=0.995,
                               beta0=-np.pi, betamax=np.pi)
    p = capi.default_params(gc.SPIN)
    p.integrator = method
    return f"perf_test_grid-m{method}-h{h:g}", spec, p, (0.0, 0, 0)


def _imageplane_case(method):
    spec = ol.imageplane_spec(10000.0, 80.0, -30.0, 30.0, 60.0 / 32, -30.0, 30.0, 60.0 / 32, gc.SPIN)
    p = capi.default_params(-gc.SPIN)
    p.integrator, p.r_max = method, 11000.0
    return f"imageplane_33-m{method}", spec, p, (0.0, 1, 0)


def _rk45_case(tol):
    # emissivity_rk45_tol_sweep.py:38 end points
    spec = ol.pointsource_spec([0.0, 5.0, 1e-3, 0.0], 0.0, gc.SPIN, 0.1, 0.1, cosalpha0=-0.995, cosalphamax=0.995,
                               beta0=-np.pi, betamax=np.pi)
    p = capi.default_params(gc.SPIN)
    p.integrator, p.rk45_tol = capi.RK45, tol
    return f"rk45_tolerance-{tol:g}", spec, p, (0.0, 0, 0)


def _without_theta_precision(over):
    return {k: v for k, v in over.items() if k != "theta_precision"}


def _step_control_case(regime, method):
    # the perf_test grid at h = 5 under a step-control regime (tests/step_control_cases.py)
    grid = sc.lamp()
    p = sc.grid_params(sc.DEFAULT, method, grid, **_without_theta_precision(sc.REGIMES[regime]))
    return f"step_control-{regime}-m{method}", sc.source_spec(grid, p.precision), p, sc.redshift_start_args(grid)


# the 33 x 33 image plane: a coarse precision with an inner boundary inside the photon orbit's reach, and both caps off
PLANE_REGIMES = {"coarse_boundary": dict(precision=20.0, horizon=2.5), "caps_off": sc.REGIMES["caps_off"]}


def _step_control_plane_case(regime, method):
    grid = sc.plane33()
    p = sc.grid_params(sc.DEFAULT, method, grid, **PLANE_REGIMES[regime])
    return f"step_control-plane33-{regime}-m{method}", sc.source_spec(grid, p.precision), p, sc.redshift_start_args(grid)


PERF = [(m, h) for h in (5.0, 10.0) for m in (capi.EULER, capi.RK4, capi.RK45)]
IMAGEPLANE = [capi.EULER, capi.RK4]
RK45_TOL = [1e-6, 1e-10]
STEP_CONTROL = [(r, m) for r in sc.NAMES for m in (capi.EULER, capi.RK4, capi.RK45)]
STEP_CONTROL_PLANE = [(r, m) for r in PLANE_REGIMES for m in IMAGEPLANE]


@pytest.mark.parametrize("method", [capi.EULER, capi.RK4, capi.RK45])
@pytest.mark.parametrize("h", [5.0, 10.0])
def test_perf_test_grid_bitwise(method, h):
    out = _check(*_perf_case(method, h))
    assert len(out) == 5167


@pytest.mark.parametrize("method", IMAGEPLANE)
def test_imageplane_33_bitwise(method):
    out = _check(*_imageplane_case(method))
    assert len(out) == 33 * 33


@pytest.mark.parametrize("tol", RK45_TOL)
def test_rk45_tolerance_bitwise(tol):
    _check(*_rk45_case(tol))


@pytest.mark.parametrize("regime,method", STEP_CONTROL, ids=[f"{r}-m{m}" for r, m in STEP_CONTROL])
def test_step_control_regimes_bitwise(regime, method):
    """The oracle off the default step-control parameters: precision (the constructor's tol), set_max_tstep, set_max_phistep and set_boundary, each
    moved to where the heuristic takes another branch.  theta_precision stays at its default here: the reference cannot vary it -- its set_precision
    assigns its parameters to themselves (raytracer.h:169-178), which the host mirror copies on purpose -- so that the oracle divides by
    theta_precision where the reference does (kr_oracle.c:276,359 against raytracer.cpp:227,858,1139,1353) is established by reading only."""
    out = _check(*_step_control_case(regime, method))
    assert len(out) == 5167 and (out["steps"] != -1).sum() == 5040


@pytest.mark.parametrize("regime,method", STEP_CONTROL_PLANE, ids=[f"{r}-m{m}" for r, m in STEP_CONTROL_PLANE])
def test_step_control_imageplane_33_bitwise(regime, method):
    out = _check(*_step_control_plane_case(regime, method))
    assert len(out) == 33 * 33


def record():
    """Runs every case on the live compiled reference and writes its digests."""
    assert ol.ref() is not None, "compiled reference (oracle/_ref) not available"
    cases = {}
    for name, spec, p, start in ([_perf_case(m, h) for m, h in PERF] + [_imageplane_case(m) for m in IMAGEPLANE] +
                                 [_rk45_case(t) for t in RK45_TOL] + [_step_control_case(r, m) for r, m in STEP_CONTROL] +
                                 [_step_control_plane_case(r, m) for r, m in STEP_CONTROL_PLANE]):
        cases[name] = field_digests(_ref_run(spec, p, start))
    with open(DIGESTS, "w") as fh:
        json.dump({"what": "SHA-256 per ray field of the compiled reference's rays after redshift_start + run_raytrace "
                           "(tests/test_oracle_vs_ref.py::field_digests)", "cases": cases}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
