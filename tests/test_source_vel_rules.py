"""CPU: the numpy restatement of the point source with any four-velocity (tests/source_vel_rules.py), which tests/test_gpu_source_vel.py lets judge
the device kernel, held to what must be true of it -- and the library's host tetrad (csrc/kr_vel_tetrad.hpp) held to the restatement bit for bit.

  orthonormality  g(leg_i, leg_j) is +1 / -1 / 0 within ORTHO_ULP ulp of the sum of the absolute terms of that product.  Each is a sum of up to sixteen
                  products of three factors that carry the rounding of a square root, a division and the Gram-Schmidt subtractions: about ten
                  roundings deep, so "a few ulp" is 8 (measured: 1.0 on all four emitters).  The scale is the sum of absolute terms, not 1, because
                  the plunging emitter's u^t is 25 and its products cancel from 600 down to 1.
  null vector     rdot^2 and thetadot^2 rebuilt from (k, h, Q) by angle_rules.momentum_from_consts equal the squares of the components the tetrad
                  launched, relative to the sum of the absolute terms of g(p, p).  MEASURED here on the CPU over the four emitters of the tests
                  (profiles/source_vel_ab.txt): 8.7e-16 and 3.5e-16; the bars are 4 x that, because near-turning-point rays cancel.
  emit            g(u / sqrt(g(u, u)), p) equals E within EMIT_ULP = 8 ulp of the sum of its absolute terms (measured: 3.5 ulp of E on the three slow
                  emitters, 1024 ulp of E = 1.7 ulp of the sum of absolute terms on the plunging one).
  orbital         for u = u^t (1, 0, 0, V) the constants agree with the host PointSource constructor's at (alpha, beta - pi/2): the relabelling is
                  worked out in source_vel_rules.orbital_difference.  Measured 7.0e-16 of the largest |Q| (k: 4.5e-16, h: 6.1e-16); the bar is 4 x.
  radial          for u = (1, 0.3, 0, 0) the constants agree with the HEALPix source's motion = 1 rule for matching directions
                  (source_vel_rules.radial_difference).  Measured 7.1e-16 of the largest |Q| (k, h: 3.4e-16); the bar is 4 x, and
                  tests/test_gpu_source_vel.py holds the device records to the same bar.
"""
import numpy as np
import pytest

import source_vel_rules as sv
from raytrace_cpu_amd import api, capi

ORTHO_ULP = 8
EMIT_ULP = 8
NULL_RDOT_SQ = 4 * 8.7e-16
NULL_THETADOT_SQ = 4 * 3.5e-16
ORBITAL = 4 * 7.0e-16
RADIAL = 4 * 7.1e-16


@pytest.mark.parametrize("name", sv.EMITTERS)
def test_tetrad_is_orthonormal_and_right_handed(name):
    pos, u = sv.emitter(name)
    fr = sv.tetrad(pos, u, sv.SPIN)
    T, g = fr["tetrad"], fr["g"]
    for i in range(4):
        for j in range(4):
            d, scale = sv.dot(g, T[i], T[j])
            want = (1.0 if i == 0 else -1.0) if i == j else 0.0
            assert abs(d - want) <= ORTHO_ULP * sv.EPS * scale, (name, i, j, d, scale)
    assert T[1][2] > 0 and T[2][3] > 0 and T[3][1] > 0 and T[0][0] > 0
    assert fr["norm_u"] > 0


@pytest.mark.parametrize("name", sv.EMITTERS)
def test_library_tetrad_equals_the_rule_bit_for_bit(name):
    spec = sv.spec_of(name)
    got = api.pointsource_vel_tetrad(spec)
    want = sv.tetrad(spec.pos, spec.u, spec.spin)["tetrad"]
    assert np.array_equal(got.view(np.int64), np.ascontiguousarray(want).view(np.int64)), (name, got, want)


@pytest.mark.parametrize("name", sv.EMITTERS)
def test_every_ray_is_a_null_vector(name):
    res = sv.null_residuals(sv.spec_of(name))
    print(name, res)
    assert res["rdot_sq"] <= NULL_RDOT_SQ and res["thetadot_sq"] <= NULL_THETADOT_SQ, (name, res)


@pytest.mark.parametrize("name", sv.EMITTERS)
@pytest.mark.parametrize("E", [1.0, 2.5])
def test_emitted_energy_is_E_in_the_emitters_frame(name, E):
    spec = sv.spec_of(name, E=E)
    L = sv.launched(spec)
    live, fr = L["live"], L["frame"]
    p = [x[live] for x in L["p"]]
    emit, scale = sv.dot(fr["g"], fr["un"], p)
    worst = float((np.abs(emit - E) / (sv.EPS * scale)).max())
    print(name, E, "worst", worst, "ulp of the absolute terms;", float(np.abs(emit / E - 1).max() / sv.EPS), "ulp of E")
    assert worst <= EMIT_ULP, (name, worst)
    rays = sv.records(spec, emit=True)
    assert np.array_equal(rays["emit"][live], emit) and (rays["emit"][~live] == 0).all()


def test_grid_counts_and_dead_slots():
    spec = sv.spec_of("blob")
    n, nc, nb = sv.grid(spec)
    assert (n, nc, nb) == api.pointsource_vel_count(spec) and n > nc * nb > 1000
    rays = sv.records(spec)
    assert (rays["steps"][nc * nb:] == -1).all() and (rays["steps"][:nc * nb] == 0).all()
    # a grid whose last row and column are out of range marks those rays alone (the PointSource rule), not everything after the first of them
    spec = sv.spec_of("blob", dcosalpha=0.25, dbeta=0.5, cosalpha0=-0.75, cosalphamax=0.75, beta0=-2.0, betamax=2.0)
    assert api.pointsource_vel_count(spec) == (63, 7, 9)
    steps = sv.records(spec)["steps"].reshape(7, 9)
    assert (steps[:6, :8] == 0).all() and (steps[6, :] == -1).all() and (steps[:, 8] == -1).all()


@pytest.mark.parametrize("pos,V,spin", sv.ORBITS)
def test_orbital_emitter_agrees_with_the_host_pointsource_constructor(pos, V, spin):
    res = sv.orbital_difference(pos, V, spin)
    print(pos, V, res)
    assert res["rays"] > 1000 and res["signs"]
    assert max(res["k"], res["h"], res["Q"]) <= ORBITAL, res


def test_radial_emitter_agrees_with_the_healpix_motion_1_rule():
    res = sv.radial_difference()
    print(res)
    assert res["signs"] and max(res["k"], res["h"], res["Q"]) <= RADIAL, res


def test_four_velocity_is_normalised_and_refuses_a_spacelike_one():
    pos = (0.0, 6.0, 1.2, 0.3)
    u = api.four_velocity(pos, sv.SPIN, omega=0.06, dr_dt=0.15, dtheta_dt=-0.01)
    assert abs(sv.tetrad(pos, u, sv.SPIN)["norm_u"] - 1) <= 8 * sv.EPS
    assert u[1] / u[0] == pytest.approx(0.15) and u[3] / u[0] == pytest.approx(0.06)
    zamo = api.four_velocity(pos, sv.SPIN)
    assert zamo[1] == 0 and zamo[2] == 0 and zamo[3] / zamo[0] == pytest.approx(float(2 * sv.SPIN * 6.0 / ((36 + sv.SPIN ** 2) ** 2 - sv.SPIN ** 2 * (36 - 12 + sv.SPIN ** 2)
                                                                                                         * np.sin(1.2) ** 2)))
    with pytest.raises(ValueError, match="not timelike"):
        api.four_velocity(pos, sv.SPIN, dr_dt=1.5)
    with pytest.raises(ValueError, match="not timelike"):
        api.four_velocity((0.0, 1.5, np.pi / 2, 0.0), sv.SPIN, omega=0.0)      # at rest inside the ergosphere


def test_angdist_rule_on_hand_made_records():
    """Five records whose bins are known: one per class, one skipped (cos alpha = 0), one out of range (beta = pi + 1)."""
    sp = api.angdist_spec(r_isco=1.24, r_disc=500.0, r_esc=1000.0, dangle=0.1, plane_iso=0, weight_norm=0)
    rays = np.zeros(6, dtype=capi.RAY_F64)
    rays["steps"] = [5, 5, 5, 5, 5, -1]
    rays["alpha"] = [0.5, 0.5, 0.5, 0.0, 0.5, 0.5]
    rays["beta"] = [0.3, 0.3, 0.3, 0.3, np.pi + 1, 0.3]
    rays["r"] = [10.0, 2000.0, 1.1, 10.0, 10.0, 10.0]
    rays["theta"] = [np.pi / 2, 1.0, 1.0, np.pi / 2, np.pi / 2, np.pi / 2]
    rays["redshift"] = [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    out = sv.angdist(sp, rays)
    assert (out["return_count"], out["escape_count"], out["lost_count"], out["skipped"], out["out_of_range"], out["other"], out["bad_g"]) == (1, 1, 1, 1, 1, 0, 1)
    assert out["ray_count"] == 3 and out["total_norm"].sum() == 3
    ia, ib = int((np.arccos(0.5) + np.pi) / 0.1), int((0.3 + np.pi) / 0.1)
    for cls in ("escape", "return", "lost"):
        assert out[cls + "_alpha"][ia] == 1 and out[cls + "_beta"][ib] == 1 and out[cls + "_alpha"].sum() == 1
