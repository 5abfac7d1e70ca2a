"""CPU: the disc flow "Keplerian, plunging inside the ISCO" (include/kr_trace.h, KR_V_PLUNGE) -- the identities of the numpy rule
(tests/plunge_rules.py), the host helpers kr_plunge_flow / kr_plunge_velocity against it, and the refusals of every entry point that takes V and does
not take the flow.  No GPU: a refusal is KR_EINVAL before anything touches a device."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import angle_rules as ar  # noqa: E402
import golden_cases as gc  # noqa: E402
import plunge_rules as pr  # noqa: E402
import source_vel_rules as svr  # noqa: E402
from raytrace_cpu_amd import api, capi  # noqa: E402

SPINS = (0.0, 0.5, 0.998)
EPS = np.finfo(np.float64).eps
EINVAL = -1                      # KR_EINVAL (include/kr_trace.h)


def radii(a):
    """nine radii from 1.001 r_h to r_ms"""
    r_h = 1 + math.sqrt((1 - a) * (1 + a))
    return np.linspace(1.001 * r_h, pr.r_ms(a), 9)


def g_at(r, a):
    g, _ = ar.metric(r, np.full_like(r, np.pi / 2), a)
    return g


def records(case="ps_h5_a05", run="rk4_flatdisc"):
    c = gc.cases()[case]
    return np.ascontiguousarray(np.load(gc.golden_path(case))[f"final__{run}"]), c["runs"][run].spin


# ---- identities -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", SPINS)
def test_four_velocity_is_normalised(a):
    r = radii(a)[:-1]                                   # (r_ms itself: the circular orbit, below)
    u = pr.velocity(r, a)
    worst = float(np.abs(ar.dot_product(g_at(r, a), u, u) - 1).max())
    print(f"a = {a}: |g(u, u) - 1| <= {worst:.2e}")
    assert worst <= 1e-9
    assert (u[1] < 0).all() and (u[0] > 0).all()


def test_schwarzschild_radial_velocity_closed_form():
    r = radii(0.0)
    u = pr.velocity(r, 0.0)
    want = -((6 / r - 1) ** 1.5) / 3
    worst = float(np.abs(u[1] - want).max())
    print(f"a = 0: |u^r + (6 / r - 1)^(3/2) / 3| <= {worst:.2e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("a", SPINS)
def test_all_four_legs_are_orthonormal(a):
    r = radii(a)[:-1]
    g, tetrad = pr.tetrad_at(r, np.full_like(r, np.pi / 2), a)
    worst = 0.0
    for i in range(4):
        for j in range(4):
            want = 0.0 if i != j else (1.0 if i == 0 else -1.0)
            worst = max(worst, float(np.abs(ar.dot_product(g, tetrad[i], tetrad[j]) - want).max()))
    print(f"a = {a}: |g(e_i, e_j) - eta_ij| <= {worst:.2e}")
    assert worst <= 1e-9
    assert (tetrad[3][1] > 0).all() and (tetrad[1][3] > 0).all()          # e3^r > 0, e1^phi > 0


@pytest.mark.parametrize("a", SPINS)
def test_flow_joins_the_circular_orbit_at_r_ms(a):
    rm = np.array([pr.r_ms(a)])
    u, circ = pr.velocity(rm, a), pr.circular_velocity(rm, a)
    # u^r = 0: the radicand is a sum of O(1) terms that cancel exactly for the circular orbit's own constants, so what is left is their rounding,
    # at most a few ulp of the largest term (2 / r <= 2): |radicand| <= 16 eps.  (Its square root, ~1e-8, is not a bound on anything.)
    rad = float(pr.radicand(rm, a)[0])
    print(f"a = {a}: radicand at r_ms {rad:.2e}")
    assert abs(rad) <= 16 * EPS
    assert abs(float(u[0][0]) / float(circ[0][0]) - 1) <= 1e-12 and abs(float(u[3][0]) / float(circ[3][0]) - 1) <= 1e-12
    # and the rule itself puts r = r_ms on the circular side: u^r is exactly 0 there
    rays = np.zeros(1, dtype=capi.RAY_F64)
    rays["r"], rays["theta"], rays["steps"] = rm[0], np.pi / 2, 1
    assert not pr.inside(rays, a, 0)[0]
    assert api.plunge_velocity(a, rm[0])[1] == 0.0


# ---- on fixture records -------------------------------------------------------------------------------------------------------------------------
def test_mu_is_the_closed_form_with_the_plunge_energy():
    rays, spin = records()
    ins = pr.inside(rays, spin, 0) & ar.disc_filter(rays, 0.0, 1e9)
    assert ins.sum() == 436
    f = pr.frame(rays, spin, pr.V_PLUNGE, 0, 0)
    mu, _ = ar.mu_chi(f)
    want = ar.mu_closed_form(rays, f, spin)
    fin = ins & np.isfinite(want)
    assert fin.sum() >= 400
    worst = float(np.abs(mu - want)[fin].max())
    print(f"|mu - closed form| <= {worst:.2e} on {int(fin.sum())} records inside the ISCO")
    assert worst <= 1e-12
    # outside r_ms the frame is V = -1's, bit for bit
    kep = ar.frame(rays, spin, -1.0, 0, 0)
    out = ~pr.inside(rays, spin, 0)
    for k in ("E", "P_r", "P_th", "P_phi"):
        assert np.array_equal(f[k][out], kep[k][out], equal_nan=True)
        assert not np.array_equal(f[k][ins], kep[k][ins], equal_nan=True) or k == "P_th"


def test_energy_and_legs_against_the_emitter_rule():
    """tests/source_vel_rules.py restates g(u, p) and the Gram-Schmidt legs for an arbitrary four-velocity, one point at a time: fed the flow's u at the
    records' own end points it must give the E and the legs of this rule."""
    rays, spin = records()
    idx = np.flatnonzero(pr.inside(rays, spin, 0) & ar.disc_filter(rays, 0.0, 1e9))[::9]
    assert len(idx) >= 40
    sub = rays[idx]
    f = pr.frame(sub, spin, pr.V_PLUNGE, 0, 0)
    u = pr.velocity(sub["r"], spin)
    p = ar.momentum_from_consts(sub["k"], sub["h"], sub["Q"], sub["rdot_sign"], sub["thetadot_sign"], sub["r"], sub["theta"], spin)
    _, (et, e1, e2, e3) = pr.tetrad_at(sub["r"], sub["theta"], spin)
    worst_e = worst_n = worst_leg = off_plane = 0.0
    for i, ray in enumerate(sub):
        ui = [float(c[i]) for c in u]
        fr = svr.tetrad([0.0, float(ray["r"]), float(ray["theta"]), 0.0], ui, spin)
        pi = [float(c[i]) for c in p]
        e_raw = svr.dot(fr["g"], ui, pi)[0]                       # u as given
        e_unit = svr.dot(fr["g"], fr["un"], pi)[0]                # the rule's emitter energy: u / sqrt(g(u, u))
        worst_e = max(worst_e, abs(float(f["E"][i]) / e_raw - 1))
        worst_n = max(worst_n, abs(float(f["E"][i]) / (e_unit * math.sqrt(fr["norm_u"])) - 1))
        off_plane = max(off_plane, abs(fr["norm_u"] - 1))
        for mine, leg in ((e3, 3), (e1, 2), (e2, 1)):
            worst_leg = max(worst_leg, max(abs(float(mine[c][i]) - fr["tetrad"][leg][c]) for c in range(4)))
    print(f"E against g(u, p): {worst_e:.2e}; against sqrt(g(u, u)) x the normalised emitter's: {worst_n:.2e}; legs: {worst_leg:.2e}; "
          f"|g(u, u) - 1| at the records' own theta <= {off_plane:.2e}")
    assert worst_e <= 1e-12          # the same sixteen terms of the same metric
    # the emitter rule normalises u; E is linear in u, so the two differ by exactly sqrt(g(u, u)) -- which is 1 only ON the plane: the records end at
    # |z| < 1e-2 and the rule takes the equatorial u in the metric at their own theta (include/kr_trace.h)
    assert worst_n <= 1e-12
    assert worst_leg <= 1e-9


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", SPINS + (-0.5,))
def test_helpers_match_the_rule(a):
    rc, got = pr.helper_flow(a)
    assert rc == 0
    want = pr.flow(a)
    assert got[0] == want[0] == api.lib().kr_kerr_isco(a, 1)
    assert abs(got[1] / float(want[1]) - 1) <= 4 * EPS and abs(got[2] / float(want[2]) - 1) <= 4 * EPS
    assert api.plunge_flow(a) == got
    r_h = 1 + math.sqrt((1 - a) * (1 + a))
    for r in list(np.linspace(1.001 * r_h, got[0], 9)[:-1]) + [got[0], 1.5 * got[0], 50.0]:
        u = api.plunge_velocity(a, r)
        ra = np.array([r])
        want_u = pr.velocity(ra, a) if r < got[0] else pr.circular_velocity(ra, a)
        for c in range(4):
            w = float(want_u[c][0])
            assert abs(u[c] - w) <= 1e-13 * max(1.0, abs(w)), (a, r, c, u[c], w)
        assert u[2] == 0 and (u[1] < 0) == (r < got[0])


def test_helpers_refuse_bad_arguments():
    L = api.lib()
    u = (C.c_double * 4)()
    x = C.c_double()
    assert L.kr_plunge_flow(0.5, None, C.byref(x), C.byref(x)) == EINVAL and b"kr_plunge_flow" in L.kr_last_error()
    assert L.kr_plunge_flow(1.5, C.byref(x), C.byref(x), C.byref(x)) == EINVAL
    assert L.kr_plunge_velocity(0.5, 3.0, None) == EINVAL and b"kr_plunge_velocity" in L.kr_last_error()
    for r in (1.0, float("nan"), float("inf")):
        assert L.kr_plunge_velocity(0.5, r, u) == EINVAL
    with pytest.raises(capi.KrError):
        api.plunge_velocity(0.5, 1.0)


def test_constant_and_abi():
    assert capi.V_PLUNGE == -2.0 == pr.V_PLUNGE
    assert api.lib().kr_abi_version() == 16 == capi.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    assert "#define KR_V_PLUNGE (-2.0)" in text and "#define KR_ABI_VERSION 16" in text


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def refusal_calls():
    """[(name expected in kr_last_error, callable -> rc)] for every entry point that takes V and refuses the flow; pointers are dummies that a refusal
    never reads."""
    L = api.lib()
    VP = capi.V_PLUNGE
    rays = np.zeros(4, dtype=capi.RAY_F64)
    rays32 = np.zeros(4, dtype=capi.RAY_F32)
    h, h32 = rays.ctypes.data_as(C.c_void_p), rays32.ctypes.data_as(C.c_void_p)
    buf = np.zeros(64)
    out = buf.ctypes.data_as(C.c_void_p)
    d = C.c_void_p(16)
    PI = math.pi
    ps, ps_ok = capi.PointSourceSpec(), capi.PointSourceSpec()
    ps.V = VP
    ip = capi.ImagePlaneSpec()
    vm, cs, hs = capi.VolumeMap(), capi.CrossingSpec(), capi.HealpixSource()
    vm.V, cs.V, hs.V = VP, VP, VP
    p = capi.default_params(0.5)
    ob = capi.ObserveBins()
    ptrs, ns = (C.c_void_p * 1)(d), (C.c_int64 * 1)(4)
    Vs = (C.c_double * 1)(VP)
    keep = [rays, rays32, buf, ps, ps_ok, ip, vm, cs, hs, p, ob, ptrs, ns, Vs]
    rm, hm, ad, hot = capi.ReturnMap(), capi.HealpixMap(), capi.AngdistSpec(), capi.HotSpot()
    lb, ib, limb, pol = capi.LineBins(), capi.ImageBins(), capi.LimbLaw(), capi.PolLaw()
    sm, resp = capi.SpectrumModel(), capi.ResponseModel()
    emis, mub = capi.EmisBins(), capi.MuBins()
    keep += [rm, hm, ad, hot, lb, ib, limb, pol, sm, resp, emis, mub]
    B = C.byref
    calls = [
        # the f32 passes, and redshift_start in every form
        ("kr_redshift_f32", lambda: L.kr_redshift_f32(0.5, VP, 0, 0, 0, h32, 4)),
        ("kr_redshift_f32", lambda: L.kr_redshift_dev_f32(0.5, VP, 0, 0, 0, d, 4, None)),
        ("kr_redshift_start", lambda: L.kr_redshift_start_f64(0.5, VP, 0, 0, h, 4)),
        ("kr_redshift_start", lambda: L.kr_redshift_start_dev_f64(0.5, VP, 0, 0, d, 4, None)),
        ("kr_redshift_start_f32", lambda: L.kr_redshift_start_f32(0.5, VP, 0, 0, h32, 4)),
        ("kr_redshift_start_f32", lambda: L.kr_redshift_start_dev_f32(0.5, VP, 0, 0, d, 4, None)),
        # motion = 1 in the passes that take the flow with motion = 0
        ("kr_redshift", lambda: L.kr_redshift_f64(0.5, VP, 0, 0, 1, h, 4)),
        ("kr_redshift", lambda: L.kr_redshift_dev_f64(0.5, VP, 0, 0, 1, d, 4, None)),
        ("kr_post_emissivity", lambda: L.kr_post_emissivity_dev_f64(0.5, VP, 0, 0, 1, -PI, PI, B(emis), d, 4, d, None)),
        ("kr_post_image", lambda: L.kr_post_image_dev_f64(0.5, VP, 0, 0, 1, -PI, PI, B(ib), d, 4, d, None)),
        ("kr_post_line", lambda: L.kr_post_line_dev_f64(0.5, VP, 0, 0, 1, -PI, PI, B(lb), d, 4, d, None)),
        ("kr_post_spectrum", lambda: L.kr_post_spectrum_dev_f64(0.5, VP, 0, 0, 1, -PI, PI, B(sm), B(limb), d, 4, d, None)),
        ("kr_post_response", lambda: L.kr_post_response_dev_f64(0.5, VP, 0, 0, 1, -PI, PI, B(resp), B(limb), d, 4, d, None)),
        # the hot spot, polarisation, the return map and its batch, the HEALPix map, the angular distribution
        ("kr_post_hotspot", lambda: L.kr_post_hotspot_dev_f64(0.5, VP, 1, 0, 0, -PI, PI, B(hot), B(limb), d, 4, d, None)),
        ("kr_polarisation", lambda: L.kr_polarisation_dev_f64(0.5, VP, 1, 0, 0, 60.0, d, 4, d, None)),
        ("kr_polarisation", lambda: L.kr_polarisation_f64(0.5, VP, 1, 0, 0, 60.0, h, 4, out)),
        ("kr_post_image_stokes", lambda: L.kr_post_image_stokes_dev_f64(0.5, VP, 1, 0, 0, -PI, PI, 60.0, B(ib), B(limb), B(pol), d, 4, d, None)),
        ("kr_post_line_stokes", lambda: L.kr_post_line_stokes_dev_f64(0.5, VP, 1, 0, 0, -PI, PI, 60.0, B(lb), B(limb), B(pol), d, 4, d, None)),
        ("kr_post_return_map", lambda: L.kr_post_return_map_dev_f64(0.5, VP, 0, 0, 0, -PI, PI, B(rm), d, 4, d, None)),
        ("kr_post_return_map_batch", lambda: L.kr_post_return_map_batch_dev_f64(1, 0.5, VP, 0, 0, 0, -PI, PI, B(rm), ptrs, ns, ptrs, None)),
        ("kr_post_healpix_map", lambda: L.kr_post_healpix_map_dev_f64(0.5, VP, 0, 0, 0, -PI, PI, B(hm), d, 4, 0, 1, d, None)),
        ("kr_post_angdist", lambda: L.kr_post_angdist_dev_f64(0.5, VP, 0, 0, 0, -PI, PI, B(ad), d, 4, d, None)),
        # the V of a volume map and of a crossing spec
        ("kr_trace_volume", lambda: L.kr_trace_volume_f64(B(p), B(vm), h, 4, out, None)),
        ("kr_trace_volume", lambda: L.kr_trace_volume_dev_f64(B(p), B(vm), d, 4, d, None, None)),
        ("kr_trace_observe", lambda: L.kr_trace_observe_dev_f64(B(p), B(vm), B(ob), d, d, d, d, 4, d, d, None, None)),
        ("kr_trace_crossings", lambda: L.kr_trace_crossings_f64(B(p), B(cs), h, 4, out, out, None)),
        ("kr_trace_crossings", lambda: L.kr_trace_crossings_dev_f64(B(p), B(cs), d, 4, d, d, None, None)),
        # every ray-source constructor
        ("kr_pointsource_init", lambda: L.kr_pointsource_init_f64(B(ps), h, 4)),
        ("kr_pointsource_init", lambda: L.kr_pointsource_init_dev_f64(B(ps), d, 4, None)),
        ("kr_pointsource_init_strided", lambda: L.kr_pointsource_init_strided_dev_f64(B(ps), 0, 1, d, 4, None)),
        ("kr_pointsource_init_emit", lambda: L.kr_pointsource_init_emit_dev_f64(B(ps_ok), 0, 1, VP, 0, 0, d, 4, None)),
        ("kr_pointsource_init_emit", lambda: L.kr_pointsource_init_emit_dev_f64(B(ps), 0, 1, 0.0, 0, 0, d, 4, None)),
        ("kr_pointsource_init_emit_batch", lambda: L.kr_pointsource_init_emit_batch_dev_f64(1, B(ps_ok), Vs, 0, 0, ptrs, ns, None)),
        ("kr_pointsource_init_emit_batch", lambda: L.kr_pointsource_init_emit_batch_dev_f64(1, B(ps), None, 0, 0, ptrs, ns, None)),
        ("kr_imageplane_init_emit", lambda: L.kr_imageplane_init_emit_dev_f64(B(ip), 0, 1, VP, 1, 0, d, 4, None)),
        ("kr_imageplane_init_emit_runs", lambda: L.kr_imageplane_init_emit_runs_dev_f64(B(ip), 0, 1, 1, VP, 1, 0, d, 4, None)),
        ("kr_bundles_init_emit", lambda: L.kr_bundles_init_emit_dev_f64(B(ip), 0.01, VP, 1, 0, d, 20, None)),
        ("kr_healpix_init", lambda: L.kr_healpix_init_f64(B(hs), h, 4)),
        ("kr_healpix_init", lambda: L.kr_healpix_init_dev_f64(B(hs), 0, 1, d, 4, None)),
        ("kr_healpix_init_emit", lambda: L.kr_healpix_init_emit_dev_f64(B(hs), 0, 1, 0, d, 4, None)),
    ]
    return calls, keep


def test_every_other_entry_point_refuses_the_flow():
    L = api.lib()
    calls, keep = refusal_calls()
    assert len(calls) >= 40
    for name, call in calls:
        rc = call()
        msg = L.kr_last_error().decode()
        assert rc == EINVAL, (name, rc, msg)
        assert msg.startswith(name + ":") and "KR_V_PLUNGE" in msg, (name, msg)
    del keep
