"""CPU: the polarisation rule of include/kr_trace.h (kr_pol_law, kr_polarisation_dev_f64).  The numpy restatement tests/polarisation_rules.py against the
identities the Walker-Penrose constant must satisfy -- its modulus, the transversality and the norm of the emitted vector, gauge invariance, the
asymptotic form that pins the sign convention, the unit norm at the observer -- then the degree law, the new struct and symbols of the C ABI, what
the entry points refuse before any device, and the new program without one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import angle_rules as ar
import golden_cases as gc
import polarisation_rules as pr
from raytrace_cpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC_DEG = 80.0                  # the inclination of the ip15 / ip16 planes
FIXTURE_RUNS = [("ip15", "rk4"), ("ip15", "euler"), ("ip15", "rk4_plane"), ("ip16", "rk4")]
NEW_SYMBOLS = ["kr_polarisation_dev_f64", "kr_polarisation_f64", "kr_post_image_stokes_dev_f64", "kr_post_line_stokes_dev_f64"]


def fixture_run(case, run, which="final"):
    """(records, spin as the trace stored it, (V, reverse, projradius) of the case's redshift pass)."""
    c = gc.cases()[case]
    g = np.load(gc.golden_path(case))
    return np.ascontiguousarray(g["init"] if which == "init" else g[f"final__{run}"]), c["runs"][run].spin, c["post"]


def disc_state(case, run):
    """The rule's state on the disc records (r_isco <= r < 30) of a fixture run: (state, emitted vector f, disc mask, records)."""
    rays, spin, (V, reverse, projradius) = fixture_run(case, run)
    disc = ar.disc_filter(rays, gc.r_isco(), 30.0)
    assert 38 <= disc.sum() <= 77, (case, run, int(disc.sum()))
    with np.errstate(all="ignore"):
        s = pr.disc_state(rays, spin, V, reverse, projradius)
        f, nrm = pr.emitted_vector(s)
    pol = pr.polarisation(rays, spin, INC_DEG, V, reverse, projradius)
    assert not (pol["bad"] & disc).any() and (nrm[disc] > 0).all(), (case, run)       # none bad-angle, none with nrm = 0
    return s, f, disc, rays


@pytest.mark.parametrize("case,run", FIXTURE_RUNS, ids=[f"{c}-{r}" for c, r in FIXTURE_RUNS])
def test_modulus_of_kappa_is_carters_constant(case, run):
    """kappa1^2 + kappa2^2 = Q + (L - a E)^2 with E = g_t,mu p^mu and L = -g_phi,mu p^mu."""
    s, f, disc, rays = disc_state(case, run)
    g, p, a = s["g"], s["p"], s["a"]
    with np.errstate(all="ignore"):
        k1, k2 = pr.walker_penrose(p, f, s["r"], s["theta"], a)
        E = g[0][0] * p[0] + g[0][3] * p[3]
        L = -1 * (g[3][0] * p[0] + g[3][3] * p[3])
        want = rays["Q"] + (L - a * E) ** 2
        rel = (np.abs(k1 * k1 + k2 * k2 - want) / want)[disc]
    print(f"{case}/{run}: {int(disc.sum())} disc records, |kappa|^2 against Q + (L - a E)^2 <= {rel.max():.2e}")
    assert rel.max() <= 1e-12


@pytest.mark.parametrize("case,run", FIXTURE_RUNS, ids=[f"{c}-{r}" for c, r in FIXTURE_RUNS])
def test_emitted_vector_is_transverse_and_unit(case, run):
    s, f, disc, _ = disc_state(case, run)
    with np.errstate(all="ignore"):
        gfp, gff = ar.dot_product(s["g"], f, s["p"])[disc], ar.dot_product(s["g"], f, f)[disc]
    print(f"{case}/{run}: |g(f, p)| <= {np.abs(gfp).max():.2e}, |g(f, f) + 1| <= {np.abs(gff + 1).max():.2e}")
    assert np.abs(gfp).max() <= 1e-12 and np.abs(gff + 1).max() <= 1e-12


@pytest.mark.parametrize("case,run", FIXTURE_RUNS, ids=[f"{c}-{r}" for c, r in FIXTURE_RUNS])
def test_kappa_is_gauge_invariant(case, run):
    """f -> f + 0.37 p leaves kappa alone (p is null and kappa is antisymmetric in (p, f))."""
    s, f, disc, _ = disc_state(case, run)
    with np.errstate(all="ignore"):
        k1, k2 = pr.walker_penrose(s["p"], f, s["r"], s["theta"], s["a"])
        j1, j2 = pr.walker_penrose(s["p"], [f[i] + 0.37 * s["p"][i] for i in range(4)], s["r"], s["theta"], s["a"])
        rel = (np.hypot(j1 - k1, j2 - k2) / np.hypot(k1, k2))[disc]
    print(f"{case}/{run}: kappa under f -> f + 0.37 p moves by <= {rel.max():.2e}")
    assert rel.max() <= 1e-9


def test_asymptotic_sign_convention():
    """On the plane itself (the init records of ip15, r ~ 1e4) a vector along e_phi must come out as (f_al, f_be) = (1, 0) and one along -e_theta as
    (0, 1), to the finite distance of the plane (b / D <= 4e-3; measured 3e-4).  This pins every sign of the rule."""
    rays, spin, (_, reverse, _) = fixture_run("ip15", "rk4", which="init")
    assert len(rays) == 256 and reverse == 1 and rays["r"].min() > 9000
    r, th = rays["r"].astype(np.float64), rays["theta"].astype(np.float64)
    a = -spin
    g, _ = ar.metric(r, th, a)
    p = ar.momentum_from_consts(rays["k"], rays["h"], rays["Q"], rays["rdot_sign"], rays["thetadot_sign"], r, th, spin)
    p = [p[0], -1 * p[1], -1 * p[2], -1 * p[3]]
    zero = np.zeros_like(r)
    u = [1 / np.sqrt(g[0][0]), zero, zero, zero]
    sin_i = np.sin(INC_DEG * np.pi / 180)
    for name, f, want in (("e_phi", [zero, zero, zero, 1 / (r * np.sin(th))], (1.0, 0.0)), ("-e_theta", [zero, zero, -1 / r, zero], (0.0, 1.0))):
        lam = ar.dot_product(g, f, p) / ar.dot_product(g, u, p)
        ft = [f[i] - lam * u[i] for i in range(4)]                      # made transverse to p without leaving the observer's rest space
        k1, k2 = pr.walker_penrose(p, ft, r, th, a)
        f_al, f_be = pr.observer_vector(k1, k2, rays["alpha"], rays["beta"], a, sin_i)
        worst = max(float(np.abs(f_al - want[0]).max()), float(np.abs(f_be - want[1]).max()))
        print(f"{name}: (f_al, f_be) within {worst:.2e} of {want}")
        assert worst <= 1e-3, name


@pytest.mark.parametrize("case,run", FIXTURE_RUNS, ids=[f"{c}-{r}" for c, r in FIXTURE_RUNS])
def test_observer_vector_has_unit_norm(case, run):
    rays, spin, post = fixture_run(case, run)
    disc = ar.disc_filter(rays, gc.r_isco(), 30.0)
    pol = pr.polarisation(rays, spin, INC_DEG, *post)
    n2 = (pol["f_al"] ** 2 + pol["f_be"] ** 2)[disc]
    print(f"{case}/{run}: |f_al^2 + f_be^2 - 1| <= {np.abs(n2 - 1).max():.2e}")
    assert np.abs(n2 - 1).max() <= 1e-3
    c2, s2 = pol["c2"][disc], pol["s2"][disc]
    assert np.abs(c2 * c2 + s2 * s2 - 1).max() <= 1e-14
    dead = rays["steps"] <= 0
    assert all(np.isnan(pol[k][dead]).all() for k in ("kappa1", "kappa2", "c2", "s2"))


def test_degree_law():
    mu = np.linspace(0.0, 1.0, 101)
    d0, d1 = pr.degree(0, 0.3, mu), pr.degree(1, pr.CHANDRASEKHAR, mu)
    assert (d0 == 0.3).all()
    assert d1[0] == pr.CHANDRASEKHAR == 0.1171 and d1[-1] == 0 and (np.diff(d1) < 0).all()
    assert capi.pol_law("chandrasekhar").law == 1 and capi.pol_law("chandrasekhar").coeff == 0.1171 and capi.pol_law((0, -0.5)).coeff == -0.5
    with pytest.raises(ValueError):
        capi.pol_law("rayleigh")


def test_word_layouts():
    """The api's two result layouts against the rules' own readers, and pdeg / evpa: NaN degree where I == 0, the angle of (Q, U) halved."""
    from raytrace_cpu_amd import api
    b = gc.image_bins(gc.cases()["ip15"]["source"], img_n=3)
    assert api.stokes_image_words(b) == 4 * 9 + 2
    words = np.arange(38, dtype=np.float64)
    words[9] = 0.0                                                                       # I of pixel 0
    got, want = api.stokes_image_from_words(b, words), pr.stokes_image_from_words(3, 3, words)
    assert all(np.array_equal(got[k], want[k]) for k in ("nrays", "I", "Q", "U")) and (got["disc_count"], got["bad_pol"]) == (36, 37)
    assert np.isnan(got["pdeg"][0]) and np.array_equal(got["pdeg"][1:], np.hypot(words[19:27], words[28:36]) / words[10:18])
    assert np.array_equal(got["evpa"], 0.5 * np.arctan2(words[27:36], words[18:27]))
    lb = capi.line_bins(ne=4, nt=2, dt=1.0)
    assert api.stokes_line_words(lb) == 4 * 8 + 3
    words = np.arange(35, dtype=np.float64)
    got, want = api.stokes_line_from_words(lb, words), pr.stokes_line_from_words(lb, words)
    assert all(got[k].shape == (2, 4) and np.array_equal(got[k], want[k]) for k in ("count", "I", "Q", "U"))
    assert (got["on_disc"], got["binned"], got["bad_pol"]) == (32, 33, 34) and len(got["energy_edges"]) == 5 and len(got["time_edges"]) == 3


# ---- struct, symbols, validation ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def test_pol_law_struct(tmp_path):
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kr_trace.h"\nint main(void) { printf("%d %d %d\\n", (int) sizeof(kr_pol_law), '
                   '(int) offsetof(kr_pol_law, coeff), (int) offsetof(kr_pol_law, law)); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 0, 8]
    assert (C.sizeof(capi.PolLaw), capi.PolLaw.coeff.offset, capi.PolLaw.law.offset) == (16, 0, 8)


def test_new_symbols_are_declared_exported_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kr_trace.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(lib, name) and name in capi.PROTOTYPES, name


def _refusals():
    """[(id, call(lib), message)]: every one must answer KR_EINVAL with that message, device or not."""
    spec = gc.cases()["ip15"]["source"]
    img, img0, line, line0 = gc.image_bins(spec), gc.image_bins(spec), capi.line_bins(), capi.line_bins(ne=0)
    img0.img_nx = 0
    limb, limb3 = capi.limb_law("laor"), capi.limb_law((3, 1.0))
    pol, pol2, polm, pol_nan, pol_big = (capi.pol_law(x) for x in ((1, 0.1171), (2, 0.1), (-1, 0.1), (0, float("nan")), (0, 1.5)))
    keep = [img, img0, line, line0, limb, limb3, pol, pol2, polm, pol_nan, pol_big]
    d, pi = C.c_void_p(64), np.pi            # a "device pointer": never dereferenced, every call below is refused first

    def rec(L, **kw):
        return L.kr_polarisation_dev_f64(-0.998, -1.0, kw.get("reverse", 1), 0, kw.get("motion", 0), kw.get("inc", 80.0), kw.get("d", d), kw.get("n", 4), kw.get("out", d), None)

    def host(L, **kw):
        return L.kr_polarisation_f64(-0.998, -1.0, kw.get("reverse", 1), 0, kw.get("motion", 0), kw.get("inc", 80.0), kw.get("d", d), kw.get("n", 4), kw.get("out", d))

    def image(L, **kw):
        return L.kr_post_image_stokes_dev_f64(-0.998, -1.0, kw.get("reverse", 1), 0, kw.get("motion", 0), -pi, pi, kw.get("inc", 80.0), kw.get("b", C.byref(img)),
                                              kw.get("limb", C.byref(limb)), kw.get("pol", C.byref(pol)), kw.get("d", d), kw.get("n", 4), kw.get("out", d), None)

    def lin(L, **kw):
        return L.kr_post_line_stokes_dev_f64(-0.998, -1.0, kw.get("reverse", 1), 0, kw.get("motion", 0), -pi, pi, kw.get("inc", 80.0), kw.get("b", C.byref(line)),
                                             kw.get("limb", C.byref(limb)), kw.get("pol", C.byref(pol)), kw.get("d", d), kw.get("n", 4), kw.get("out", d), None)

    cases = []
    for who, call in (("kr_polarisation", rec), ("kr_polarisation", host), ("kr_post_image_stokes", image), ("kr_post_line_stokes", lin)):
        tag = f"{who}-{call.__name__}"
        cases += [
            (f"{tag}-reverse-0", lambda L, call=call: call(L, reverse=0), f"{who}: reverse must be 1 (the rule is stated for image-plane records)"),
            (f"{tag}-motion", lambda L, call=call: call(L, motion=1), f"{who}: motion must be 0 (the orbiting observer)"),
            (f"{tag}-inc-nan", lambda L, call=call: call(L, inc=float("nan")), f"{who}: non-finite inclination"),
            (f"{tag}-inc-inf", lambda L, call=call: call(L, inc=float("inf")), f"{who}: non-finite inclination"),
            (f"{tag}-null-rays", lambda L, call=call: call(L, d=None), f"{who}: null argument or negative n"),
            (f"{tag}-null-out", lambda L, call=call: call(L, out=None), f"{who}: null argument or negative n"),
            (f"{tag}-negative-n", lambda L, call=call: call(L, n=-1), f"{who}: null argument or negative n"),
        ]
    for who, call, null_bins, bad_bins, bad_bins_msg in (("kr_post_image_stokes", image, "null bins", img0, "image size must be positive"),
                                                         ("kr_post_line_stokes", lin, "null bins", line0, "ne and nt must be >= 1")):
        cases += [
            (f"{who}-null-bins", lambda L, call=call: call(L, b=None), f"{who}: {null_bins}"),
            (f"{who}-bad-bins", lambda L, call=call, bb=bad_bins: call(L, b=C.byref(bb)), f"{who}: {bad_bins_msg}"),
            (f"{who}-null-out-n0", lambda L, call=call: call(L, out=None, n=0), f"{who}: null argument or negative n"),
            (f"{who}-null-limb", lambda L, call=call: call(L, limb=None), f"{who}: null limb law"),
            (f"{who}-limb-3", lambda L, call=call: call(L, limb=C.byref(limb3)), f"{who}: limb law must be 0 (isotropic), 1 (1 + coeff mu) or 2 (log(1 + 1 / mu))"),
            (f"{who}-null-pol", lambda L, call=call: call(L, pol=None), f"{who}: null pol law"),
            (f"{who}-pol-2", lambda L, call=call: call(L, pol=C.byref(pol2)), f"{who}: pol law must be 0 (constant) or 1 (coeff (1 - mu) / (1 + 3.582 mu))"),
            (f"{who}-pol-negative", lambda L, call=call: call(L, pol=C.byref(polm)), f"{who}: pol law must be 0 (constant) or 1 (coeff (1 - mu) / (1 + 3.582 mu))"),
            (f"{who}-pol-nan", lambda L, call=call: call(L, pol=C.byref(pol_nan)), f"{who}: non-finite pol coefficient"),
            (f"{who}-pol-above-1", lambda L, call=call: call(L, pol=C.byref(pol_big)), f"{who}: pol coefficient must lie in [-1, 1]"),
        ]
    return keep, cases


_KEEP, REFUSALS = _refusals()


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_bad_arguments_are_refused_before_any_device_work(lib, case):
    _, call, message = case
    assert call(lib) == capi.KR_EINVAL
    assert lib.kr_last_error().decode() == message


def test_valid_calls_need_a_device(lib):
    if lib.kr_device_count() > 0:
        pytest.skip("a GPU is visible: the calls would launch kernels on dummy pointers")
    d, pi = C.c_void_p(64), np.pi
    rays, out = np.zeros(4, dtype=capi.RAY_F64), np.zeros(16)
    img, line, limb, pol = gc.image_bins(gc.cases()["ip15"]["source"]), capi.line_bins(), capi.limb_law("isotropic"), capi.pol_law("chandrasekhar")
    assert lib.kr_polarisation_dev_f64(-0.998, -1.0, 1, 0, 0, 80.0, d, 4, d, None) == capi.KR_ENODEVICE
    assert lib.kr_polarisation_f64(-0.998, -1.0, 1, 0, 0, 80.0, rays.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p)) == capi.KR_ENODEVICE
    assert lib.kr_post_image_stokes_dev_f64(-0.998, -1.0, 1, 0, 0, -pi, pi, 80.0, C.byref(img), C.byref(limb), C.byref(pol), d, 4, d, None) == capi.KR_ENODEVICE
    assert lib.kr_post_line_stokes_dev_f64(-0.998, -1.0, 1, 0, 0, -pi, pi, 80.0, C.byref(line), C.byref(limb), C.byref(pol), d, 4, d, None) == capi.KR_ENODEVICE
    assert b"no HIP device" in lib.kr_last_error() and (out == 0).all()


def test_polarisation_program_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raytrace_cpu_amd", "apps")], check=True)
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_imageplane_polarisation")
    out, spec = tmp_path / "pol.fits", tmp_path / "pol.dat"
    r = subprocess.run([exe, f"--parfile={os.path.join(ROOT, 'tests', 'golden', 'apps', 'imageplane_polarisation.par')}", f"--outfile={out}", f"--spec_outfile={spec}"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and not out.exists() and not spec.exists()
    assert "no HIP device available" in r.stderr or "no ROCm-capable device" in r.stderr
