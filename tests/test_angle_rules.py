"""CPU: the photon's angles in the disc frame (include/kr_trace.h, kr_angles_dev_f64).  The numpy restatement tests/angle_rules.py against the closed
form mu = sqrt(|Theta|) / (rho E), against the host mirror's own kerr_metric / tetrad / dot_product / momentum_from_consts (a C++ program compiled
here), and against the Schwarzschild expression; then the new structs and symbols of the C ABI and what its entry points refuse before any device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import angle_rules as ar
import golden_cases as gc
from raytrace_cpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case, run, r_disc, rays on the disc, bad-angle rays among them, largest share of them the test accepts
FIXTURE_RUNS = [("ip15", "rk4", 30.0, 46, 0, 0.01), ("ip16", "rk4", 30.0, 42, 0, 0.01), ("ps_h10", "rk4", 500.0, 691, 2, 0.01), ("ps_h10", "euler", 500.0, 682, 12, 0.025),
                ("ps_kep5k", "rk4", 500.0, 3148, 5, 0.01), ("ps_h5", "rk4", 500.0, 809, 0, 0.01), ("ps_h5_a05", "rk4_flatdisc", 500.0, 1059, 0, 0.01)]
NEW_SYMBOLS = ["kr_angles_dev_f64", "kr_angles_f64", "kr_post_line_limb_dev_f64", "kr_post_emissivity_mu_dev_f64"]


def fixture_run(case, run):
    """(records, spin as the trace stored it, (V, reverse, projradius) of the case's redshift pass)."""
    c = gc.cases()[case]
    return np.load(gc.golden_path(case))[f"final__{run}"], c["runs"][run].spin, c["post"]


@pytest.mark.parametrize("case,run,r_disc,n_disc,n_bad,max_share", FIXTURE_RUNS, ids=[f"{c}-{r}" for c, r, *_ in FIXTURE_RUNS])
def test_rule_matches_the_closed_form(case, run, r_disc, n_disc, n_bad, max_share):
    rays, spin, (V, reverse, projradius) = fixture_run(case, run)
    f = ar.frame(rays, spin, V, reverse, projradius)
    disc = ar.disc_filter(rays, gc.r_isco(abs(spin)), r_disc)
    bad = ar.bad_angle(f) & disc
    assert (int(disc.sum()), int(bad.sum())) == (n_disc, n_bad)
    assert bad.sum() <= max_share * disc.sum()
    mu, chi = ar.mu_chi(f)
    worst = float(np.nanmax(np.abs(mu - ar.mu_closed_form(rays, f, spin))[disc]))
    good = disc & ~bad
    null = float((np.abs(f["E"] ** 2 - f["P_r"] ** 2 - f["P_th"] ** 2 - f["P_phi"] ** 2) / f["E"] ** 2)[good].max())
    print(f"{case}/{run}: |mu - closed form| <= {worst:.2e}, null condition <= {null:.2e}, mu in [{mu[good].min():.3f}, {mu[good].max():.3f}]")
    assert worst <= 1e-14
    assert null <= 1e-12
    assert (mu[good] >= 0).all() and (mu[good] <= 1).all() and (np.abs(chi[good]) <= np.pi).all()
    assert np.isnan(mu[rays["steps"] <= 0]).all() and np.isnan(chi[rays["steps"] <= 0]).all()


def test_five_mu_bins_are_populated_on_the_point_sources():
    for case in ("ps_h10", "ps_h5", "ps_kep5k"):
        rays, spin, (V, reverse, projradius) = fixture_run(case, "rk4")
        f = ar.frame(rays, spin, V, reverse, projradius)
        good = ar.disc_filter(rays, gc.r_isco(spin), 500.0) & ~ar.bad_angle(f)
        mu, _ = ar.mu_chi(f)
        assert (np.bincount(np.minimum((mu[good] * 5).astype(int), 4), minlength=5) > 0).all(), case


MIRROR_CPP = r"""
#include <cstdio>
#include "kerr.h"
// stdin: spin a V reverse, then records "r theta k h Q rdot_sign thetadot_sign"; stdout: g(p, e_t) g(p, e1) g(p, e2) g(p, e3) per record
int main()
{
    double spin, a, V;
    int reverse;
    if (std::scanf("%lf %lf %lf %d", &spin, &a, &V, &reverse) != 4) return 1;
    double r, theta, k, h, Q;
    int rs, ts;
    while (std::scanf("%lf %lf %lf %lf %lf %d %d", &r, &theta, &k, &h, &Q, &rs, &ts) == 7) {
        double x[4] = {0, r, theta, 0}, g[4][4], et[4], e1[4], e2[4], e3[4], p[4];
        kerr_metric<double>(g, x, a);
        const double Vr = (V == -1) ? 1 / (a + r * std::sqrt(r)) : V;
        tetrad<double>(et, e1, e2, e3, x, Vr, a);
        momentum_from_consts<double>(p[0], p[1], p[2], p[3], k, h, Q, rs, ts, r, theta, 0.0, spin);
        if (reverse) { p[1] *= -1; p[2] *= -1; p[3] *= -1; }
        std::printf("%.17g %.17g %.17g %.17g\n", dot_product<double>(g, p, et), dot_product<double>(g, p, e1), dot_product<double>(g, p, e2), dot_product<double>(g, p, e3));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def mirror_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("angle_mirror")
    src, exe = d / "angle_mirror.cpp", d / "angle_mirror"
    src.write_text(MIRROR_CPP)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "raytrace_cpu_amd", "host", "include"), "-o", str(exe), str(src)], check=True)
    return str(exe)


@pytest.mark.parametrize("case,run", [("ip15", "rk4"), ("ps_h10", "rk4")])
def test_rule_matches_the_host_mirror(mirror_exe, case, run):
    """g(p, e_i) of about 50 on-disc fixture records from the host mirror's kerr.h against the numpy rule, 1e-13 relative to the photon's energy E
    (the scale of every component: E^2 = P_r^2 + P_th^2 + P_phi^2)."""
    rays, spin, (V, reverse, projradius) = fixture_run(case, run)
    f = ar.frame(rays, spin, V, reverse, projradius)
    pick = np.flatnonzero(ar.disc_filter(rays, gc.r_isco(abs(spin)), 500.0) & ~ar.bad_angle(f))[:50]
    assert len(pick) >= 40
    lines = [f"{spin!r} {(-spin if reverse else spin)!r} {V!r} {reverse}"]
    lines += [" ".join(repr(float(rays[n][i])) for n in ("r", "theta", "k", "h", "Q")) + f" {rays['rdot_sign'][i]} {rays['thetadot_sign'][i]}" for i in pick]
    r = subprocess.run([mirror_exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60)
    got = np.array([[float(x) for x in l.split()] for l in r.stdout.splitlines()])
    assert got.shape == (len(pick), 4)
    want = np.stack([f["E"][pick], -f["P_phi"][pick], -f["P_th"][pick], -f["P_r"][pick]], axis=1)
    rel = np.abs(got - want) / f["E"][pick][:, None]
    print(f"{case}/{run}: host mirror vs rule, worst {rel.max():.2e} of E over {len(pick)} records")
    assert rel.max() <= 1e-13


def test_schwarzschild_static_observer():
    rays = np.load(gc.golden_path("ps_h10_a0"))["final__rk4_flatdisc"]
    f = ar.frame(rays, 0.0, 0.0, 0, 0)
    disc = ar.disc_filter(rays, 6.0, 500.0)
    assert disc.sum() > 500
    mu, _ = ar.mu_chi(f)
    r, th, k = rays["r"][disc], rays["theta"][disc], rays["k"][disc]
    Theta = rays["Q"][disc] - np.cos(th) ** 2 * rays["h"][disc] ** 2 / np.sin(th) ** 2
    want = np.sqrt(np.abs(Theta)) * np.sqrt(1 - 2 / r) / (r * k)
    assert np.abs(mu[disc] - want).max() <= 1e-13


def test_limb_weights():
    mu = np.array([0.25, 0.5, 1.0])
    assert (ar.limb_weight(0, 2.06, mu) == 1).all()
    assert (ar.limb_weight(1, 2.06, mu) == 1 + 2.06 * mu).all()
    np.testing.assert_allclose(ar.limb_weight(2, 0.0, mu), np.log([5.0, 3.0, 2.0]), rtol=1e-15)


# ---- structs, symbols, validation ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def test_structs_and_abi(lib, tmp_path):
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kr_trace.h"\nint main(void) { printf("%d %d %d %d %d\\n", (int) sizeof(kr_limb_law), '
                   '(int) offsetof(kr_limb_law, law), (int) sizeof(kr_mu_bins), (int) offsetof(kr_mu_bins, nmu), KR_ABI_VERSION); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [16, 8, 8, 0, 16]
    assert (C.sizeof(capi.LimbLaw), capi.LimbLaw.law.offset, C.sizeof(capi.MuBins), capi.MuBins.nmu.offset) == (16, 8, 8, 0)
    assert capi.limb_law("laor").law == 1 and capi.limb_law("laor").coeff == 2.06 and capi.limb_law((2, 0.0)).law == 2 and capi.limb_law("isotropic").law == 0
    with pytest.raises(ValueError):
        capi.limb_law("darkening")


def test_new_symbols_are_declared_exported_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kr_trace.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(lib, name) and name in capi.PROTOTYPES, name


def _refusals():
    """[(id, call(lib, pointers), message)]: every one must answer KR_EINVAL with that message, device or not."""
    good_line, good_emis = capi.line_bins(), gc.emis_bins(gc.cases()["ps_h10"]["source"])
    bad_line = capi.line_bins(ne=0)
    nr0 = gc.emis_bins(gc.cases()["ps_h10"]["source"])
    nr0.nr = 0
    law, law3, mb, mb0 = capi.limb_law("laor"), capi.limb_law((3, 1.0)), capi.MuBins(5, 0), capi.MuBins(0, 0)
    lawm = capi.limb_law((-1, 1.0))
    d = C.c_void_p(64)            # a "device pointer": never dereferenced, every call below is refused first
    pi = np.pi
    line = lambda L, **kw: L.kr_post_line_limb_dev_f64(0.998, -1.0, 1, 0, kw.get("motion", 0), -pi, pi, kw.get("b", C.byref(good_line)), kw.get("law", C.byref(law)),  # noqa: E731
                                                       kw.get("d", d), kw.get("n", 4), kw.get("out", d), None)
    emis = lambda L, **kw: L.kr_post_emissivity_mu_dev_f64(0.998, -1.0, 0, 0, kw.get("motion", 0), -pi, pi, kw.get("b", C.byref(good_emis)), kw.get("mb", C.byref(mb)),  # noqa: E731
                                                           kw.get("d", d), kw.get("n", 4), kw.get("hist", d), kw.get("mu", d), None)
    keep = [good_line, good_emis, bad_line, nr0, law, law3, lawm, mb, mb0]
    return keep, [
        ("angles_dev-motion", lambda L: L.kr_angles_dev_f64(0.998, -1.0, 0, 0, 1, d, 4, d, None), "kr_angles: motion must be 0 (the orbiting observer)"),
        ("angles_dev-null-rays", lambda L: L.kr_angles_dev_f64(0.998, -1.0, 0, 0, 0, None, 4, d, None), "kr_angles: null argument or negative n"),
        ("angles_dev-null-out", lambda L: L.kr_angles_dev_f64(0.998, -1.0, 0, 0, 0, d, 4, None, None), "kr_angles: null argument or negative n"),
        ("angles_dev-negative-n", lambda L: L.kr_angles_dev_f64(0.998, -1.0, 0, 0, 0, d, -1, d, None), "kr_angles: null argument or negative n"),
        ("angles-motion", lambda L: L.kr_angles_f64(0.998, -1.0, 0, 0, 2, d, 4, d), "kr_angles: motion must be 0 (the orbiting observer)"),
        ("angles-null-out", lambda L: L.kr_angles_f64(0.998, -1.0, 0, 0, 0, d, 4, None), "kr_angles: null argument or negative n"),
        ("angles-negative-n", lambda L: L.kr_angles_f64(0.998, -1.0, 0, 0, 0, d, -3, d), "kr_angles: null argument or negative n"),
        ("line-null-bins", lambda L: line(L, b=None), "kr_post_line_limb: null bins"),
        ("line-bad-bins", lambda L: line(L, b=C.byref(bad_line)), "kr_post_line_limb: ne and nt must be >= 1"),
        ("line-null-law", lambda L: line(L, law=None), "kr_post_line_limb: null limb law"),
        ("line-law-3", lambda L: line(L, law=C.byref(law3)), "kr_post_line_limb: limb law must be 0 (isotropic), 1 (1 + coeff mu) or 2 (log(1 + 1 / mu))"),
        ("line-law-negative", lambda L: line(L, law=C.byref(lawm)), "kr_post_line_limb: limb law must be 0 (isotropic), 1 (1 + coeff mu) or 2 (log(1 + 1 / mu))"),
        ("line-motion", lambda L: line(L, motion=1), "kr_post_line_limb: motion must be 0 (the orbiting observer)"),
        ("line-null-rays", lambda L: line(L, d=None), "kr_post_line_limb: null argument or negative n"),
        ("line-null-out", lambda L: line(L, out=None, n=0), "kr_post_line_limb: null argument or negative n"),
        ("line-negative-n", lambda L: line(L, n=-1), "kr_post_line_limb: null argument or negative n"),
        ("emis-null-bins", lambda L: emis(L, b=None), "kr_post_emissivity_mu: null bins"),
        ("emis-null-mu-bins", lambda L: emis(L, mb=None), "kr_post_emissivity_mu: null bins"),
        ("emis-nr-0", lambda L: emis(L, b=C.byref(nr0)), "kr_post_emissivity_mu: nr must be positive"),
        ("emis-nmu-0", lambda L: emis(L, mb=C.byref(mb0)), "kr_post_emissivity_mu: nmu must be >= 1"),
        ("emis-motion", lambda L: emis(L, motion=1), "kr_post_emissivity_mu: motion must be 0 (the orbiting observer)"),
        ("emis-null-rays", lambda L: emis(L, d=None), "kr_post_emissivity_mu: null argument or negative n"),
        ("emis-null-hist", lambda L: emis(L, hist=None, n=0), "kr_post_emissivity_mu: null argument or negative n"),
        ("emis-null-mu", lambda L: emis(L, mu=None), "kr_post_emissivity_mu: null argument or negative n"),
        ("emis-negative-n", lambda L: emis(L, n=-2), "kr_post_emissivity_mu: null argument or negative n"),
    ]


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
    rays, angles = np.zeros(4, dtype=capi.RAY_F64), np.zeros(8)
    b, law, eb, mb = capi.line_bins(), capi.limb_law("laor"), gc.emis_bins(gc.cases()["ps_h10"]["source"]), capi.MuBins(5, 0)
    assert lib.kr_angles_dev_f64(0.998, -1.0, 0, 0, 0, d, 4, d, None) == capi.KR_ENODEVICE
    assert lib.kr_angles_f64(0.998, -1.0, 0, 0, 0, rays.ctypes.data_as(C.c_void_p), 4, angles.ctypes.data_as(C.c_void_p)) == capi.KR_ENODEVICE
    assert lib.kr_post_line_limb_dev_f64(0.998, -1.0, 1, 0, 0, -pi, pi, C.byref(b), C.byref(law), d, 4, d, None) == capi.KR_ENODEVICE
    assert lib.kr_post_emissivity_mu_dev_f64(0.998, -1.0, 0, 0, 0, -pi, pi, C.byref(eb), C.byref(mb), d, 4, d, d, None) == capi.KR_ENODEVICE
    assert b"no HIP device" in lib.kr_last_error() and (angles == 0).all()
