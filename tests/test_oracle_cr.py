"""CPU: the correctly rounded build of the oracle (oracle/libkr_oracle_cr.so; routing table at the top of oracle/kr_oracle.c).

(1) The shim is the header: oracle/cr_math_shim.cpp's entry points return the bits of a direct host compile of kr_sincos_f64 and krcr::* (tests/cr_shim_check.cpp),
    on tests/test_gpu_fast_step_diet.py's sine / cosine arguments and on the awkward sets of tests/crmath_check.cpp (|x| -> 1, next to pi/2, tiny).
(2) The correctly rounded oracle is the oracle up to glibc: on the fixtures, no ray beyond parity.RAY_RTOL, no integer field and no step count that
    differs; the share of rays with identical bits is recorded, not bounded (glibc 2.35: point sources 0.998-1.0, image planes 0.965-0.983 -- the
    shares the device shows against the plain oracle, reproduced here by swapping nothing but the elementary functions).
(3) The image-plane constructor with cr = True against the plain one, held the way tests/test_gpu_geometry_sweep.py holds the device's."""
import os
import subprocess

import numpy as np
import pytest

import exact_parity_cases as xp
import oracle_lib as ol
import parity


# ---- (1) the shim is the header -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def direct_compile(tmp_path_factory):
    """The two headers compiled for the host on their own, as tests/test_crmath_accuracy.py compiles them."""
    exe = str(tmp_path_factory.mktemp("cr_shim") / "cr_shim_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(xp.gc.ROOT, "tests", "cr_shim_check.cpp"), "-lm"])

    def run(name, a, b=None):
        d = os.path.dirname(exe)
        np.concatenate([a] if b is None else [a, b]).astype(np.float64).tofile(os.path.join(d, "in.bin"))
        subprocess.check_call([exe, str(ol.CR_OPS[name]), os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
        return np.fromfile(os.path.join(d, "out.bin"), dtype=np.float64)
    return run


def _same_bits(x, y):
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


def test_the_shim_returns_the_headers_bits(direct_compile):
    from test_gpu_fast_step_diet import sincos_arguments
    sets = {"sin": (sincos_arguments(), None), "cos": (sincos_arguments(), None)}
    sets.update(xp.awkward_sets())
    # the polar angles and azimuths a trace actually passes, small angles (kr_sincos_small_f64) and the library range included
    more = np.concatenate([np.linspace(-1e-2, 1e-2, 4001), [1e-300, 5e-324, 1023.999, 1024.0, -1500.25, 1e6, np.inf, np.nan]])
    for name in ("sin", "cos"):
        sets[name] = (np.concatenate([sets[name][0], more, sets["tan"][0]]), None)
    for name, (a, b) in sets.items():
        want = direct_compile(name, a, b)
        got = ol.cr_apply(name, a, b)
        assert len(want) == len(a) and _same_bits(got, want).all(), (name, int((~_same_bits(got, want)).sum()))
        # ... and the scalar entry points the oracle calls are the array one
        fn = getattr(ol.oracle_cr(), f"kro_cr_{name}")
        for i in range(0, len(a), max(1, len(a) // 200)):
            one = np.array([fn(a[i]) if b is None else fn(a[i], b[i])])
            assert _same_bits(one, got[i:i + 1]).all(), (name, a[i])


def test_the_routines_differ_from_glibc_somewhere_and_rarely():
    """What the correctly rounded build changes is small: on uniform arguments the shim differs from numpy's (the C library's) function on fewer than
    0.5 % of them (tests/test_crmath_accuracy.py's bar for glibc 2.35) -- a shim that had picked up another routine would not."""
    rng = np.random.default_rng(7)
    x = rng.uniform(-7, 7, 200000)
    for name, f in (("sin", np.sin), ("cos", np.cos), ("tan", np.tan)):
        d = int((~_same_bits(ol.cr_apply(name, x), f(x))).sum())
        assert d <= 0.005 * len(x), (name, d)


# ---- (2) the correctly rounded oracle is the oracle up to glibc ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_name,run", xp.CPU_RUNS, ids=lambda v: v)
def test_cr_oracle_is_the_oracle_up_to_glibc(case_name, run):
    plain, st_plain = xp.oracle_run(case_name, run, False)
    cr, st_cr = xp.oracle_run(case_name, run, True)
    res = parity.compare_rays(cr, plain, rtol=parity.RAY_RTOL, steps_slack=0)
    share, _ = xp.bit_identical_share(cr, plain)
    parity.record_margin("test_cr_oracle_is_the_oracle_up_to_glibc", f"{case_name}-{run}", res, None, frac_bit_identical_every_field=share,
                         exemptions={}, steps_total_plain=st_plain["steps_total"], steps_total_cr=st_cr["steps_total"])
    print(f"cr oracle vs plain {case_name}-{run}: rays {res['n_traced']}, bit-identical {res['frac_bit_identical']:.4f} (every field {share:.4f}), beyond 1e-9 {res['n_bad']}, "
          f"integer fields {res['n_int_fields_differ']}, steps {res['n_steps_differ']}, worst {res['worst_ok']:.3e}")
    assert res["n_traced"] == int((xp.init(case_name)["steps"] >= 0).sum()) > 0
    assert res["n_bad"] == 0 and res["n_int_fields_differ"] == 0 and res["n_steps_differ"] == 0, res
    assert st_cr["steps_total"] == st_plain["steps_total"] == xp.steps_total(xp.init(case_name), cr)


# ---- (3) the image-plane constructor -------------------------------------------------------------------------------------------------------------------
def _specs():
    c = xp.cases()
    out = [("ip15", c["ip15"]["source"]), ("ip16", c["ip16"]["source"])]
    out += [(f"incl{pl[0]}-a{pl[1]}", xp.plane_spec(*pl, rays=1e4)) for pl in xp.PLANES]
    return out


@pytest.mark.parametrize("tag,spec", _specs(), ids=lambda v: v if isinstance(v, str) else "")
def test_cr_imageplane_constructor_is_the_constructor_up_to_glibc(tag, spec):
    want = ol.oracle_imageplane(spec)
    got = ol.oracle_imageplane(spec, cr=True)
    assert len(got) == len(want) and np.array_equal(got["steps"], want["steps"])
    live = want["steps"] == 0
    all_same = live.copy()
    for f in ("t", "r", "theta", "phi", "pt", "pr", "ptheta", "pphi", "k", "h", "Q", "alpha", "beta"):
        g, w = got[f][live], want[f][live]
        all_same[live] &= _same_bits(g, w)
        assert np.array_equal(np.isnan(g), np.isnan(w)), f
        ok = ~np.isnan(w)
        np.testing.assert_allclose(g[ok], w[ok], rtol=1e-13, atol=1e-13 * max(1.0, float(np.nanmax(np.abs(w)))), err_msg=f)
    for f in ("rdot_sign", "thetadot_sign", "status", "rdot_flips", "equatorial_crossings"):
        assert np.array_equal(got[f][live], want[f][live]), f
    # what does not go through a switched call site is untouched: r, pr, alpha, beta, k
    for f in ("t", "r", "pr", "k", "alpha", "beta"):
        assert _same_bits(got[f][live], want[f][live]).all(), f
    n_diff = int((live & ~all_same).sum())
    parity.record_margin("test_cr_imageplane_constructor_is_the_constructor_up_to_glibc", tag, {"n_traced": int(live.sum()), "n_bad": n_diff,
                         "frac_bad": n_diff / live.sum(), "worst_ok": None}, frac_bit_identical_every_field=float(all_same[live].mean()))
    print(f"cr constructor vs plain {tag}: rays {int(live.sum())}, every field bit-identical {all_same[live].mean():.4f}")
