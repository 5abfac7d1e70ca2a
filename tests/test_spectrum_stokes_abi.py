"""CPU: the C ABI of the continuum's Stokes spectra (kr_post_spectrum_stokes_dev_f64, kr_reduce_spectrum_stokes_dev_f64,
kr_reduce_spectrum_stokes_f64): the three symbols declared, exported and bound, kr_spectrum_model unchanged, every refusal of the header's comment with
its message -- before any device is touched, so the dummy device pointers below are never dereferenced --, `out` untouched by a refused call, and, on a
machine without a GPU, KR_ENODEVICE for a valid call (there is no CPU fallback)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from raytrace_cpu_amd import capi
from test_spectrum_abi import REFUSALS, table, thermal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
DUMMY = C.c_void_p(16)          # a "device pointer": only ever handed to calls that are refused, or made where there is no device
SPIN, INC = 0.998, 30.0
NAMES = ("kr_post_spectrum_stokes_dev_f64", "kr_reduce_spectrum_stokes_dev_f64", "kr_reduce_spectrum_stokes_f64")
WORDS = 3 * 4096 + 4            # the largest buffer a valid model asks for


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def call_all(lib, m=None, law=None, pol=None, V=-1.0, reverse=1, motion=0, inc=INC, out=None, n=4, null=()):
    """The three entry points with one argument set off its valid value: [(who, rc, message)].  m, law, pol: ctypes structs or "null" (a null pointer)
    -- left out, the valid ones.  motion goes to the fused form alone (the reduce forms have none).  null: "rays" and / or "out"."""
    m = thermal() if m is None else m
    law = capi.limb_law("laor") if law is None else law
    pol = capi.pol_law((1, 0.1171)) if pol is None else pol
    ref = lambda s: None if isinstance(s, str) else C.byref(s)          # noqa: E731
    host_rays = np.zeros(4, dtype=capi.RAY_F64)
    host_out = np.full(WORDS, 7.0) if out is None else out
    d_rays, d_out = (None if "rays" in null else DUMMY), (None if "out" in null else DUMMY)
    h_rays, h_out = (None if "rays" in null else host_rays.ctypes.data_as(C.c_void_p)), (None if "out" in null else host_out.ctypes.data_as(C.c_void_p))
    res = []
    rc = lib.kr_post_spectrum_stokes_dev_f64(SPIN, V, reverse, 0, motion, -math.pi, math.pi, inc, ref(m), ref(law), ref(pol), d_rays, n, d_out, None)
    res.append(("kr_post_spectrum_stokes", rc, lib.kr_last_error().decode()))
    rc = lib.kr_reduce_spectrum_stokes_dev_f64(SPIN, V, reverse, 0, inc, ref(m), ref(law), ref(pol), d_rays, n, d_out, None)
    res.append(("kr_reduce_spectrum_stokes", rc, lib.kr_last_error().decode()))
    rc = lib.kr_reduce_spectrum_stokes_f64(SPIN, V, reverse, 0, inc, ref(m), ref(law), ref(pol), h_rays, n, h_out)
    res.append(("kr_reduce_spectrum_stokes", rc, lib.kr_last_error().decode()))
    assert (host_out == 7.0).all() or out is not None                     # a refused call writes nothing
    return res


def refused(res, why, only=None):
    for q, (who, rc, msg) in enumerate(res):
        if only is not None and q not in only:
            continue
        assert rc == capi.KR_EINVAL and msg == f"{who}: {why}", (q, who, rc, msg)


def test_symbols_and_the_unchanged_struct(lib):
    header = open(os.path.join(ROOT, "include", "kr_trace.h")).read()
    exported = open(capi.LIB_PATH, "rb").read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name            # declared
        assert name.encode() in exported and hasattr(lib, name)              # exported
        assert name in capi.PROTOTYPES and getattr(lib, name).argtypes == capi.PROTOTYPES[name][1]          # bound
    assert int(re.search(r"static_assert\(sizeof\(kr_spectrum_model\) == (\d+)", header).group(1)) == C.sizeof(capi.SpectrumModel) == 168
    assert capi.ABI_VERSION == 16 == lib.kr_abi_version()                    # additive
    assert "STOKES SPECTRA" in header
    assert len(capi.PROTOTYPES["kr_post_spectrum_stokes_dev_f64"][1]) == 15 and len(capi.PROTOTYPES["kr_reduce_spectrum_stokes_dev_f64"][1]) == 12
    assert len(capi.PROTOTYPES["kr_reduce_spectrum_stokes_f64"][1]) == 11


@pytest.mark.parametrize("label,make,why", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_of_the_model(lib, label, make, why):
    """Every refusal of spectrum_validate (the list of tests/test_spectrum_abi.py), under the new function names."""
    refused(call_all(lib, m=make() if make else "null"), why)


def test_the_refusals_of_the_polarisation_entry_points(lib):
    refused(call_all(lib, reverse=0), "reverse must be 1 (the rule is stated for image-plane records)")
    refused(call_all(lib, reverse=2), "reverse must be 1 (the rule is stated for image-plane records)")
    refused(call_all(lib, motion=1), "motion must be 0 (the orbiting observer)", only=(0,))
    for inc in (NAN, INF, -INF):
        refused(call_all(lib, inc=inc), "non-finite inclination")
    refused(call_all(lib, V=capi.V_PLUNGE), "V = KR_V_PLUNGE (the plunging disc flow) is not supported here")
    refused(call_all(lib, m=table(), V=capi.V_PLUNGE), "V = KR_V_PLUNGE (the plunging disc flow) is not supported here")


def test_bad_laws_are_refused(lib):
    refused(call_all(lib, law="null"), "null limb law")
    for law in (3, -1):
        refused(call_all(lib, law=capi.limb_law((law, 0.0))), "limb law must be 0 (isotropic), 1 (1 + coeff mu) or 2 (log(1 + 1 / mu))")
    refused(call_all(lib, law=capi.limb_law((1, NAN))), "non-finite limb coefficient")
    refused(call_all(lib, pol="null"), "null pol law")
    for law in (2, -1):
        refused(call_all(lib, pol=capi.pol_law((law, 0.1))), "pol law must be 0 (constant) or 1 (coeff (1 - mu) / (1 + 3.582 mu))")
    refused(call_all(lib, pol=capi.pol_law((0, NAN))), "non-finite pol coefficient")
    for coeff in (1.5, -1.0000001):
        refused(call_all(lib, pol=capi.pol_law((1, coeff))), "pol coefficient must lie in [-1, 1]")


def test_null_pointers_and_negative_counts_are_refused(lib):
    why = "null argument or negative n"
    for m in (thermal(), table()):
        refused(call_all(lib, m=m, null=("rays",)), why)
        refused(call_all(lib, m=m, null=("out",)), why)
        refused(call_all(lib, m=m, n=-1), why)
        refused(call_all(lib, m=m, n=0, null=("out",)), why)
        refused(call_all(lib, m=m, n=0, null=("rays", "out")), why)


def test_a_refused_call_leaves_out_as_it_was(lib):
    out = np.full(WORDS, 7.0)
    for kw in (dict(reverse=0), dict(inc=NAN), dict(pol=capi.pol_law((0, 2.0))), dict(m=thermal(f_col=0.0)), dict(m=table(nz=0)), dict(n=-1), dict(V=capi.V_PLUNGE),
               dict(law=capi.limb_law((3, 0.0)))):
        res = call_all(lib, out=out, **kw)
        assert all(rc == capi.KR_EINVAL for _, rc, _ in res), kw
        assert (out == 7.0).all(), kw


@pytest.mark.parametrize("make", [thermal, table, lambda: table(table_emis=np.ones(8).ctypes.data_as(C.POINTER(C.c_double)), table_nr=8, table_r_min=1.2, table_dr=1.3),
                                  lambda: thermal(ne=4096), lambda: table(ne=1)], ids=["thermal", "table", "table+emis", "ne4096", "ne1"])
@pytest.mark.parametrize("pol", [(0, 0.3), (1, 0.1171), (0, 0.0), (1, -1.0)])
def test_valid_calls_reach_the_device_check(lib, make, pol):
    """Without a GPU a valid call ends in KR_ENODEVICE and writes nothing.  With one, only n = 0 is tried here (anything else would run kernels on the
    dummy pointers): KR_OK, and nothing is added."""
    m, plaw = make(), capi.pol_law(pol)
    if lib.kr_device_count() > 0:
        res = call_all(lib, m=m, pol=plaw, n=0, null=("rays",))
        assert [rc for _, rc, _ in res][:2] == [capi.KR_OK, capi.KR_OK]
        return
    out = np.full(WORDS, 7.0)
    res = call_all(lib, m=m, pol=plaw, out=out)
    assert [rc for _, rc, _ in res] == [capi.KR_ENODEVICE] * 3
    assert all("no HIP device" in msg for _, _, msg in res)
    assert (out == 7.0).all()


def program(args, tmp_path):
    apps = os.path.join(ROOT, "tests", "golden", "apps")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raytrace_cpu_amd", "apps")], check=True)
    out = tmp_path / "out.dat"
    r = subprocess.run([os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_disc_spectrum"), f"--parfile={os.path.join(apps, 'disc_spectrum_stokes.par')}",
                        f"--outfile={out}", *args], capture_output=True, text=True, timeout=120, cwd=apps)
    return r, out


def test_program_refuses_the_plunging_flow_with_the_pol_keys(lib, tmp_path):
    """plunge = 1 together with a pol key: exit 1 with a message, before anything is traced (so with or without a device), and no file."""
    r, out = program(["--plunge=1"], tmp_path)
    assert r.returncode == 1 and not out.exists()
    assert "the Stokes spectra do not take the plunging disc flow" in r.stderr + r.stdout
    assert "no HIP device" not in r.stderr and "no ROCm-capable device" not in r.stderr


def test_program_with_the_pol_keys_fails_loudly_without_gpu(lib, tmp_path):
    """kr_disc_spectrum with pol_law / pol_coeff (tests/golden/apps/disc_spectrum_stokes.par, settings only): without a device exit 1 and no file."""
    if lib.kr_device_count() > 0:
        return                                                               # (with a device: tests/test_gpu_spectrum_stokes.py runs the program)
    r, out = program([], tmp_path)
    assert r.returncode == 1 and not out.exists()
    assert "no HIP device available" in r.stderr or "no ROCm-capable device" in r.stderr
