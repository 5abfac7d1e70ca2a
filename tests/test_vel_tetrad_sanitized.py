"""CPU: the host tetrad code (raytrace_cpu_amd/csrc/kr_vel_tetrad.hpp) in a stand-alone program (tests/cpp/vel_tetrad_check.cpp) built with
-fsanitize=address,undefined and run once per emitter: no report, and the printed tetrad, normalised four-velocity and g(u, u) equal the numpy
rule bit for bit.  Also on a four-velocity that is not timelike (the library refuses it before it would use the frame): the arithmetic must still be
defined behaviour."""
import os
import subprocess

import numpy as np
import pytest

import source_vel_rules as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "vel_tetrad_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("vel_tetrad") / "vel_tetrad_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, pos, u, spin):
    r = subprocess.run([exe] + [repr(float(x)) for x in list(pos) + list(u) + [spin]], capture_output=True, text=True, timeout=60)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return r.returncode, np.array([float.fromhex(x) for x in r.stdout.split()])


@pytest.mark.parametrize("name", sv.EMITTERS)
def test_sanitized_tetrad_equals_the_rule(exe, name):
    pos, u = sv.emitter(name)
    rc, got = run(exe, pos, u, sv.SPIN)
    assert rc == 0 and got.shape == (21,)
    fr = sv.tetrad(pos, u, sv.SPIN)
    want = np.concatenate([fr["tetrad"].ravel(), fr["un"], [fr["norm_u"]]])
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (name, got, want)


def test_sanitized_run_on_a_spacelike_velocity(exe):
    rc, got = run(exe, (0.0, 6.0, 1.2, 0.3), (1.0, 1.5, 0.0, 0.0), sv.SPIN)
    assert rc in (0, 2) and got.shape == (21,) and got[20] < 0                 # g(u, u) < 0 is what the library's validator refuses
