"""GPU: the program raytrace_cpu_amd/apps/kr_angdist against api.source_angdist on the same source, for both of its modes: the reference's disc
source (tests/golden/apps/angdist_disc.par: a PointSource on the Keplerian orbit at r = 3, the half of its sky above the disc) and an emitter with
its own four-velocity (angdist_vel.par: an orbiting and outflowing blob off the disc).  The 13-column table must equal api.angdist_text of the
Python result to the printed digits, and the three printed fractions api's fractions at cout's six significant digits."""
import math
import os
import subprocess

import pytest

from raytrace_cpu_amd import api, capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPS = os.path.join(ROOT, "raytrace_cpu_amd", "apps")
PAR = os.path.join(ROOT, "tests", "golden", "apps")
SPIN = 0.998


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "-C", APPS], check=True)
    return os.path.join(APPS, "_build", "kr_angdist")


def run(exe, *argv):
    env = dict(os.environ, KRTRACE_ARITHMETIC="strict")                 # api.source_angdist below traces with flags = 0
    r = subprocess.run([exe, *argv], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def params():
    p = capi.default_params(SPIN)
    p.integrator, p.r_max, p.theta_max, p.stop_kind = capi.EULER, 1.1 * 1000.0, math.pi / 2, capi.STOP_THETA
    return p


def fractions(stdout):
    got = {line.split(":")[0]: float(line.split(":")[1]) for line in stdout.splitlines() if line.startswith(("Escape:", "Return:", "Lost:"))}
    assert set(got) == {"Escape", "Return", "Lost"}
    return got


def check(stdout, text, res):
    assert text == api.angdist_text(res)
    assert len(text.splitlines()) == 62 and all(len(row) == 13 * 20 for row in text.splitlines())
    for name, key in (("Escape", "escape"), ("Return", "return"), ("Lost", "lost")):
        assert fractions(stdout)[name] == float("%g" % res[key + "_frac"]), (name, res[key + "_frac"])
    assert res["escape_sum"] > 0 and res["return_sum"] > 0 and res["lost_sum"] > 0 and res["ray_count"] > 100


def test_disc_source_mode_equals_api(exe, tmp_path, krlib):
    V = krlib.kr_disc_velocity(3.0, SPIN, 1)
    spec = capi.PointSourceSpec()
    spec.pos[0], spec.pos[1], spec.pos[2], spec.pos[3] = 0.0, 3.0, math.pi / 2 - 1e-6, 1.5707
    spec.V, spec.spin, spec.tol, spec.E = V, SPIN, 100.0, 1.0
    spec.dcosalpha, spec.dbeta, spec.cosalpha0, spec.cosalphamax, spec.beta0, spec.betamax = 0.06, 0.09, -0.995, 0.995, 0.0, math.pi
    sp = api.angdist_spec(krlib.kr_kerr_isco(SPIN, 1), 1000.0, 1000.0, dangle=0.1, labels=0)        # r_disc := the r_esc key (sic)
    res = api.source_angdist(spec, params(), sp, normalise_az=True)
    out = tmp_path / "disc.dat"
    stdout = run(exe, f"--parfile={os.path.join(PAR, 'angdist_disc.par')}", f"--outfile={out}")
    check(stdout, out.read_text(), res)
    assert "beta = 0 to 3.14159" in stdout


def test_velocity_mode_equals_api(exe, tmp_path, krlib):
    pos = (0.0, 6.0, 1.2, 0.3)
    vel = api.pointsource_vel_spec(pos, (1.0, 0.15, -0.01, 0.06), SPIN, 0.06, 0.18)
    sp = api.angdist_spec(krlib.kr_kerr_isco(SPIN, 1), 400.0, 1000.0, dangle=0.1, limb=1, labels=1)
    res = api.source_angdist(vel, params(), sp, normalise_az=True)
    out = tmp_path / "vel.dat"
    stdout = run(exe, f"--parfile={os.path.join(PAR, 'angdist_vel.par')}", f"--outfile={out}")
    check(stdout, out.read_text(), res)
    with pytest.raises(capi.KrError, match="labels"):
        api.source_angdist(vel, params(), api.angdist_spec(1.24, 400.0, 1000.0, labels=0))
