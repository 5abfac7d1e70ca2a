"""CPU: the option reader and setup that the image-plane disc programs share (raytrace_cpu_amd/apps/imageplane_app.h, krapp::Options in app_common.h).
tests/cpp/app_setup_test prints every field of the kr_imageplane, kr_params, kr_image_bins and AxisInfo it builds from a parameter file and --key=value
arguments; the expected values are worked out here from the file's numbers, and the printed doubles (17 significant digits) must equal them exactly.
Then the three programs that had no such test: without a GPU each exits 1 with the library's message and creates no output file."""
import math
import os
import subprocess

import pytest

import golden_cases as gc
from raytrace_cpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPS = os.path.join(ROOT, "tests", "golden", "apps")
EXE = os.path.join(ROOT, "tests", "cpp", "app_setup_test")
ENV = {k: v for k, v in os.environ.items() if k != "KRTRACE_ARITHMETIC"}
REQUIRED = {"outfile": "unused.fits", "dist": "1234.5", "incl": "61.25", "spin": "0.7", "r_disc": "41.7", "Nx": "13"}
INTEGRATORS = {"euler": capi.EULER, "rk4": capi.RK4, "rk45": capi.RK45}
ARITHMETIC = {"strict": 0, "hybrid": capi.FLAG_HYBRID, "fast": capi.FLAG_FAST_MATH}


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), EXE], check=True)
    return EXE


def read_par(path):
    """key -> text, as ParameterFile stores it: `#` starts a comment, the first value of a repeated key is kept."""
    keys = {}
    for line in open(path):
        line = line.split("#")[0]
        if "=" in line:
            k, v = line.split("=", 1)
            keys.setdefault(k.strip(), v.strip())
    return keys


def expected(keys, arithmetic=None):
    """name -> value of every line the program prints, from the keys (the file's, overridden by the command line's)."""
    num = lambda k, d=None: float(keys[k]) if k in keys else d
    dist, incl, spin, r_disc = num("dist"), num("incl"), num("spin"), num("r_disc")
    x0 = num("x0", -r_disc)
    xmax = num("xmax", r_disc)
    Nx = int(keys["Nx"])
    y0 = num("y0", x0)
    ymax = num("ymax", xmax)
    Ny = int(keys.get("Ny", Nx))
    img_nx = int(keys.get("img_Nx", Nx))
    img_ny = int(keys.get("img_Ny", img_nx))
    precision = num("precision", 100.0)
    dx, dy = (xmax - x0) / Nx, (ymax - y0) / Ny
    want = {"plane.dist": dist, "plane.inc_deg": incl, "plane.x0": x0, "plane.xmax": xmax, "plane.dx": dx, "plane.y0": y0, "plane.ymax": ymax, "plane.dy": dy,
            "plane.spin": spin, "plane.phi0": num("plane_phi0", 0.0), "plane.precision": precision}
    # the seven overrides of the defaults: precision, integrator, rk45_tol (RK45 only), theta_max, r_max, stop_kind, flags
    p = capi.default_params(-spin)
    p.precision = precision
    p.integrator = INTEGRATORS.get(keys.get("integrator", "rk45"), capi.RK45)
    if p.integrator == capi.RK45:
        p.rk45_tol = num("rk45_tol", 1e-8)
    p.theta_max = math.pi / 2
    p.r_max = 1.1 * dist
    p.stop_kind = capi.STOP_THETA
    p.flags = ARITHMETIC[arithmetic] if arithmetic else (0 if p.integrator == capi.RK45 else capi.FLAG_HYBRID)
    for name, _ in capi.Params._fields_:
        if name == "stop_params":
            want.update({f"p.stop_params{i}": p.stop_params[i] for i in range(4)})
        else:
            want[f"p.{name}"] = getattr(p, name)
    want.update({"b.x0": x0, "b.y0": y0, "b.img_dx": (xmax - x0) / img_nx, "b.img_dy": (ymax - y0) / img_ny, "b.r_isco": gc.r_isco(spin), "b.r_disc": r_disc,
                 "b.q1": num("q1", 3.0), "b.rb1": num("rb1", 4.0), "b.q2": num("q2", 3.0), "b.rb2": num("rb2", 10.0), "b.q3": num("q3", 3.0),
                 "b.img_nx": img_nx, "b.img_ny": img_ny, "b.flip_image": int(keys.get("flip_image", 1)), "b.pad": 0})
    want.update({"ax.x0": x0, "ax.xmax": xmax, "ax.dx": dx, "ax.y0": y0, "ax.ymax": ymax, "ax.dy": dy, "ax.img_nx": img_nx, "ax.img_ny": img_ny})
    return want


def run(exe, par, *args):
    return subprocess.run([exe, f"--parfile={par}", *args], capture_output=True, text=True, timeout=60, env=ENV)


def check(exe, par, args=(), arithmetic=None):
    keys = read_par(par)
    keys.update(a[2:].split("=", 1) for a in args)
    r = run(exe, par, *args, *([f"--arithmetic={arithmetic}"] if arithmetic else []))
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "Done" and lines[-2].split()[0] == "rays" and int(lines[-2].split()[1]) > 0
    got = dict(line.split() for line in lines[:-2])
    want = expected(keys, arithmetic)
    assert list(got) == list(want)                  # every field, each once
    for name, value in want.items():
        assert float(got[name]) == value, (name, got[name], value)
        if isinstance(value, int):
            assert got[name] == str(value), (name, got[name], value)


def write_par(path, keys):
    path.write_text("".join(f"{k} = {v}\n" for k, v in keys.items()))
    return str(path)


@pytest.mark.parametrize("par", ["imageplane_rk4", "imageplane_rk45", "hotspot_lightcurve", "disc_spectrum_thermal"])
def test_setup_of_the_golden_parameter_files(exe, par):
    check(exe, os.path.join(APPS, par + ".par"))


def test_every_default_of_a_file_with_only_the_required_keys(exe, tmp_path):
    check(exe, write_par(tmp_path / "required.par", REQUIRED))


def test_command_line_overrides_the_file(exe, tmp_path):
    check(exe, os.path.join(APPS, "imageplane_rk4.par"), ["--incl=33.5", "--x0=-17.25", "--Nx=19"])
    check(exe, write_par(tmp_path / "required.par", REQUIRED), ["--incl=33.5", "--x0=-17.25", "--Nx=19"])


@pytest.mark.parametrize("arithmetic", ["strict", "hybrid", "fast"])
@pytest.mark.parametrize("par", ["imageplane_rk4", "imageplane_rk45"])
def test_arithmetic_choice(exe, par, arithmetic):
    check(exe, os.path.join(APPS, par + ".par"), arithmetic=arithmetic)


def test_unknown_arithmetic_is_refused(exe):
    r = run(exe, os.path.join(APPS, "imageplane_rk4.par"), "--arithmetic=bogus")
    assert r.returncode == 1
    assert r.stderr.strip() == "arithmetic: expected hybrid, strict or fast, got 'bogus'"


def test_missing_Nx_is_named(exe, tmp_path):
    r = run(exe, write_par(tmp_path / "no_nx.par", {k: v for k, v in REQUIRED.items() if k != "Nx"}))
    assert r.returncode == 1
    assert r.stderr.strip() == "ParameterFile ERROR : ParameterFile ERROR: Nx not found in parameter file"


@pytest.mark.parametrize("program,par", [("kr_line_profile", "imageplane_rk4"), ("kr_disc_spectrum", "disc_spectrum_thermal"),
                                         ("kr_hotspot_lightcurve", "hotspot_lightcurve")])
def test_program_fails_loudly_without_gpu(tmp_path, program, par):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raytrace_cpu_amd", "apps")], check=True)
    out = tmp_path / "out.dat"
    r = subprocess.run([os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", program), f"--parfile={os.path.join(APPS, par + '.par')}", f"--outfile={out}"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and not out.exists()
    assert "no HIP device available" in r.stderr or "no ROCm-capable device" in r.stderr
