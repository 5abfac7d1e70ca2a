"""Shared by the ray-path tests (TEST INFRASTRUCTURE): the fixtures of tests/golden/paths/ (written by the reference's own code, see
make_paths_golden.sh there), how a .par file becomes the arguments of api.trace_paths, and the block-by-block comparison of two trajectory files.

The comparison rule.  A trajectory file is a sequence of blocks, one per traced ray: its rows (four fields of width 20, scientific, precision 8)
followed by two blank lines.  Two files agree when they have the same number of blocks and, ray by ray, the same number of rows with every printed
field equal or off by one unit in the ninth significant digit -- which is what a relative difference within parity.RAY_RTOL = 1e-9 can do to a
nine-digit print, so no tolerance of its own is introduced.  A ray that misses that is "bad"; the share of bad rays is held to
parity.allowed_bad_frac_strict, the bar of the strict Euler / RK4 traces."""
import gzip
import os
from decimal import Decimal

import numpy as np

from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS_DIR = os.path.join(ROOT, "tests", "golden", "paths")
CASES = ("ps_euler", "ps_euler_window", "ip_euler", "rk4_theta", "rk4_isco", "rk4_window")
APP_OF = {"ps_euler": "kr_trace_rays", "ps_euler_window": "kr_trace_rays", "ip_euler": "kr_trace_rays_imageplane"}


def read_par(path):
    """ParameterFile (src/include/par_file.h): `key = value`, '#' starts a comment."""
    pars = {}
    for line in open(path):
        line = line.split("#", 1)[0]
        if "=" not in line:
            continue
        k, v = line.split("=", 1)
        pars.setdefault(k.strip(), v.strip())
    return pars


def par_path(name):
    return os.path.join(PATHS_DIR, name + ".par")


def reference_text(name):
    with gzip.open(os.path.join(PATHS_DIR, name + ".txt.gz"), "rt", newline="") as f:      # (compressed: five files, 0.96 MB of text)
        return f.read()


def reference_records(name):
    """The final ray records the reference left behind after writing <name>.txt (ref_paths_dump.cpp, records = 1), as a RAY_F64 array with the
    fields parity.compare_rays reads (the others zero)."""
    ints = ("steps", "status", "rdot_sign", "thetadot_sign", "rdot_flips", "equatorial_crossings")
    floats = ("t", "r", "theta", "phi", "pt", "pr", "ptheta", "pphi")
    with gzip.open(os.path.join(PATHS_DIR, name + ".records.txt.gz"), "rt") as f:
        lines = [l.split() for l in f if l.strip()]
    out = np.zeros(len(lines), dtype=capi.RAY_F64)
    for i, w in enumerate(lines):
        for k, v in zip(ints, w[:6]):
            out[k][i] = int(v)
        for k, v in zip(floats, w[6:]):
            out[k][i] = float.fromhex(v)
    return out


def case_inputs(name):
    """(params, initial rays, trace_paths keyword arguments) of a fixture, as the program that wrote it sets them up: trace_rays.cpp:34-71,
    trace_rays_imageplane.cpp:30-61, tests/golden/paths/ref_paths_dump.cpp."""
    par = read_par(par_path(name))
    f = lambda k, d=None: float(par[k]) if k in par else d          # noqa: E731
    spin = f("spin")
    kw = dict(write_step=int(f("write_step", 10.0)), write_rmin=f("write_rmin", -1.0), write_rmax=f("write_rmax", -1.0), cartesian=bool(f("write_cartesian", 1.0)))
    if name.startswith("ip_"):
        nx, ny = int(par["Nx"]), int(par["Ny"])
        s = capi.ImagePlaneSpec()
        s.dist, s.inc_deg, s.spin = f("dist"), f("incl"), spin
        s.x0, s.xmax, s.dx = f("x0"), f("xmax"), (f("xmax") - f("x0")) / (nx - 1)
        s.y0, s.ymax, s.dy = f("y0"), f("ymax"), (f("ymax") - f("y0")) / (ny - 1)
        s.phi0, s.precision = f("tol", 100.0), f("plane_phi0", 0.0)      # (sic: trace_rays_imageplane.cpp:59)
        p = capi.default_params(-spin)
        p.precision, p.integrator, p.theta_max, p.r_max = s.precision, capi.EULER, f("thetamax", 0.0), 1.5 * s.dist
        return p, api.imageplane_init(s), kw
    s = capi.PointSourceSpec()
    for i, x in enumerate(par["source"].split()[:4]):
        s.pos[i] = float(x)
    V = f("V", -1.0 if name.startswith("ps_") else 0.0)
    s.V = V if V >= 0 else 1.0 / (spin + s.pos[1] ** 1.5)
    s.spin, s.tol, s.E = spin, 100.0, 1.0
    s.cosalpha0, s.cosalphamax, s.dcosalpha = f("cosalpha0", -0.995), f("cosalphamax", 0.995), f("dcosalpha")
    s.beta0, s.betamax, s.dbeta = f("beta0", -np.pi), f("betamax", np.pi), f("dbeta")
    p = capi.default_params(spin)
    p.integrator = capi.RK4 if name.startswith("rk4_") else capi.EULER
    p.theta_max, p.r_max = f("theta_max", np.pi / 2), f("r_max", 100.0)
    if int(f("dest", 0)) == 1:
        p.stop_kind = capi.STOP_DISC_ISCO
        for i, x in enumerate((api.lib().kr_kerr_isco(spin, 1), f("r_out", -1.0), np.pi / 2)):      # DiscWithISCODestination(r_isco, r_out, theta_lim = pi / 2)
            p.stop_params[i] = x
    return p, api.pointsource_init(s), kw


def blocks_of(text):
    """The rows of every block, as lists of field strings.  Asserts the file's shape: every block ends in exactly two blank lines."""
    lines = text.split("\n")
    assert lines[-1] == "", "the file does not end in a newline"
    lines.pop()
    blocks, rows, i = [], [], 0
    while i < len(lines):
        if lines[i].strip():
            assert len(lines[i]) % 20 == 0, f"line {i + 1}: fields are not 20 wide"
            rows.append(lines[i].split())
            assert len(rows[-1]) == 4, f"line {i + 1}: expected four fields"
            i += 1
            continue
        assert i + 1 < len(lines) and lines[i + 1] == "" and lines[i] == "", f"line {i + 1}: a block must end in two blank lines"
        blocks.append(rows)
        rows = []
        i += 2
    assert not rows, "rows after the last block's blank lines"
    return blocks


def field_close(a, b):
    """Equal, or off by one unit in the ninth significant digit (of the larger of the two)."""
    if a == b or ("nan" in a and "nan" in b):
        return True
    try:
        x, y = Decimal(a), Decimal(b)
    except Exception:
        return False
    if not (x.is_finite() and y.is_finite()):
        return False
    top = max(x.adjusted() if x else -10**6, y.adjusted() if y else -10**6)
    return abs(x - y) <= Decimal(1).scaleb(top - 8)


def compare_texts(got, want):
    """dict in the shape of parity.compare_rays (n_traced, n_bad, frac_bad, worst_ok, bad_index) plus frac_blocks_identical, n_blocks_got."""
    g, w = blocks_of(got), blocks_of(want)
    res = {"n_blocks_got": len(g), "n_traced": len(w)}
    bad, identical, worst = [], 0, 0.0
    for i, (a, b) in enumerate(zip(g, w)):
        if a == b:
            identical += 1
        elif len(a) != len(b) or not all(field_close(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb)):
            bad.append(i)
        else:           # accepted with differing prints: the largest relative difference of the printed values
            for x, y in ((x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb) if x != y and "nan" not in x):
                worst = max(worst, abs(float(x) - float(y)) / max(abs(float(y)), 1e-300))
    res["worst_ok"] = worst
    res.update(n_bad=len(bad), frac_bad=len(bad) / max(len(w), 1), bad_index=bad, frac_blocks_identical=identical / max(len(w), 1))
    return res
