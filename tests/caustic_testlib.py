"""TEST INFRASTRUCTURE: what the caustic test modules share besides the rules (tests/caustic_rules.py, tests/source_caustic_rules.py): the fixtures'
names and planes, the coordinate bound of the CPU rule tests, the host mirror's bundle constructor, and the device bundles of the GPU tests
(dev: a raytrace_cpu_amd.devmem.DeviceScope)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import oracle_lib as ol
from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "raytrace_cpu_amd", "host")
CSRC = os.path.join(ROOT, "raytrace_cpu_amd", "csrc")

# (derived in tests/test_source_caustic_rules.py)
COORD_ULPS = 16 * 2.0 ** -52
FIXTURES = {"sphere": ("caustic_sourceplane", "sphere"), "plane-bundles": ("caustic_plane", "plane"), "plane-grid": ("caustic_plane_grid", "plane")}

# a plane away from the fixtures that contains the point (0, 0): 65 x 49 grid points (64 x 48 steps of 0.5), inclination 45 degrees, a = 0.9
OFF = dict(dist=500.0, incl=45.0, spin=0.9, r_disc=20.0, x0=-16.0, xmax=16.0, y0=-12.0, ymax=12.0, phi0=0.0, Nx=64, Ny=48, dx=0.5, dy=0.5, nx=65, ny=49,
           eps_frac=0.01, precision=100.0, rk45_tol=1e-8)

FLOATS = ("t", "r", "theta", "phi", "pt", "pr", "ptheta", "pphi", "k", "h", "Q", "alpha", "beta")
INTS = ("rdot_sign", "thetadot_sign", "status")


def spec_of(g):
    return ol.imageplane_spec(g["dist"], g["incl"], g["x0"], g["xmax"], g["dx"], g["y0"], g["ymax"], g["dy"], g["spin"], phi0=g["phi0"], precision=g["precision"])


def build_bundle_dump(tmp_path):
    """tests/cpp/bundle_ctor_dump.cpp -> tmp_path, with the flags tests/cpp/Makefile uses for host_ctor_dump and absolute rpaths"""
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    exe = os.path.join(str(tmp_path), "bundle_ctor_dump")
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-Wall", "-Wno-unused-parameter", "-I" + HOST, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "bundle_ctor_dump.cpp"), "-L" + HOST, "-lkr_host", "-L" + CSRC, "-lkrtrace",
                    "-Wl,-rpath," + HOST, "-Wl,-rpath," + CSRC], check=True)
    return exe


def mirror_bundles(exe, tmp_path, g, eps_frac):
    """The host mirror's ImagePlaneBundles<double> rays of the plane `g` (caustic_rules.plane_geometry)."""
    out = os.path.join(str(tmp_path), "bundles.bin")
    args = [g["dist"], g["incl"], g["x0"], g["xmax"], g["dx"], g["y0"], g["ymax"], g["dy"], g["spin"], g["phi0"], eps_frac]
    subprocess.run([exe, out] + [repr(float(a)) for a in args], check=True, stdout=subprocess.DEVNULL, timeout=300)
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:4], dtype=np.int32)[0])
    return np.frombuffer(raw[4:], dtype=capi.RAY_F64, count=n).copy()


def device_bundles(dev, g):
    L, spec = dev.lib, spec_of(g)
    n, nx, ny = api.bundles_count(spec)
    assert (nx, ny) == (g["nx"], g["ny"]) and n == 5 * nx * ny
    d = dev.alloc(n * 144)
    capi.check(L, L.kr_bundles_init_emit_dev_f64(C.byref(spec), g["eps_frac"], 0.0, 1, 0, d, n, None), "kr_bundles_init_emit")
    return d, n


def same_bits(a, b):
    if a.dtype.kind == "f":
        return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def bundle_identity_mask(dev, g, tmp_path):
    """[nx, ny]: True where all five device-built rays of the bundle carry the host mirror's bits in every field (emit against the oracle's
    redshift_start on the mirror's rays).  Also returns (device rays, mirror rays with emit)."""
    d, n = device_bundles(dev, g)
    got = dev.fetch(d, n, capi.RAY_F64)
    want = mirror_bundles(build_bundle_dump(tmp_path), tmp_path, g, g["eps_frac"])
    assert len(want) == n
    ol.oracle().kro_redshift_start_f64(-g["spin"], 0.0, 1, 0, ol.ptr(want), n)
    same = np.ones(n, bool)
    for f in FLOATS + INTS + ("emit", "steps"):
        same &= same_bits(got[f], want[f])
    return same.reshape(g["nx"], g["ny"], 5).all(axis=2), got, want


# ---- hand-made records ----------------------------------------------------------------------------------------------------------------------------
RLIM_OR_DEST = capi.STATUS_RLIM | capi.STATUS_DEST          # a synthetic record that is a hit for either source kind
# pixel counts 1, 63, 64, 65, 129: the last-chunk cases of the 64-pixel bundle pass and, with 255, 256, 257 (the 15 x 17, 16 x 16 planes and one beyond),
# of the 256-thread grid pass; nx or ny < 3: every pixel is border
SHAPES = [(1, 1), (7, 9), (8, 8), (5, 13), (3, 43), (15, 17), (16, 16), (257, 3), (2, 9), (9, 2), (1, 70), (70, 1)]


def synthetic(kind, bundles, nx, ny, seed, trailing=0, sprinkle=True):
    """Records of a smooth map image plane -> source (so that determinants exist) with every branch of the rules sprinkled in: steps <= 0, HORIZON,
    STEPLIM, a winding number of their own (another ORDER next door -> SENTINEL), satellites with another rdot_flips / more than pi / 2 away in phi /
    that missed.  The sphere's phi runs through pi inside the grid, so neighbour pairs straddle the branch cut of PHI_S.  `trailing` records with
    steps = -1 follow, full of values that would be hits: they are no pixels."""
    rng = np.random.default_rng(seed)
    rpb = 5 if bundles else 1
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    rays = np.zeros((nx, ny, rpb), dtype=capi.RAY_F64)
    da = (0.0, 1.0, -1.0, 0.0, 0.0)
    db = (0.0, 0.0, 0.0, 1.0, -1.0)
    for m in range(rpb):
        a, b = ix + 0.01 * da[m], iy + 0.01 * db[m]                       # image-plane position in pixels
        q = rays[:, :, m]
        q["r"] = 1000.0 if kind == "sphere" else 800.0 + 3.0 * a + 2.0 * b
        q["theta"] = 1.0 + 0.011 * a - 0.004 * b + 0.0003 * a * b
        q["phi"] = (3.06 if kind == "sphere" else 2.9) + 0.021 * a + 0.013 * b - 0.0002 * a * a
        q["steps"] = 100 + ix
        q["status"] = RLIM_OR_DEST
        q["rdot_flips"] = 1
        q["equatorial_crossings"] = (ix + 2 * iy) % 4
        q["t"], q["k"], q["emit"], q["redshift"] = 5.0, 1.0, 0.5, 0.25        # never read
    c = rays[:, :, 0]
    pick = rng.random((nx, ny)) if sprinkle else np.ones((nx, ny))
    c["steps"][pick < 0.04] = 0
    c["steps"][(pick >= 0.04) & (pick < 0.07)] = -7
    c["status"][(pick >= 0.07) & (pick < 0.11)] = capi.STATUS_HORIZON
    c["status"][(pick >= 0.11) & (pick < 0.14)] = capi.STATUS_STEPLIM | RLIM_OR_DEST
    c["status"][(pick >= 0.14) & (pick < 0.16)] = capi.STATUS_STEPLIM | capi.STATUS_HORIZON
    wound = (pick >= 0.16) & (pick < 0.22)
    for m in range(rpb):                                                  # a whole bundle on another winding: another ORDER, still a hit
        rays[:, :, m]["phi"][wound] += 2 * math.pi * 3
    c["rdot_flips"][(pick >= 0.22) & (pick < 0.25)] = 5
    c["phi"][(pick >= 0.25) & (pick < 0.27)] *= -1
    if bundles and sprinkle:
        spick = rng.random((nx, ny))
        sat = rng.integers(1, 5, size=(nx, ny))
        for m in range(1, 5):
            q, mine = rays[:, :, m], sat == m
            q["rdot_flips"][mine & (spick < 0.08)] += 2                                   # another rdot_flips -> SENTINEL
            q["phi"][mine & (spick >= 0.08) & (spick < 0.16)] += 1.6                      # more than pi / 2 away -> SENTINEL
            q["phi"][mine & (spick >= 0.16) & (spick < 0.20)] -= 1.5                      # within pi / 2: a (large) determinant
            q["status"][mine & (spick >= 0.20) & (spick < 0.26)] = capi.STATUS_RLIM       # no DEST: the satellite missed -> NaN
            q["steps"][mine & (spick >= 0.26) & (spick < 0.30)] = 0
    out = rays.reshape(-1)
    if trailing:
        tail = np.zeros(trailing, dtype=capi.RAY_F64)
        tail["r"], tail["theta"], tail["phi"], tail["status"], tail["steps"] = 900.0, 1.2, 0.4, RLIM_OR_DEST, -1
        out = np.concatenate([out, tail])
    return out
