"""CPU: the class mirror HealpixPointSource<double> (raytrace_cpu_amd/host/raytracer/healpix_pointsource.h) against the numpy rule.

A small dump program of this test's own is compiled against raytrace_cpu_amd/host/ (one g++ line below); it builds the source at order 2 for each
of the three tetrads -- its constructor runs on the host, no GPU is asked for -- and writes rays[] and the pixel vectors the mirror computed, then
rays[] after redshift_start() (the moving source only: that one is host code) and after set_disc_source().  The
vectors must be the reference's (tests/golden/healpix_vectors.npz, within the geometry bound of tests/test_healpix_rules.py), and k, h, Q, both
signs and every other field must equal the rule fed with the mirror's own vectors, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import healpix_rules as hr
import oracle_lib as ol
from raytrace_cpu_amd import api, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "raytrace_cpu_amd", "host")
CSRC = os.path.join(ROOT, "raytrace_cpu_amd", "csrc")

DUMP = r"""
#include <cstdio>
#include <cstdlib>
#include "raytracer/healpix_pointsource.h"
int main(int argc, char** argv)
{
    double pos[4] = {atof(argv[1]), atof(argv[2]), atof(argv[3]), atof(argv[4])};
    const double V = atof(argv[5]), spin = atof(argv[6]);
    const int order = atoi(argv[7]), motion = atoi(argv[8]), basis = atoi(argv[9]);
    HealpixPointSource<double> src(pos, V, spin, order, motion, basis);
    FILE* f = fopen(argv[10], "wb");
    fwrite(src.rays, sizeof(Ray<double>), src.get_count(), f);
    fclose(f);
    f = fopen(argv[11], "wb");
    for (int pix = 0; pix < src.get_num_pix(); pix++) {
        double v[15];
        krhost_healpix::pixel_vectors<double>(order, pix, v, v + 12);
        fwrite(v, sizeof v, 1, f);
    }
    fclose(f);
    try { HealpixPointSource<double> bad(pos, V, spin, order, 1, 1); return 3; } catch (const std::invalid_argument&) {}
    if (motion == 1) {                      // the moving source's redshift_start is host code; the orbiting one's is the base class's device pass
        src.redshift_start();
        f = fopen(argv[12], "wb");
        fwrite(src.rays, sizeof(Ray<double>), src.get_count(), f);
        fclose(f);
    }
    src.set_disc_source();
    f = fopen(argv[13], "wb");
    fwrite(src.rays, sizeof(Ray<double>), src.get_count(), f);
    fclose(f);
    return src.get_count() == 5 * src.get_num_pix() ? 0 : 4;
}
"""

TETRADS = [("orbital-basis-0", (0.0, 5.0, 1e-3, 1.5707), 0.0, 0.998, 0, 0),
           ("orbital-basis-1", (0.0, 6.0, 1.2, 1.5707), 0.06411, 0.9, 0, 1),
           ("radial", (0.0, 5.0, 1e-3, 1.5707), 0.3, 0.998, 1, 0)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    d = tmp_path_factory.mktemp("healpix_mirror")
    src, exe = d / "dump.cpp", d / "dump"
    src.write_text(DUMP)
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fopenmp", "-Wall", "-Wno-unused-parameter", "-I" + HOST, "-o", str(exe), str(src),
                    "-L" + HOST, "-lkr_host", "-L" + CSRC, "-lkrtrace", "-Wl,-rpath," + HOST, "-Wl,-rpath," + CSRC], check=True)
    return exe, d


@pytest.mark.parametrize("case,pos,V,spin,motion,basis", TETRADS, ids=[t[0] for t in TETRADS])
def test_constructor_equals_rule(dump, case, pos, V, spin, motion, basis):
    exe, d = dump
    rays_file, vec_file, emit_file, disc_file = d / f"{case}.rays", d / f"{case}.vec", d / f"{case}.emit", d / f"{case}.disc"
    subprocess.run([str(exe)] + [repr(float(x)) for x in pos] + [repr(V), repr(spin), "2", str(motion), str(basis), str(rays_file), str(vec_file), str(emit_file),
                                                                 str(disc_file)], check=True, timeout=120)
    rays = np.fromfile(rays_file, dtype=capi.RAY_F64)
    vec = np.fromfile(vec_file, dtype=np.float64).reshape(-1, 15)
    assert len(rays) == 5 * 192 and vec.shape == (192, 15)
    z = np.load(os.path.join(ROOT, "tests", "golden", "healpix_vectors.npz"))
    want_vec = z["bits"].view(np.float64)[z["order"] == 2]
    assert np.abs(vec - want_vec).max() <= 4.5e-16
    spec = api.healpix_spec(pos, V, spin, 2, motion, basis, rays_per_pixel=5)
    v = hr.source_vectors(spec, vec)
    want = hr.records(spec, v, beta=rays["beta"])
    bad = ol.rays_equal_bitwise(rays, want)
    assert not bad, bad
    assert np.abs(rays["beta"] - np.arctan2(v[:, 1], v[:, 0])).max() <= 4.5e-16
    assert (rays["steps"] == 0).all() and (rays["emit"] == 0).all()
    after = rays
    if motion == 1:
        # redshift_start() of the moving source: p . u = E = 1 in its own frame on every ray, the un-normalised centres included, and nothing else moves
        after = np.fromfile(emit_file, dtype=capi.RAY_F64)
        worst = float(np.abs(after["emit"] - 1).max())
        print(f"mirror, radial motion: worst |emit - 1| = {worst:.3e}")
        assert worst <= 1e-12
        assert not ol.rays_equal_bitwise(after, rays, fields=[f for f in rays.dtype.names if f != "emit"])
    # set_disc_source(): the rays that start into the disc become unused slots, nothing else changes
    disc = np.fromfile(disc_file, dtype=capi.RAY_F64)
    assert np.array_equal(disc["steps"], np.where(rays["thetadot_sign"] > 0, -1, 0)) and 0 < (disc["steps"] == -1).sum() < len(disc)
    assert not ol.rays_equal_bitwise(disc, after, fields=[f for f in rays.dtype.names if f != "steps"])
