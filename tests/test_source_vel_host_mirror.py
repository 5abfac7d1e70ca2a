"""CPU: the class mirror PointSourceVel<double> (raytrace_cpu_amd/host/raytracer/pointsource_vel.h) against the numpy rule.

A small dump program of this test's own is compiled against raytrace_cpu_amd/host/; it builds the source for each of the four emitters -- its
constructor runs on the host, no GPU is asked for -- and writes rays[], its tetrad and rays[] after redshift_start() (host code too).  The tetrad
must equal the rule bit for bit (the same csrc/kr_vel_tetrad.hpp the device source uses).  The mirror's acos / sin / cos are the C library's, the
rule's are correctly rounded, so k, h, Q are held to MIRROR_RTOL of the source's largest |k|, |h|, |Q| -- the bar tests/test_source_vel_rules.py
measured for two restatements that differ only in such last bits (RADIAL) -- and everything else bit for bit; emit is E within EMIT_ULP."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import source_vel_rules as sv
from raytrace_cpu_amd import capi
from test_source_vel_rules import EMIT_ULP, RADIAL as MIRROR_RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "raytrace_cpu_amd", "host")
CSRC = os.path.join(ROOT, "raytrace_cpu_amd", "csrc")

DUMP = r"""
#include <cstdio>
#include <cstdlib>
#include "raytracer/pointsource_vel.h"
int main(int argc, char** argv)
{
    double pos[4], u[4];
    for (int i = 0; i < 4; i++) { pos[i] = atof(argv[1 + i]); u[i] = atof(argv[5 + i]); }
    const double spin = atof(argv[9]), E = atof(argv[10]);
    PointSourceVel<double> src(pos, u, spin, TOL, 0.06, 0.18, -0.995, 0.995, -1 * M_PI, M_PI, E);
    FILE* f = fopen(argv[11], "wb");
    fwrite(src.rays, sizeof(Ray<double>), src.get_count(), f);
    fwrite(src.tetrad(), sizeof(double), 16, f);
    src.redshift_start();
    fwrite(src.rays, sizeof(Ray<double>), src.get_count(), f);
    fclose(f);
    double bad[4] = {1.0, 1.5, 0.0, 0.0};
    try { PointSourceVel<double> no(pos, bad, spin, TOL, 0.06, 0.18); return 3; } catch (const std::invalid_argument&) {}
    return 0;
}
"""


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    d = tmp_path_factory.mktemp("vel_mirror")
    src, exe = d / "dump.cpp", d / "dump"
    src.write_text(DUMP)
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fopenmp", "-Wall", "-Wno-unused-parameter", "-I" + HOST, "-o", str(exe), str(src),
                    "-L" + HOST, "-lkr_host", "-L" + CSRC, "-lkrtrace", "-Wl,-rpath," + HOST, "-Wl,-rpath," + CSRC], check=True)
    return exe, d


@pytest.mark.parametrize("name", sv.EMITTERS)
def test_constructor_and_redshift_start_equal_the_rule(dump, name):
    exe, d = dump
    E = 2.5
    spec = sv.spec_of(name, E=E)
    out = d / f"{name}.bin"
    subprocess.run([str(exe)] + [repr(float(x)) for x in list(spec.pos) + list(spec.u) + [spec.spin, E]] + [str(out)], check=True, timeout=120)
    raw = out.read_bytes()
    n = sv.grid(spec)[0]
    size = n * capi.RAY_F64.itemsize
    assert len(raw) == 2 * size + 128
    rays = np.frombuffer(raw[:size], dtype=capi.RAY_F64)
    tetrad = np.frombuffer(raw[size:size + 128], dtype=np.float64).reshape(4, 4)
    after = np.frombuffer(raw[size + 128:], dtype=capi.RAY_F64)
    want = sv.records(spec, emit=True)
    assert np.array_equal(tetrad.view(np.int64), np.ascontiguousarray(sv.tetrad(spec.pos, spec.u, spec.spin)["tetrad"]).view(np.int64))
    exact = [f for f in capi.RAY_F64.names if f not in ("k", "h", "Q", "emit", "redshift", "status", "rdot_flips", "equatorial_crossings")]
    live = want["steps"] == 0
    assert np.array_equal(rays["steps"] == 0, live) and (rays["steps"][~live] == -1).all()
    assert not ol.rays_equal_bitwise(rays[live], want[live], fields=exact)
    for f in ("k", "h", "Q"):
        assert np.abs(rays[f][live] - want[f][live]).max() <= MIRROR_RTOL * np.abs(want[f][live]).max(), f
    assert (rays["emit"][live] == 0).all()
    L = sv.launched(spec)
    scale = sv.dot(L["frame"]["g"], L["frame"]["un"], [x[live] for x in L["p"]])[1]
    assert (np.abs(after["emit"][live] - E) <= EMIT_ULP * sv.EPS * scale).all()
    assert not ol.rays_equal_bitwise(after[live], rays[live], fields=[f for f in capi.RAY_F64.names if f != "emit"])
