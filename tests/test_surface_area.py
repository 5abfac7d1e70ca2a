"""CPU: api.surface_area / api.surface_area_density, the proper area of the rings of a disc surface z = H(rho) for the orbiting gas, against the
project's disc-area function (host/include/disc.h: integrate_disc_area, and integrate_surface_area, which the kr_emissivity program divides by) and
against flat space."""
import math
import os
import subprocess

import numpy as np
import pytest

from raytrace_cpu_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPIN = 0.5

AREA_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "include/disc.h"
int main(int argc, char** argv)
{
    const double a = atof(argv[1]), slope = atof(argv[2]), scale = atof(argv[3]);
    const double r_in = kerr_isco<double>(a, +1);
    printf("%a\n", r_in);
    for (int i = 4; i + 1 < argc; i++) {
        const double lo = strtod(argv[i], nullptr), hi = strtod(argv[i + 1], nullptr);
        printf("%a %a %a\n", integrate_disc_area<double>(lo, hi, a), integrate_disc_area<double>(lo, hi, a, true), integrate_surface_area<double>(lo, hi, r_in, slope, scale, a));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def area_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("surface_area")
    src, exe = d / "area.cpp", d / "area"
    src.write_text(AREA_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-I" + os.path.join(ROOT, "raytrace_cpu_amd", "host"), "-o", str(exe), str(src)], check=True)
    return str(exe)


def host_areas(exe, slope, scale, edges):
    r = subprocess.run([exe, repr(SPIN), repr(slope), repr(scale)] + [float(e).hex() for e in edges], capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.split("\n")
    return float.fromhex(lines[0]), np.array([[float.fromhex(x) for x in line.split()] for line in lines[1:] if line])


# Both sides add up the same <= 50 positive pieces (the same running product rho_k = rho_{k-1} step, the same step from the C library's exp / log),
# and a piece is a chain of some 40-100 correctly rounded + - x / sqrt on well-conditioned quantities -- from the ISCO outwards Delta = r^2 - 2 r + a^2
# and 1 - (Omega - omega)^2 e2psi / e2nu lose at most two bits to cancellation -- plus sin, cos, atan2 within an ulp: 100 operations x 1.1e-16 x 4
# is 5e-14 per piece, a sum of positive terms keeps the relative error of its terms and adds 50 x 1.1e-16.  1e-12 leaves a factor of twenty.
RTOL = 1e-12


def test_zero_thickness_is_the_disc_area_function(area_program):
    """slope = scale = 0 from the ISCO outwards, in the bins of the emissivity program (30 logarithmic bins to 500) and in three wide rings: the
    areas integrate_disc_area gives -- with circular orbits everywhere, and as the program calls it (the plunge region starts below these rings)."""
    r_in, _ = host_areas(area_program, 0.0, 0.0, [])
    for edges in (r_in * (500.0 / r_in) ** (np.arange(31) / 30.0), np.array([r_in, 10.0, 100.0, 1000.0])):
        _, want = host_areas(area_program, 0.0, 0.0, edges)
        got = api.surface_area(edges, r_in, 0.0, 0.0, SPIN)
        assert got.shape == (len(edges) - 1,) and (got > 0).all()
        for col, name in ((0, "integrate_disc_area"), (1, "integrate_disc_area(force_keplerian)"), (2, "integrate_surface_area")):
            rel = np.abs(got - want[:, col]) / want[:, col]
            assert rel.max() <= RTOL, (name, float(rel.max()))


@pytest.mark.parametrize("slope,scale", [(0.05, 1.0), (0.1, 0.0), (0.0, 2.0)])
def test_python_and_host_rules_agree_on_a_surface(area_program, slope, scale):
    """api.surface_area == integrate_surface_area (what kr_emissivity divides by) on the surfaces of the fixtures."""
    r_in, _ = host_areas(area_program, 0.0, 0.0, [])
    edges = r_in * (400.0 / r_in) ** (np.arange(26) / 25.0)
    _, want = host_areas(area_program, slope, scale, edges)
    got = api.surface_area(edges, r_in, slope, scale, SPIN)
    assert (np.abs(got - want[:, 2]) / want[:, 2]).max() <= RTOL
    flat = api.surface_area(edges, r_in, 0.0, 0.0, SPIN)
    assert (np.abs(got / flat - 1) < 0.2).all() and (got != flat).all()              # (the surfaces of the fixtures are thin: a tilt of at most 0.3)


def test_cone_tends_to_flat_space():
    """Far out the area of a cone z = s rho per unit rho and phi tends to rho sqrt(1 + s^2).  The leading corrections are all of first order in 1 / rho
    and positive: sqrt(Sigma / Delta) = 1 + 1 / r + O(r^-2) along the generator (whose tangent has no theta component on a cone), the Lorentz factor of
    the orbit, v^2 = 1 / rho, is 1 + 1 / (2 rho), and sqrt(e2psi) = rho (1 + O(a^2 / r^2)).  With r >= rho their sum is at most 1.5 / rho; the second-order
    terms are a few rho^-2, below 1e-3 of that beyond rho = 1e4.  So the ratio lies in (1, 1 + 2 / rho)."""
    rho = np.exp(np.linspace(math.log(1e4), math.log(1e7), 40))
    for s in (0.0, 0.1, 0.5):
        ratio = api.surface_area_density(rho, 4.233, s, 0.0, SPIN) / (rho * math.sqrt(1 + s * s))
        assert (ratio > 1).all() and (ratio - 1 < 2 / rho).all(), (s, float((ratio - 1).max()))
    # the ring itself, over the whole circle: the rule takes a sub-ring at its inner edge, which for an integrand proportional to rho falls short of
    # pi sqrt(1 + s^2) (hi^2 - lo^2) by the factor 2 / (step + 1) exactly, step = (hi / lo)^(1 / 49), when the running product ends the loop after 49 pieces
    lo, hi, s = 2e4, 2.2e4, 0.1
    step = math.exp(math.log(hi / lo) / 49)
    subs, x = 0, lo
    while x < hi:
        subs, x = subs + 1, x * step
    got = api.surface_area([lo, hi], 4.233, s, 0.0, SPIN, dphi=2 * math.pi)[0]
    want = math.pi * math.sqrt(1 + s * s) * (lo * lo * step ** (2 * subs) - lo * lo) * 2 / (step + 1)
    assert 0 < got / want - 1 < 2 / lo
