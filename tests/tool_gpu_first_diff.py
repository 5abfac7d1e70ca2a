#!/usr/bin/env python3
"""GPU tool (not a pytest file), the f64 sibling of tests/tool_gpu_f32_first_diff.py: where does a strict (flags = 0) trace first leave the correctly
rounded oracle (oracle/libkr_oracle_cr.so)?  Both sides trace the same records with steplim = 1, 2, 3, ... ; for the rays that end up different the
first step and the fields that differ there are reported, with the record both sides agreed on one step earlier -- the operands of that step, ready
for kr_debug_arith_f64 (ops 4 / 5: kr_sincos_f64, 22-25: kr_crmath.hpp, 1 / 3: the lean quotient and root).

usage: tool_gpu_first_diff.py CASE RUN [MAX_RAYS]      e.g.  tool_gpu_first_diff.py ip15 rk4_plane"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import exact_parity_cases as xp  # noqa: E402
import oracle_lib as ol  # noqa: E402
from raytrace_cpu_amd import api, capi  # noqa: E402

FIELDS = ("t", "r", "theta", "phi", "pt", "pr", "ptheta", "pphi", "steps", "status", "rdot_sign", "thetadot_sign", "rdot_flips", "equatorial_crossings")


def differing_fields(got, want, i):
    return [f for f in FIELDS if not (got[f][i] == want[f][i] or (got[f][i] != got[f][i] and want[f][i] != want[f][i]))]


def main():
    case_name, run = sys.argv[1], sys.argv[2]
    max_rays = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    p = capi.copy_params(xp.cases()[case_name]["runs"][run], flags=0)
    init = xp.init(case_name)
    want, _ = ol.oracle_trace(p, init, cr=True)
    got, _ = api.trace(p, init)
    _, differ = xp.bit_identical_share(got, want)
    print(f"{case_name}-{run}: {int(differ.sum())} of {int((want['steps'] != -1).sum())} rays differ from the correctly rounded oracle")
    for i in np.flatnonzero(differ)[:max_rays]:
        one = init[i:i + 1]
        n = abs(int(want["steps"][i]))
        lo, hi = 0, n          # bisection on the step limit: equal after lo steps, different after hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            q = capi.copy_params(p, steplim=mid)
            g, w = api.trace(q, one)[0], ol.oracle_trace(q, one, cr=True)[0]
            if differing_fields(g, w, 0):
                hi = mid
            else:
                lo = mid
        q = capi.copy_params(p, steplim=hi)
        g, w = api.trace(q, one)[0], ol.oracle_trace(q, one, cr=True)[0]
        print(f"ray {i}: {n} steps; first differs after step {hi}: " + "; ".join(f"{f} {g[f][0]!r} / {w[f][0]!r}" for f in differing_fields(g, w, 0)))
        if lo > 0:
            b = ol.oracle_trace(capi.copy_params(p, steplim=lo), one, cr=True)[0]
            print(f"   record after step {lo} (both sides): " + ", ".join(f"{f} {b[f][0]!r}" for f in FIELDS) + f" | k {one['k'][0]!r} h {one['h'][0]!r} Q {one['Q'][0]!r}")
            print("   (a call's turning-point latches start afresh: a ray stored on a turning point may differ from its uninterrupted trace on BOTH sides alike)")


if __name__ == "__main__":
    main()
