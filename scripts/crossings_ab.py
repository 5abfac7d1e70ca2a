"""What recording the equatorial crossings costs: kernel_ms of kr_trace_crossings_dev_f64 (M = 4, stop_when_full 0 and 1) against kernel_ms of
kr_trace_dev_f64(flags = 0) -- the strict trace, existing code: the baseline -- on the same device-built rays and parameters, all free-running
(theta_max = 0) under ONE step limit, Euler and RK4:

  lamp a=0.998   ~1e6 rays of the ps_h10 lamp post (source (0, 10, 1e-3, 1.5707), dcosalpha = dbeta), r_max = 100
  lamp a=0.5     the same source at a = 0.5
  plane 80 deg   a 1025 x 1025 image plane at 80 degrees (dist 10000, +-30, a = 0.998), r_max = 11000

and, beside them, the path recorder's record pass on the same rays with a write_step no ray reaches (no rows: what the shared loop costs with the
lightest recorder on it).  One library per process (KRTRACE_LIB picks an experiment build, scripts/ab_kernels.py):

  python scripts/crossings_ab.py [--rays 1e6] [--plane 1025] [--steplim 100000] [--repeats 3]

Every figure: one warm-up, then the median and the best of --repeats launches on freshly built rays; longest_ray_steps of each.  Prints one JSON object.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytrace_cpu_amd import api, capi  # noqa: E402

vp = C.c_void_p
M = 4


def lamp(spin, rays):
    s = capi.PointSourceSpec()
    for i, v in enumerate((0.0, 10.0, 1e-3, 1.5707)):
        s.pos[i] = v
    d = math.sqrt(1.99 * 2 * math.pi / rays)
    s.V, s.spin, s.tol, s.E = 0.0, spin, 100.0, 1.0
    s.cosalpha0, s.cosalphamax, s.dcosalpha = -0.995, 0.995, d
    s.beta0, s.betamax, s.dbeta = -math.pi, math.pi, d
    return s


def plane(n_side):
    s = capi.ImagePlaneSpec()
    s.dist, s.inc_deg, s.x0, s.xmax, s.y0, s.ymax = 10000.0, 80.0, -30.0, 30.0, -30.0, 30.0
    s.dx = s.dy = 60.0 / (n_side - 1)
    s.spin, s.phi0, s.precision = 0.998, 0.0, 100.0
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=1e6)
    ap.add_argument("--plane", type=int, default=1025)
    ap.add_argument("--steplim", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    L = capi.load()
    workloads = []
    for spin in (0.998, 0.5):
        s = lamp(spin, args.rays)
        workloads.append((f"lamp a={spin}", L.kr_pointsource_count(C.byref(s), None, None), spin, 100.0, 0,
                          lambda d, n, s=s: L.kr_pointsource_init_emit_dev_f64(C.byref(s), 0, 1, 0.0, 0, 0, d, n, None)))
    ip = plane(args.plane)
    workloads.append((f"plane 80 deg {args.plane}^2", L.kr_imageplane_count(C.byref(ip), None, None), -0.998, 11000.0, 1,
                      lambda d, n: L.kr_imageplane_init_emit_dev_f64(C.byref(ip), 0, 1, 0.0, 1, 0, d, n, None)))
    n_max = max(w[1] for w in workloads)
    res = {"library": os.environ.get("KRTRACE_LIB", capi.LIB_PATH), "max_crossings": M, "steplim": args.steplim, "repeats": args.repeats, "runs": []}
    d_rays, d_rows, d_seen, d_off = vp(), vp(), vp(), vp()
    try:
        capi.check(L, L.kr_malloc(C.byref(d_rays), n_max * 144), "kr_malloc")
        capi.check(L, L.kr_malloc(C.byref(d_rows), n_max * M * 32), "kr_malloc")
        capi.check(L, L.kr_malloc(C.byref(d_seen), n_max * 4), "kr_malloc")
        capi.check(L, L.kr_malloc(C.byref(d_off), (n_max + 1) * 8), "kr_malloc")
        for name, n, spin, r_max, reverse, init in workloads:
            def timed(launch, prepare=None):
                ms, st = [], capi.Stats()
                for _ in range(args.repeats + 1):
                    capi.check(L, init(d_rays, n), "init")
                    if prepare:
                        prepare()
                    capi.check(L, L.kr_synchronize(None), "sync")
                    capi.check(L, launch(st), "launch")
                    ms.append(st.kernel_ms)
                return {"median_ms": statistics.median(ms[1:]), "best_ms": min(ms[1:]), "steps": int(st.steps_total), "rays_traced": int(st.rays_traced),
                        "longest_ray_steps": int(st.longest_ray_steps)}

            for integ, iname in ((capi.EULER, "euler"), (capi.RK4, "rk4")):
                p = capi.copy_params(capi.default_params(spin), integrator=integ, flags=0, r_max=r_max, theta_max=0.0, steplim=args.steplim)
                row = {"workload": name, "rays": int(n), "integrator": iname,
                       "trace_flags0": timed(lambda st: L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)))}
                for stop in (0, 1):
                    spec = api.crossing_spec(M, bool(stop), V=-1.0, reverse=reverse)
                    t = timed(lambda st: L.kr_trace_crossings_dev_f64(C.byref(p), C.byref(spec), d_rays, n, d_rows, d_seen, None, C.byref(st)))
                    seen = (C.c_int32 * n)()
                    capi.check(L, L.kr_memcpy_d2h(seen, d_seen, 4 * n), "d2h")
                    hist = np.bincount(np.frombuffer(seen, dtype=np.int32))
                    t.update(rays_by_crossings=hist[:8].tolist() + ([int(hist[8:].sum())] if len(hist) > 8 else []), ratio_to_trace=t["median_ms"] / row["trace_flags0"]["median_ms"])
                    row[f"crossings stop_when_full={stop}"] = t
                w = api.path_spec(write_step=1 << 30)
                total = C.c_int64()

                def count():
                    capi.check(L, L.kr_trace_paths_count_dev_f64(C.byref(p), C.byref(w), d_rays, n, d_off, None, C.byref(total), None), "count")
                t = timed(lambda st: L.kr_trace_paths_record_dev_f64(C.byref(p), C.byref(w), d_rays, n, d_off, d_rows, max(total.value, 0), None, C.byref(st)), prepare=count)
                t.update(rows=int(total.value), ratio_to_trace=t["median_ms"] / row["trace_flags0"]["median_ms"])
                row["paths record pass, no rows"] = t
                res["runs"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        print(json.dumps(res, indent=1))
    finally:
        L.kr_synchronize(None)
        for dptr in (d_rays, d_rows, d_seen, d_off):
            if dptr.value:
                L.kr_free(dptr)


if __name__ == "__main__":
    main()
