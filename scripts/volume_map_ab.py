"""What mapping costs: kernel_ms of kr_trace_volume_dev_f64 on a ~1e6-ray lamp post (the ps_h10 geometry: source (0, 10, 1e-3, 1.5707), a = 0.998,
dcosalpha = dbeta) in passage and every-row mode, for a 100 x 50 x 1 logarithmic and a 64 x 32 x 64 linear grid over r in [1.2, 100], against
kernel_ms of kr_trace_dev_f64(flags = 0) on the same rays.  One library per process (KRTRACE_LIB picks an experiment build, scripts/ab_kernels.py):

  python scripts/volume_map_ab.py                      the library's map launches and its own strict trace
  python scripts/volume_map_ab.py --baseline           the strict trace only (a library of a commit without the map: the parent's)

Every figure: one warm-up, then the median and the best of --repeats launches on freshly built rays.  Prints one JSON object.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytrace_cpu_amd import capi  # noqa: E402

SPIN = 0.998
vp = C.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=1e6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()
    if args.baseline:
        for name in ("kr_trace_volume_dev_f64", "kr_trace_volume_f64"):
            capi.PROTOTYPES.pop(name, None)
    L = capi.load()
    s = capi.PointSourceSpec()
    for i, v in enumerate((0.0, 10.0, 1e-3, 1.5707)):
        s.pos[i] = v
    d = math.sqrt(1.99 * 2 * math.pi / args.rays)
    s.V, s.spin, s.tol, s.E = 0.0, SPIN, 100.0, 1.0
    s.cosalpha0, s.cosalphamax, s.dcosalpha = -0.995, 0.995, d
    s.beta0, s.betamax, s.dbeta = -math.pi, math.pi, d
    n = L.kr_pointsource_count(C.byref(s), None, None)
    d_rays, d_map = vp(), vp()
    res = {"library": os.environ.get("KRTRACE_LIB", capi.LIB_PATH), "rays": int(n), "dcosalpha_dbeta": d, "repeats": args.repeats, "runs": []}
    grids = {}
    if not args.baseline:
        from raytrace_cpu_amd import api
        grids = {"log 100x50x1": api.volume_map_struct(1.2, 100.0, 100, 50, 1, True), "linear 64x32x64": api.volume_map_struct(1.2, 100.0, 64, 32, 64, False)}
    words = max([3 * m.nr * m.ntheta * m.nphi + 4 for m in grids.values()] + [4])
    try:
        capi.check(L, L.kr_malloc(C.byref(d_rays), n * 144), "kr_malloc")
        capi.check(L, L.kr_malloc(C.byref(d_map), words * 8), "kr_malloc")

        def timed(launch):
            ms, st = [], capi.Stats()
            for _ in range(args.repeats + 1):
                capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(s), 0, 1, 0.0, 0, 0, d_rays, n, None), "init")
                capi.check(L, L.kr_memset(d_map, 0, words * 8), "kr_memset")
                capi.check(L, L.kr_synchronize(None), "sync")
                capi.check(L, launch(st), "launch")
                ms.append(st.kernel_ms)
            return {"median_ms": statistics.median(ms[1:]), "best_ms": min(ms[1:]), "steps": int(st.steps_total), "rays_traced": int(st.rays_traced)}

        for integ, name in ((capi.EULER, "euler"), (capi.RK4, "rk4")):
            p = capi.default_params(SPIN)
            p.integrator, p.flags = integ, 0
            row = {"integrator": name, "trace_flags0": timed(lambda st: L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)))}
            for gname, m in grids.items():
                for mode in (0, 1):
                    m.mode = mode
                    t = timed(lambda st: L.kr_trace_volume_dev_f64(C.byref(p), C.byref(m), d_rays, n, d_map, None, C.byref(st)))
                    tail = (C.c_double * 4)()
                    ncell = m.nr * m.ntheta * m.nphi
                    capi.check(L, L.kr_memcpy_d2h(tail, vp(d_map.value + 24 * ncell), 32), "d2h")
                    t.update(rows=int(tail[0]), in_grid=int(tail[1]), deposits=int(tail[2]), bad_g=int(tail[3]))
                    row[f"map {gname} {'every row' if mode else 'passage'}"] = t
            res["runs"].append(row)
        print(json.dumps(res, indent=1))
    finally:
        L.kr_synchronize(None)
        for dptr in (d_rays, d_map):
            if dptr.value:
                L.kr_free(dptr)


if __name__ == "__main__":
    main()
