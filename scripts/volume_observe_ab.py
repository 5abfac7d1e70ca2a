"""What observing a volume map costs: kernel_ms of kr_trace_observe_dev_f64 on the rays of a camera at 60 degrees, 1e4 rg away, |x|, |y| <= 50 rg
(a = 0.998, the mirrored spin of an ImagePlane, rays run to 1.5 dist), at three sizes of rays / grid / bins

  small    256 x 256 rays,   100 x 50 x 1 logarithmic grid over r in [1.2, 100],  64 energy bins, no response
  medium   512 x 512 rays,   64 x 32 x 64 linear grid,                            256 energy x 64 time bins
  large    1024 x 1024 rays, 100 x 50 x 1 logarithmic grid,                       1024 energy x 256 time bins

with synthetic fields from the cell index (emis = 1 / (1 + cell % 7), zero in every fifth cell; kappa = 0.05 (cell % 3); delay = 0.1 cell), against
kernel_ms of kr_trace_dev_f64(flags = 0) on the same rays.  One library per process (KRTRACE_LIB picks an experiment build, scripts/ab_kernels.py:
-DKR_OBSERVE_ACC=0 is the plain accumulation, -DKR_OBSERVE_RK4_WAVES=2 another register budget):

  python scripts/volume_observe_ab.py                      the library's observing launches and its own strict trace
  python scripts/volume_observe_ab.py --baseline           the strict trace only (a library of a commit without the observer: the parent's)

Every figure: one warm-up, then the median and the best of --repeats launches on freshly built rays.  Prints one JSON object.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytrace_cpu_amd import capi  # noqa: E402

SPIN, DIST = 0.998, 10000.0
vp = C.c_void_p
SIZES = {"small": (256, (100, 50, 1, True), 64, 0), "medium": (512, (64, 32, 64, False), 256, 64), "large": (1024, (100, 50, 1, True), 1024, 256)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--sizes", default="small,medium,large")
    args = ap.parse_args()
    if args.baseline:
        for name in ("kr_trace_observe_dev_f64", "kr_trace_observe_f64"):
            capi.PROTOTYPES.pop(name, None)
    L = capi.load()
    res = {"library": os.environ.get("KRTRACE_LIB", capi.LIB_PATH), "repeats": args.repeats, "runs": []}
    for size in args.sizes.split(","):
        nx, (nr, ntheta, nphi, logbin), nen, nt = SIZES[size]
        s = capi.ImagePlaneSpec()
        s.dist, s.inc_deg, s.x0, s.xmax, s.y0, s.ymax, s.spin, s.phi0, s.precision = DIST, 60.0, -50.0, 50.0, -50.0, 50.0, SPIN, 0.0, 100.0
        s.dx = s.dy = 100.0 / nx          # (a power of two: the quotient is exact, nx + 1 rays a side)
        n = L.kr_imageplane_count(C.byref(s), None, None)
        ncell = nr * ntheta * nphi
        words = 2 * nen + nen * nt + 6
        bufs = {k: vp() for k in ("rays", "out", "image", "emis", "kappa", "delay")}
        try:
            for k, nbytes in (("rays", n * 144), ("out", words * 8), ("image", n * 8), ("emis", ncell * 8), ("kappa", ncell * 8), ("delay", ncell * 8)):
                capi.check(L, L.kr_malloc(C.byref(bufs[k]), nbytes), "kr_malloc")
            cell = np.arange(ncell)
            emis = 1.0 / (1 + cell % 7)
            emis[::5] = 0.0
            for k, a in (("emis", emis), ("kappa", 0.05 * (cell % 3)), ("delay", 0.1 * cell)):
                a = np.ascontiguousarray(a, dtype=np.float64)
                capi.check(L, L.kr_memcpy_h2d(bufs[k], a.ctypes.data_as(vp), a.nbytes), "h2d")

            def timed(launch):
                ms, st = [], capi.Stats()
                for _ in range(args.repeats + 1):
                    capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(s), 0, 1, 0.0, 1, 0, bufs["rays"], n, None), "init")
                    capi.check(L, L.kr_memset(bufs["out"], 0, words * 8), "kr_memset")
                    capi.check(L, L.kr_synchronize(None), "sync")
                    capi.check(L, launch(st), "launch")
                    ms.append(st.kernel_ms)
                return {"median_ms": statistics.median(ms[1:]), "best_ms": min(ms[1:]), "steps": int(st.steps_total), "rays_traced": int(st.rays_traced)}

            for integ, name in ((capi.EULER, "euler"), (capi.RK4, "rk4")):
                p = capi.default_params(-SPIN)
                p.integrator, p.flags, p.r_max = integ, 0, 1.5 * DIST
                row = {"size": size, "rays": int(n), "grid": [nr, ntheta, nphi], "nen": nen, "nt": nt, "integrator": name,
                       "trace_flags0": timed(lambda st: L.kr_trace_dev_f64(C.byref(p), bufs["rays"], n, None, C.byref(st)))}
                if not args.baseline:
                    from raytrace_cpu_amd import api
                    m = api.volume_map_struct(1.2, 100.0, nr, ntheta, nphi, logbin, reverse=1)
                    b = api.observe_bins_struct(0.05, 1.85, nen, t0=DIST - 150.0, tmax=DIST + 250.0, nt=nt)
                    for label, kappa, image in (("observe thin", None, bufs["image"]), ("observe absorbing", bufs["kappa"], bufs["image"])):
                        t = timed(lambda st: L.kr_trace_observe_dev_f64(C.byref(p), C.byref(m), C.byref(b), bufs["emis"], kappa, bufs["delay"], bufs["rays"], n,
                                                                        bufs["out"], image, None, C.byref(st)))
                        tail = (C.c_double * 6)()
                        capi.check(L, L.kr_memcpy_d2h(tail, vp(bufs["out"].value + 8 * (words - 6)), 48), "d2h")
                        t.update({k: int(tail[q]) for q, k in enumerate(api.OBSERVE_TALLIES)})
                        row[label] = t
                res["runs"].append(row)
        finally:
            L.kr_synchronize(None)
            for d in bufs.values():
                if d.value:
                    L.kr_free(d)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
