"""Timing of the HEALPix point source and its fate pass next to the existing yardsticks, on one GPU (profiles/healpix_ab.txt):

  init    kr_healpix_init_emit_dev_f64 at order 10 with 1 ray per pixel (12 582 912 records) and at order 9 with 5 rays per pixel (15 728 640),
          against kr_pointsource_init_emit_dev_f64 at the same record counts; stored bytes per second of each (144 B per record)
  pass    kr_post_healpix_map_dev_f64 against kr_post_emissivity_dev_f64 on the same traced, resident records (both are idempotent on them)

Each figure: a warm-up, then the best and the median of `--repeats` runs between two device synchronisations.  KRTRACE_LIB selects another build
of the library (an experiment variant of a kernel, _build.build(tag=...)), `--label` names it in the output.

  python scripts/healpix_ab.py [--repeats 5] [--label product] [--skip-pass] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytrace_cpu_amd import api, capi  # noqa: E402

vp = C.c_void_p
POS, SPIN = (0.0, 5.0, 1e-3, 1.5707), 0.998


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="product")
    ap.add_argument("--skip-pass", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    L = api.lib()
    held = []

    def malloc(nbytes):
        d = vp()
        capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
        held.append(d)
        return d

    def sync():
        capi.check(L, L.kr_synchronize(None), "kr_synchronize")

    def timed(fn):
        fn()
        sync()
        ms = []
        for _ in range(args.repeats):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"best_ms": min(ms), "median_ms": statistics.median(ms)}

    res = {"label": args.label, "library": os.environ.get("KRTRACE_LIB", capi.LIB_PATH), "device": api.device_info()["name"], "repeats": args.repeats, "init": []}
    try:
        for order, rpp, motion, V in ((10, 1, 0, 0.0), (9, 5, 0, 0.0), (10, 1, 1, 0.3), (9, 5, 1, 0.3)):
            s = api.healpix_spec(POS, V, SPIN, order, motion, 0, rpp)
            n, _ = api.healpix_count(s)
            d = malloc(n * 144)
            row = {"order": order, "rays_per_pixel": rpp, "motion": motion, "records": n}
            row["healpix"] = timed(lambda: capi.check(L, L.kr_healpix_init_emit_dev_f64(C.byref(s), 0, 1, 0, d, n, None), "kr_healpix_init_emit"))
            if motion == 0:
                step = 2.0 / math.sqrt(n)                                  # a square grid of about n rays
                ps = capi.PointSourceSpec()
                for i in range(4):
                    ps.pos[i] = POS[i]
                ps.V, ps.spin, ps.tol, ps.E = V, SPIN, 100.0, 1.0
                ps.cosalpha0, ps.cosalphamax, ps.dcosalpha, ps.beta0, ps.betamax, ps.dbeta = -0.9999, 0.9999, step * 0.9999, -math.pi, math.pi, step * math.pi
                m = min(n, api.pointsource_count(ps)[0])
                row["pointsource_records"] = m
                row["pointsource"] = timed(lambda: capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(ps), 0, 1, V, 0, 0, d, m, None), "kr_pointsource_init_emit"))
                row["pointsource"]["stored_GB_per_s"] = 144.0 * m / row["pointsource"]["best_ms"] / 1e6
            row["healpix"]["stored_GB_per_s"] = 144.0 * n / row["healpix"]["best_ms"] / 1e6
            res["init"].append(row)
            L.kr_free(held.pop())

        if not args.skip_pass:
            s = api.healpix_spec(POS, 0.0, SPIN, 10, 0, 0, 1)
            n, npix = api.healpix_count(s)
            d = malloc(n * 144)
            capi.check(L, L.kr_healpix_init_emit_dev_f64(C.byref(s), 0, 1, 0, d, n, None), "kr_healpix_init_emit")
            p = capi.default_params(SPIN)
            p.integrator, p.r_max, p.theta_max, p.flags = capi.EULER, 1000.0, math.pi / 2, capi.FLAG_HYBRID
            t0 = time.perf_counter()
            st = api.trace_dev(p, d.value, n)
            res["trace"] = {"records": n, "wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st["kernel_ms"], "steps_total": st["steps_total"]}
            r_isco = L.kr_kerr_isco(SPIN, 1)
            m = api.healpix_map_struct(npix, r_isco, 500.0, 999.0, 0.0, 5.0, 1.5707, 0, 1)
            d_map = malloc(8 * api.healpix_map_words(m))
            b = capi.EmisBins()
            b.r_min, b.dr, b.r_isco, b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = r_isco, math.exp(math.log(500.0 / r_isco) / 100), r_isco, 2.0, SPIN, float(n), 100, 1
            d_hist = malloc(8 * (5 * b.nr + 1))
            capi.check(L, L.kr_memset(d_map, 0, 8 * api.healpix_map_words(m)), "kr_memset")
            capi.check(L, L.kr_memset(d_hist, 0, 8 * (5 * b.nr + 1)), "kr_memset")
            res["pass"] = {
                "records": n,
                "healpix_map": timed(lambda: capi.check(L, L.kr_post_healpix_map_dev_f64(SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(m), d, n, 0, 1, d_map, None), "kr_post_healpix_map")),
                "emissivity": timed(lambda: capi.check(L, L.kr_post_emissivity_dev_f64(SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(b), d, n, d_hist, None), "kr_post_emissivity")),
            }
            res["pass"]["healpix_map"]["bytes_per_record"] = 144 + 16 + 56
            res["pass"]["emissivity"]["bytes_per_record"] = 144 + 16
        print(json.dumps(res, indent=1))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        L.kr_synchronize(None)
        for d in held:
            L.kr_free(d)


if __name__ == "__main__":
    main()
