"""Timing of the source-to-observer link next to the nearest existing pass, on one GPU (profiles/observer_link_ab.txt):

  pass    kr_post_observer_dev_f64 and kr_reduce_observer_dev_f64 on 1e7 traced, resident records of the lamp post ps_h10 (a 3162 x 3162 grid), with
          the planes in LDS (nmu = 20, nt = 64: 1360 words) and in global memory (nmu = 128, nt = 64: 8704 words), against kr_post_angdist_dev_f64
          (Nangle = 62) on the same records -- the same loads, wrap and redshift -- from this library and, with --parent LIB, from the parent commit's
  A/B     with --noagg LIB / --agg LIB the observer passes from builds that never / always sum the lanes of a wave before they add
          (_build.build(extra_flags=("-DKR_OBSERVER_AGG=0",), tag="obs_noagg"), ("-DKR_OBSERVER_AGG=2",), tag="obs_agg"); the product groups on the
          global planes only), alternating with the product in the same process

Each figure: a warm-up, then `--repeats` windows of `--inner` launches between two device synchronisations, the candidates alternating window by
window; best and median time per launch.  All passes are idempotent on the records (the fused ones rewrite phi and redshift with the same values).

  python scripts/observer_ab.py [--repeats 7] [--inner 10] [--parent LIB] [--noagg LIB] [--agg LIB] [--out FILE.json]
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
SPIN = 0.998
POS = (0.0, 10.0, 1e-3, 1.5707)
SIDE = 3162


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--parent", default="")
    ap.add_argument("--noagg", default="")
    ap.add_argument("--agg", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    L = api.lib()
    libs = {"product": L}
    for tag in ("noagg", "agg"):
        if getattr(args, tag):
            libs[tag] = capi.load(getattr(args, tag))
    parent = None
    if args.parent:                                  # the parent commit's library has no observer symbols: bind the one pass that is timed
        parent = C.CDLL(args.parent)
        parent.kr_post_angdist_dev_f64.restype, parent.kr_post_angdist_dev_f64.argtypes = capi.PROTOTYPES["kr_post_angdist_dev_f64"]
    held = []

    def malloc(nbytes):
        d = vp()
        capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
        held.append(d)
        capi.check(L, L.kr_memset(d, 0, nbytes), "kr_memset")
        return d

    def sync():
        capi.check(L, L.kr_synchronize(None), "kr_synchronize")

    def timed(candidates):
        for fn in candidates.values():
            fn()
        sync()
        ms = {k: [] for k in candidates}
        for _ in range(args.repeats):
            for k, fn in candidates.items():
                sync()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    fn()
                sync()
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.inner)
        return {k: {"best_ms": min(v), "median_ms": statistics.median(v)} for k, v in ms.items()}

    res = {"library": capi.LIB_PATH, "parent": args.parent, "noagg": args.noagg, "agg": args.agg, "device": api.device_info()["name"], "repeats": args.repeats,
           "inner": args.inner}
    try:
        dc, db = 1.99 / (SIDE - 0.5), 2 * math.pi / (SIDE - 0.5)
        ps = capi.PointSourceSpec()
        for i in range(4):
            ps.pos[i] = POS[i]
        ps.V, ps.spin, ps.tol, ps.E = 0.0, SPIN, 100.0, 1.0
        ps.cosalpha0, ps.cosalphamax, ps.dcosalpha, ps.beta0, ps.betamax, ps.dbeta = -0.995, 0.995, dc, -math.pi, math.pi, db
        n = api.pointsource_count(ps)[0]
        d = malloc(n * 144)
        capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(ps), 0, 1, ps.V, 0, 0, d, n, None), "ps init emit")
        p = capi.default_params(SPIN)
        p.integrator, p.r_max, p.theta_max, p.flags = capi.EULER, 1100.0, math.pi / 2, capi.FLAG_HYBRID
        t0 = time.perf_counter()
        st = api.trace_dev(p, d.value, n)
        res["trace"] = {"records": n, "wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st["kernel_ms"], "steps_total": st["steps_total"]}
        r_isco = L.kr_kerr_isco(SPIN, 1)
        ang = api.angdist_spec(r_isco, 400.0, 1000.0, dangle=2 * math.pi / 62.5, labels=0)
        d_ang = malloc(8 * api.angdist_words(ang))
        res["pass"] = {"records": n, "bytes_per_record_fused": 144 + 16, "bytes_per_record_reduce": 144}
        for label, nmu, nt in (("lds_20x64", 20, 64), ("global_128x64", 128, 64)):
            sp = api.observer_spec(SPIN, r_isco, 400.0, 1000.0, nmu=nmu, gamma=2.0, dist=10000.0, t0=10000.0, dt=0.5, nt=nt)
            nw = api.observer_words(sp)
            d_out = malloc(8 * nw)
            cand = {}
            for name, lib in libs.items():
                cand[f"post_observer[{name}]"] = (lambda lib=lib, sp=sp, d_out=d_out: capi.check(
                    lib, lib.kr_post_observer_dev_f64(SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(sp), d, n, d_out, None), "kr_post_observer"))
                cand[f"reduce_observer[{name}]"] = (lambda lib=lib, sp=sp, d_out=d_out: capi.check(
                    lib, lib.kr_reduce_observer_dev_f64(C.byref(sp), d, n, d_out, None), "kr_reduce_observer"))
            cand["post_angdist[product]"] = lambda: capi.check(L, L.kr_post_angdist_dev_f64(SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(ang), d, n, d_ang, None), "kr_post_angdist")
            if parent is not None:
                cand["post_angdist[parent]"] = lambda: capi.check(L, parent.kr_post_angdist_dev_f64(SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(ang), d, n, d_ang, None),
                                                                  "kr_post_angdist (parent)")
            rows = timed(cand)
            for k, row in rows.items():
                row["GB_per_s"] = (144.0 if k.startswith("reduce") else 160.0) * n / row["best_ms"] / 1e6
            res["pass"][label] = rows
            capi.check(L, L.kr_memset(d_out, 0, 8 * nw), "kr_memset")
            capi.check(L, L.kr_reduce_observer_dev_f64(C.byref(sp), d, n, d_out, None), "kr_reduce_observer")
            words = api.observer_from_words(sp, api.DeviceScope(L).fetch(d_out, nw))
            res["pass"][label]["tallies"] = {k: words[k] for k in api.OBSERVER_TALLIES}
            res["pass"][label]["observer_flux"] = [float(x) for x in api.observer_flux(words)][:20]
        print(json.dumps(res, indent=1))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        L.kr_synchronize(None)
        for d_ in held:
            L.kr_free(d_)


if __name__ == "__main__":
    main()
