"""Timing of the point source with any four-velocity and of the angular-distribution pass next to the existing yardsticks, on one GPU
(profiles/source_vel_ab.txt):

  init    kr_pointsource_vel_init_emit_dev_f64 and kr_pointsource_vel_init_dev_f64 on a 3162 x 3162 grid (1e7 records) against
          kr_pointsource_init_emit_dev_f64 on the same grid; stored bytes per second of each (144 B per record)
  pass    kr_post_angdist_dev_f64 and kr_reduce_angdist_dev_f64 (Nangle = 62: histograms in LDS; 4096: global atomics) against
          kr_post_emissivity_dev_f64 on the same 1e7 traced, resident records (all idempotent on them)
  A/B     with --variant LIB the same passes from a second build of the library (the reduction without the wave-grouped adds:
          _build.build(extra_flags=("-DKR_ANGDIST_AGG=0",), tag="noagg")), alternating with the product in the same process

Each figure: a warm-up, then `--repeats` windows of `--inner` launches between two device synchronisations, the candidates alternating window by
window; best and median time per launch.

  python scripts/source_vel_ab.py [--repeats 7] [--inner 10] [--variant raytrace_cpu_amd/csrc/libkrtrace_noagg.so] [--out FILE.json]
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
POS = (0.0, 6.0, 1.2, 0.3)
SIDE = 3162


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--variant", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    L = api.lib()
    libs = {"product": L}
    if args.variant:
        libs["variant"] = capi.load(args.variant)
    held = []

    def malloc(nbytes):
        d = vp()
        capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
        held.append(d)
        return d

    def sync():
        capi.check(L, L.kr_synchronize(None), "kr_synchronize")

    def timed(candidates):
        """candidates: {name: fn}; alternating windows.  Returns {name: {best_ms, median_ms}} per launch."""
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

    res = {"library": capi.LIB_PATH, "variant": args.variant, "device": api.device_info()["name"], "repeats": args.repeats, "inner": args.inner}
    try:
        u = api.four_velocity(POS, SPIN, omega=0.06, dr_dt=0.15, dtheta_dt=-0.01)
        dc, db = 1.99 / (SIDE - 0.5), 2 * math.pi / (SIDE - 0.5)
        vel = api.pointsource_vel_spec(POS, u, SPIN, dc, db)
        n = api.pointsource_vel_count(vel)[0]
        ps = capi.PointSourceSpec()
        for i in range(4):
            ps.pos[i] = POS[i]
        ps.V, ps.spin, ps.tol, ps.E = 0.06, SPIN, 100.0, 1.0
        ps.cosalpha0, ps.cosalphamax, ps.dcosalpha, ps.beta0, ps.betamax, ps.dbeta = -0.995, 0.995, dc, -math.pi, math.pi, db
        assert api.pointsource_count(ps)[0] == n
        d = malloc(n * 144)
        init = timed({
            "pointsource_vel_init_emit": lambda: capi.check(L, L.kr_pointsource_vel_init_emit_dev_f64(C.byref(vel), d, n, None), "vel init emit"),
            "pointsource_vel_init": lambda: capi.check(L, L.kr_pointsource_vel_init_dev_f64(C.byref(vel), d, n, None), "vel init"),
            "pointsource_init_emit": lambda: capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(ps), 0, 1, ps.V, 0, 0, d, n, None), "ps init emit"),
        })
        for row in init.values():
            row["stored_GB_per_s"] = 144.0 * n / row["best_ms"] / 1e6
        res["init"] = {"records": n, **init}

        capi.check(L, L.kr_pointsource_vel_init_emit_dev_f64(C.byref(vel), d, n, None), "vel init emit")
        p = capi.default_params(SPIN)
        p.integrator, p.r_max, p.theta_max, p.flags = capi.EULER, 1100.0, math.pi / 2, capi.FLAG_HYBRID
        t0 = time.perf_counter()
        st = api.trace_dev(p, d.value, n)
        res["trace"] = {"records": n, "wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st["kernel_ms"], "steps_total": st["steps_total"]}
        r_isco = L.kr_kerr_isco(SPIN, 1)
        b = capi.EmisBins()
        b.r_min, b.dr, b.r_isco, b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = r_isco, math.exp(math.log(500.0 / r_isco) / 100), r_isco, 2.0, SPIN, float(n), 100, 1
        d_hist = malloc(8 * (5 * b.nr + 1))
        capi.check(L, L.kr_memset(d_hist, 0, 8 * (5 * b.nr + 1)), "kr_memset")
        res["pass"] = {"records": n, "bytes_per_record": 144 + 16}
        for nangle in (62, 4096):
            sp = api.angdist_spec(r_isco, 500.0, 1000.0, dangle=2 * math.pi / (nangle + 0.5), labels=1)
            nw = api.angdist_words(sp)
            d_out = malloc(8 * nw)
            capi.check(L, L.kr_memset(d_out, 0, 8 * nw), "kr_memset")
            cand = {}
            for name, lib in libs.items():
                cand[f"post_angdist[{name}]"] = (lambda lib=lib, sp=sp, d_out=d_out: capi.check(
                    lib, lib.kr_post_angdist_dev_f64(SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(sp), d, n, d_out, None), "kr_post_angdist"))
                cand[f"reduce_angdist[{name}]"] = (lambda lib=lib, sp=sp, d_out=d_out: capi.check(
                    lib, lib.kr_reduce_angdist_dev_f64(C.byref(sp), d, n, d_out, None), "kr_reduce_angdist"))
            cand["post_emissivity"] = lambda: capi.check(L, L.kr_post_emissivity_dev_f64(SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, C.byref(b), d, n, d_hist, None), "kr_post_emissivity")
            rows = timed(cand)
            for row in rows.values():
                row["GB_per_s"] = (144.0 + 16.0) * n / row["best_ms"] / 1e6
            res["pass"][f"nangle_{nangle}"] = rows
            # the tallies of the last window, for the record: what the 1e7 rays did
            capi.check(L, L.kr_memset(d_out, 0, 8 * nw), "kr_memset")
            capi.check(L, L.kr_reduce_angdist_dev_f64(C.byref(sp), d, n, d_out, None), "kr_reduce_angdist")
            words = api.angdist_from_words(sp, api.DeviceScope(L).fetch(d_out, nw))
            res["pass"][f"nangle_{nangle}"]["tallies"] = {k: words[k] for k in ("ray_count", "escape_sum", "return_sum", "lost_sum", "other", "skipped", "out_of_range", "bad_g")}
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
