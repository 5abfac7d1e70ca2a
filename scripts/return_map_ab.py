"""A/B of the returning-radiation sweep's post pass at the workload's own size (100 source radii x ~1e6 rays, Euler, the merged-batch pipeline of
bench.py::ReturnRadiationWorkload.step_grouped), on one GPU:

  A   init -> trace -> kr_redshift_dev_f64 per radius -> kr_post_return_batch_dev_f64        (two sweeps over the records; four numbers per radius)
  B   init -> trace -> kr_post_return_map_batch_dev_f64                                      (one sweep; the landing map per radius)

Two measurements, each a warm-up followed by three alternating repeats in this one process:
  pass   the post pass alone on traced, resident records (range_phi and redshift are idempotent, so the same records serve every repeat),
         against its memory floor (144 B read + 16 B written per ray over the HBM bandwidth);
  span   the whole sweep, the radii in four interleaved groups on four streams as the benchmark runs them.

  python scripts/return_map_ab.py [--radii 100] [--rays 1e6] [--nr 100] [--arithmetic hybrid|strict] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytrace_cpu_amd import api, capi  # noqa: E402

SPIN, R_DISC, R_ESC = 0.998, 500.0, 1000.0
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12       # bytes / s: spec and measured copy rate of the MI355X
vp = C.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radii", type=int, default=100)
    ap.add_argument("--rays", type=float, default=1e6)
    ap.add_argument("--nr", type=int, default=100, help="landing bins (the program uses as many as source radii)")
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--arithmetic", default="hybrid", choices=["hybrid", "strict"], help="of the trace (the benchmark's default for Euler is hybrid)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    L = api.lib()
    k = args.radii
    r_isco = L.kr_kerr_isco(SPIN, 1)
    dr = math.exp(math.log(R_DISC / r_isco) / k)
    radii = [r_isco * dr ** ir for ir in range(k)]
    d = 1.99 / (math.sqrt(args.rays) - 1.0)
    specs = api.return_radiation_sources(SPIN, radii, d, d * (math.pi / 2) / 0.995)
    counts = [api.pointsource_count(s)[0] for s in specs]
    total = sum(counts)
    dr_map = math.exp(math.log(R_DISC / r_isco) / args.nr)
    maps = [api.return_map_struct(r_isco, R_DISC, R_ESC, r, 1.5707, r_isco, dr_map, args.nr, 1) for r in radii]
    p = capi.default_params(SPIN)
    p.integrator, p.r_max, p.flags = capi.EULER, 1.1 * R_ESC, capi.FLAG_HYBRID if args.arithmetic == "hybrid" else 0
    nw = 5 * args.nr + 6
    held, streams = [], []

    def malloc(nbytes):
        dptr = vp()
        capi.check(L, L.kr_malloc(C.byref(dptr), nbytes), "kr_malloc")
        held.append(dptr)
        return dptr

    def sync(stream=None):
        capi.check(L, L.kr_synchronize(stream), "kr_synchronize")

    try:
        bufs = [malloc(c * 144) for c in counts]
        out4, outm = malloc(k * 32), malloc(k * nw * 8)
        for _ in range(args.groups):
            s = vp()
            capi.check(L, L.kr_stream_create(C.byref(s)), "kr_stream_create")
            streams.append(s)
        groups = []
        for g in range(args.groups):
            idx = list(range(g, k, args.groups))
            n = len(idx)
            groups.append(dict(idx=idx, n=n, specs=(capi.PointSourceSpec * n)(*[specs[j] for j in idx]), V=(C.c_double * n)(*[specs[j].V for j in idx]),
                               ptrs=(vp * n)(*[bufs[j].value for j in idx]), ns=(C.c_int64 * n)(*[counts[j] for j in idx]),
                               bins=(capi.ReturnBins * n)(*[maps[j].cls for j in idx]), maps=(capi.ReturnMap * n)(*[maps[j] for j in idx]),
                               out4=(vp * n)(*[out4.value + 32 * j for j in idx]), outm=(vp * n)(*[outm.value + 8 * nw * j for j in idx])))

        def post(side, grp, stream):
            if side == "A":
                for q in range(grp["n"]):
                    capi.check(L, L.kr_redshift_dev_f64(SPIN, -1.0, 0, 0, 0, grp["ptrs"][q], grp["ns"][q], stream), "kr_redshift_dev")
                capi.check(L, L.kr_post_return_batch_dev_f64(grp["n"], -math.pi, math.pi, grp["bins"], grp["ptrs"], grp["ns"], grp["out4"], stream), "kr_post_return_batch")
            else:
                capi.check(L, L.kr_post_return_map_batch_dev_f64(grp["n"], SPIN, -1.0, 0, 0, 0, -math.pi, math.pi, grp["maps"], grp["ptrs"], grp["ns"], grp["outm"], stream),
                           "kr_post_return_map_batch")

        def zero(side):
            capi.check(L, L.kr_memset(out4, 0, k * 32) if side == "A" else L.kr_memset(outm, 0, k * nw * 8), "kr_memset")
            sync()

        def sweep(side):
            """The whole sweep as the benchmark runs it; returns the wall span in ms."""
            zero(side)
            t0 = time.perf_counter()
            tickets = []
            for grp, s in zip(groups, streams):
                capi.check(L, L.kr_pointsource_init_emit_batch_dev_f64(grp["n"], grp["specs"], grp["V"], 0, 0, grp["ptrs"], grp["ns"], s), "init")
                tickets += api.trace_batch_async([p] * grp["n"], [bufs[j].value for j in grp["idx"]], [counts[j] for j in grp["idx"]], [s.value] * grp["n"])
                post(side, grp, s)
            for s in streams:
                sync(s)
            ms = (time.perf_counter() - t0) * 1e3
            api.trace_wait_many(tickets)
            return ms

        def the_pass(side):
            """The post pass alone over all radii on the default stream, the records traced and resident; returns ms."""
            zero(side)
            t0 = time.perf_counter()
            for grp in groups:
                post(side, grp, None)
            sync()
            return (time.perf_counter() - t0) * 1e3

        import numpy as np
        res = {"radii": k, "rays": total, "landing_bins": args.nr, "arithmetic": args.arithmetic, "device": api.device_info()["name"]}
        sweep("A"), sweep("B")                                             # warm-up: tables, workspaces, code objects; leaves traced records
        for name, fn in (("pass_ms", the_pass), ("span_ms", sweep)):
            fn("A"), fn("B")
            rows = {"A": [], "B": []}
            for _ in range(args.repeats):
                for side in ("A", "B"):
                    rows[side].append(fn(side))
            res[name] = rows
        # the two sides agree on the four sums they share
        a, b = np.zeros((k, 4)), np.zeros((k, nw))
        sync()
        capi.check(L, L.kr_memcpy_d2h(a.ctypes.data_as(vp), out4, a.nbytes), "d2h")
        capi.check(L, L.kr_memcpy_d2h(b.ctypes.data_as(vp), outm, b.nbytes), "d2h")
        res["worst_rel_difference_of_the_shared_sums"] = float(np.max(np.abs(a - b[:, 5 * args.nr:5 * args.nr + 4]) / np.maximum(np.abs(a), 1e-300)))
        res["on_disc"], res["binned"] = int(b[:, 5 * args.nr + 4].sum()), int(b[:, 5 * args.nr + 5].sum())
        res["fullest_bin_share_of_its_source"] = float((b[:, :args.nr].max(axis=1) / np.maximum(b[:, :args.nr].sum(axis=1), 1)).max())
        floor_bytes = 160.0 * total
        res["memory_floor_ms"] = {"at_8.0_TB/s_spec": floor_bytes / HBM_PEAK * 1e3, "at_6.29_TB/s_measured_copy": floor_bytes / HBM_MEASURED * 1e3}
        for side in ("A", "B"):
            best = min(res["pass_ms"][side])
            res[f"pass_{side}_best_ms"] = best
            res[f"pass_{side}_floor_share_spec"] = res["memory_floor_ms"]["at_8.0_TB/s_spec"] / best
        print(json.dumps(res, indent=1))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        L.kr_synchronize(None)
        for s in streams:
            L.kr_stream_destroy(s)
        for dptr in held:
            L.kr_free(dptr)


if __name__ == "__main__":
    main()
