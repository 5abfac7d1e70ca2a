"""What the finite-thickness disc costs on the device (profiles/thick_disc_ab.txt):

  trace   ~1e6 rays of a lamp post (source (0, 5, 1e-3, 0), a = 0.5, r_max = 1000) to KR_STOP_THICKDISC (r_in = ISCO, r_out = 400, slope 0.05,
          scale 1) against the same rays to KR_STOP_DISC_ISCO (ISCO, 400, pi/2): kernel_ms of kr_trace_dev_f64 on freshly built rays, strict and
          hybrid, RK4 and RK45; steps and the longest ray of each
  pass    kr_post_emissivity_surface_dev_f64 / kr_post_image_surface_dev_f64 against kr_post_emissivity_dev_f64 / kr_post_image_dev_f64 on the same
          ~1e7 traced, resident records (all idempotent on them): host clock around a device synchronise

One warm-up, then the median and the best of --repeats launches.  Prints one JSON line per measurement.
    python scripts/thick_disc_ab.py [--rays 1e6] [--records 1e7] [--repeats 5]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPIN = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=1e6)
    ap.add_argument("--records", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from raytrace_cpu_amd import api, capi
    from raytrace_cpu_amd.devmem import DeviceScope
    L = api.lib()
    r_isco = L.kr_kerr_isco(SPIN, 1)

    def source(n_target):
        s = capi.PointSourceSpec()
        for i, v in enumerate((0.0, 5.0, 1e-3, 0.0)):
            s.pos[i] = v
        d = 1.99 / (math.sqrt(n_target) - 1)
        s.V, s.spin, s.tol, s.E = 0.0, SPIN, 100.0, 1.0
        s.cosalpha0, s.cosalphamax, s.dcosalpha, s.beta0, s.betamax, s.dbeta = -0.995, 0.995, d, -math.pi, math.pi, d * math.pi / 0.995
        return s, api.pointsource_count(s)[0]

    def params(kind, integrator, flags):
        p = capi.default_params(SPIN)
        p.integrator, p.r_max, p.flags = integrator, 1000.0, flags
        if kind == "thick":
            return api.thick_disc_params(p, r_isco, 400.0, 0.05, 1.0)
        return capi.copy_params(p, stop_kind=capi.STOP_DISC_ISCO, stop_params=(r_isco, 400.0, math.pi / 2, 0.0))

    def stats_of(times):
        return {"median_ms": statistics.median(times), "best_ms": min(times)}

    with DeviceScope(L) as dev:
        spec, n = source(args.rays)
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)

        def build(spec=spec, d=d_rays, n=n):
            capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(spec), 0, 1, 0.0, 0, 0, d, n, None), "init")

        rows = {}
        for iname, integrator in (("rk4", capi.RK4), ("rk45", capi.RK45)):
            for mname, flags in (("strict", 0), ("hybrid", capi.FLAG_HYBRID)):
                for kind in ("isco", "thick"):
                    p = params(kind, integrator, flags)
                    times, last = [], None
                    for rep in range(args.repeats + 1):
                        build()
                        st = capi.Stats()
                        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "trace")
                        if rep:
                            times.append(st.kernel_ms)
                        last = st
                    rec = dev.fetch(d_rays, n, capi.RAY_F64)
                    row = dict(what="trace", integrator=iname, arithmetic=mname, stop=kind, rays=int(last.rays_traced), steps=int(last.steps_total),
                               longest=int(last.longest_ray_steps), dest=int(((rec["status"] & capi.STATUS_DEST) != 0).sum()), side=int(last.rays_strict_side), **stats_of(times))
                    rows[(iname, mname, kind)] = row
                    print(json.dumps(row), flush=True)
                a, b = rows[(iname, mname, "isco")], rows[(iname, mname, "thick")]
                print(json.dumps(dict(what="trace ratio thick / isco", integrator=iname, arithmetic=mname, median=b["median_ms"] / a["median_ms"], best=b["best_ms"] / a["best_ms"],
                                      steps=b["steps"] / a["steps"], ms_per_gigastep_isco=a["median_ms"] / a["steps"] * 1e9, ms_per_gigastep_thick=b["median_ms"] / b["steps"] * 1e9)), flush=True)

    with DeviceScope(L) as dev:
        spec, n = source(args.records)
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(spec), 0, 1, 0.0, 0, 0, d_rays, n, None), "init")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params("thick", capi.RK4, capi.FLAG_HYBRID)), d_rays, n, None, None), "trace")
        eb = capi.EmisBins(r_min=r_isco, dr=math.exp(math.log(400.0 / r_isco) / 100), r_isco=r_isco, gamma=2.0, spin=SPIN, num_primary_rays=float(n), nr=100, logbin=1)
        ib = capi.ImageBins(x0=-1.0, y0=-math.pi, img_dx=2.0 / 512, img_dy=2 * math.pi / 512, r_isco=r_isco, r_disc=400.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0,
                            img_nx=512, img_ny=512, flip_image=0)
        d_hist, d_planes = dev.zeros(8 * api.emissivity_surface_words(eb)), dev.zeros(8 * api.image_words(ib))
        PI = math.pi
        passes = [("kr_post_emissivity_dev_f64 (flat, projradius 0)", lambda: L.kr_post_emissivity_dev_f64(SPIN, -1.0, 0, 0, 0, -PI, PI, C.byref(eb), d_rays, n, d_hist, None)),
                  ("kr_post_emissivity_dev_f64 (flat, projradius 1)", lambda: L.kr_post_emissivity_dev_f64(SPIN, -1.0, 0, 1, 0, -PI, PI, C.byref(eb), d_rays, n, d_hist, None)),
                  ("kr_post_emissivity_surface_dev_f64", lambda: L.kr_post_emissivity_surface_dev_f64(SPIN, 0, -PI, PI, C.byref(eb), d_rays, n, d_hist, None)),
                  ("kr_reduce_emissivity_dev_f64 (flat)", lambda: L.kr_reduce_emissivity_dev_f64(C.byref(eb), d_rays, n, d_hist, None)),
                  ("kr_reduce_emissivity_surface_dev_f64", lambda: L.kr_reduce_emissivity_surface_dev_f64(C.byref(eb), d_rays, n, d_hist, None)),
                  ("kr_post_image_dev_f64 (flat, projradius 1)", lambda: L.kr_post_image_dev_f64(SPIN, -1.0, 0, 1, 0, -PI, PI, C.byref(ib), d_rays, n, d_planes, None)),
                  ("kr_post_image_surface_dev_f64", lambda: L.kr_post_image_surface_dev_f64(SPIN, 0, -PI, PI, C.byref(ib), d_rays, n, d_planes, None))]
        for name, call in passes:
            times = []
            image = "image" in name
            tally = (7 * ib.img_nx * ib.img_ny) if image else ((6 if "surface" in name else 5) * eb.nr)      # where the pass counts the records it accepted
            dev.zero(d_planes if image else d_hist, 8 * (api.image_words(ib) if image else api.emissivity_surface_words(eb)))
            for rep in range(args.repeats + 1):
                capi.check(L, L.kr_synchronize(None), "sync")
                t0 = time.perf_counter()
                capi.check(L, call(), name)
                capi.check(L, L.kr_synchronize(None), "sync")
                if rep:
                    times.append((time.perf_counter() - t0) * 1e3)
            accepted = dev.fetch(C.c_void_p((d_planes if image else d_hist).value + 8 * tally), 1)[0] / (args.repeats + 1)
            print(json.dumps(dict(what="pass", name=name, records=n, accepted=int(round(accepted)), gb_per_s_read=n * 144 / 1e9 / (statistics.median(times) / 1e3), **stats_of(times))), flush=True)


if __name__ == "__main__":
    main()
