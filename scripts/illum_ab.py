"""What the (r, phi) illumination map and the table flavour of the line and the response cost on the device, next to the passes they stand beside
(profiles/illum_map_ab.txt, profiles/illum_pass_ab.txt):

  map     kr_post_illum_dev_f64 and kr_reduce_illum_dev_f64 against kr_post_emissivity_dev_f64 (a kernel this tree does not touch) on the same traced,
          resident records: 1e7 of the lamp post (0, 10, 1e-3, 1.5707) and 1e7 of a source at r = 6, theta = 1.2 (a 3162 x 3162 grid each, Euler, hybrid
          arithmetic); nr = 100 with nphi = 1, 32, 256 (100 cells: the planes in LDS; 3200 and 25 600: global atomics, grouped by wave) and 32 x 32 /
          33 x 32 either side of the 1024-cell crossover.  With --variant LIB the same from a second build whose crossover is 0 --
          _build.build(extra_flags=("-DKR_ILLUM_LDS_CELLS=0",), tag="illumglobal") -- i.e. the global path below the crossover too.  (There is no LDS
          path above it to measure: 5 planes of more than 1024 cells do not fit the budget.)
  pass    kr_post_line_illum_dev_f64 / kr_reduce_line_illum_dev_f64 against kr_post_line_limb_dev_f64 / kr_reduce_line_dev_f64, and
          kr_post_response_illum_dev_f64 / kr_reduce_response_illum_dev_f64 against kr_post_response_dev_f64 / kr_reduce_response_dev_f64 with radial
          tables of the same content, on the records of a --plane x --plane image plane at 80 degrees (RK4, hybrid): nphi = 32 and 256, with and
          without the time plane.

Each figure: a warm-up, then --repeats windows of --inner launches between two device synchronisations, the candidates alternating window by window;
best and median time per launch.

  python scripts/illum_ab.py [--what map,pass] [--plane 4097] [--repeats 5] [--inner 5] [--variant LIB] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytrace_cpu_amd import api, capi  # noqa: E402

vp = C.c_void_p
SPIN = 0.998
SIDE = 3162
PI = math.pi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="map,pass")
    ap.add_argument("--plane", type=int, default=4097)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--variant", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    L = api.lib()
    libs = {"product": L}
    if args.variant:
        libs["global-only"] = capi.load(args.variant)
    held = []

    def malloc(nbytes):
        d = vp()
        capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
        held.append(d)
        return d

    def zeros(nwords):
        d = malloc(8 * nwords)
        capi.check(L, L.kr_memset(d, 0, 8 * nwords), "kr_memset")
        return d

    def release():
        L.kr_synchronize(None)
        while held:
            L.kr_free(held.pop())

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

    res = {"library": capi.LIB_PATH, "variant": args.variant, "device": api.device_info()["name"], "repeats": args.repeats, "inner": args.inner}
    r_isco = L.kr_kerr_isco(SPIN, 1)
    try:
        if "map" in args.what:
            res["map"] = {}
            for source, pos, V in (("lamp post", (0.0, 10.0, 1e-3, 1.5707), 0.0), ("r = 6, theta = 1.2", (0.0, 6.0, 1.2, 0.3), 0.06)):
                ps = capi.PointSourceSpec()
                for i in range(4):
                    ps.pos[i] = pos[i]
                ps.V, ps.spin, ps.tol, ps.E = V, SPIN, 100.0, 1.0
                ps.cosalpha0, ps.cosalphamax, ps.dcosalpha, ps.beta0, ps.betamax, ps.dbeta = -0.995, 0.995, 1.99 / (SIDE - 0.5), -PI, PI, 2 * PI / (SIDE - 0.5)
                n = api.pointsource_count(ps)[0]
                d = malloc(n * 144)
                capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(ps), 0, 1, ps.V, 0, 0, d, n, None), "init emit")
                p = capi.default_params(SPIN)
                p.integrator, p.r_max, p.theta_max, p.flags = capi.EULER, 1100.0, PI / 2, capi.FLAG_HYBRID
                st = api.trace_dev(p, d.value, n)
                rows = {"records": n, "trace_kernel_ms": st["kernel_ms"]}
                for nr, nphi in ((100, 1), (100, 32), (100, 256), (32, 32), (33, 32)):
                    b = capi.EmisBins()
                    b.r_min, b.dr, b.r_isco, b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = r_isco, math.exp(math.log(500.0 / r_isco) / nr), r_isco, 2.0, SPIN, float(n), nr, 1
                    m = capi.illum_bins(b, nphi, 0.0137)
                    d_hist, d_out = zeros(5 * nr + 1), zeros(api.illum_words(m))
                    cand = {"post_emissivity": lambda b=b, d_hist=d_hist: capi.check(
                        L, L.kr_post_emissivity_dev_f64(SPIN, -1.0, 0, 0, 0, -PI, PI, C.byref(b), d, n, d_hist, None), "kr_post_emissivity")}
                    for name, lib in libs.items():
                        cand[f"post_illum[{name}]"] = lambda lib=lib, m=m, d_out=d_out: capi.check(
                            lib, lib.kr_post_illum_dev_f64(SPIN, -1.0, 0, 0, 0, -PI, PI, C.byref(m), d, n, d_out, None), "kr_post_illum")
                        cand[f"reduce_illum[{name}]"] = lambda lib=lib, m=m, d_out=d_out: capi.check(lib, lib.kr_reduce_illum_dev_f64(C.byref(m), d, n, d_out, None), "kr_reduce_illum")
                    t = timed(cand)
                    capi.check(L, L.kr_memset(d_out, 0, 8 * api.illum_words(m)), "kr_memset")
                    capi.check(L, L.kr_reduce_illum_dev_f64(C.byref(m), d, n, d_out, None), "kr_reduce_illum")
                    got = api.illum_from_words(m, api.DeviceScope(L).fetch(d_out, api.illum_words(m)))
                    t["cells"] = nr * nphi
                    t["binned"], t["disc_count"], t["lit_cells"], t["fullest_cell"] = got["binned"], got["disc_count"], int((got["count"] > 0).sum()), int(got["count"].max())
                    rows[f"{nr}x{nphi}"] = t
                res["map"][source] = rows
                release()
        if "pass" in args.what:
            ip = capi.ImagePlaneSpec()
            side = args.plane - 1
            ip.dist, ip.inc_deg, ip.x0, ip.xmax, ip.dx, ip.y0, ip.ymax, ip.dy, ip.spin, ip.phi0, ip.precision = 10000.0, 80.0, -30.0, 30.0, 60.0 / side, -30.0, 30.0, 60.0 / side, SPIN, 0.0, 100.0
            n = api.imageplane_count(ip)[0]
            d = malloc(n * 144)
            capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(ip), 0, 1, 0.0, 1, 0, d, n, None), "init")
            p = capi.copy_params(capi.default_params(-SPIN), integrator=capi.RK4, flags=capi.FLAG_HYBRID, r_max=11000.0, theta_max=PI / 2)
            st = api.trace_dev(p, d.value, n)
            rows = {"records": n, "trace_kernel_ms": st["kernel_ms"]}
            law = capi.limb_law("laor")
            nr, r_disc = 40, 30.0
            dr = (r_disc / r_isco) ** (1.0 / nr)
            emis_r, time_r = np.linspace(2.0, 0.1, nr), 12.0 + 9.0 * np.sqrt(np.arange(nr) / nr)
            s_de = math.exp(math.log(500.0 / 0.05) / 299)
            e = 0.05 * s_de ** np.arange(300)
            S = np.array([e ** -(1.6 + 0.2 * z) * np.exp(-e / 100.0) for z in range(2)])

            def spec(**kw):
                return capi.spectrum_model("table", 0.5, math.exp(math.log(200.0) / 256), 256, log_e=True, r_isco=r_isco, r_disc=r_disc, s=S, s_e_min=0.05, s_de=s_de, **kw)

            for with_time in (False, True):
                line_kw = dict(line_energy=6.4, e_min=1.0, de=0.1, ne=90, t0=9950.0, dt=2.0 if with_time else 0.0, nt=64 if with_time else 1, r_isco=r_isco, r_disc=r_disc)
                flat_b = capi.line_bins(**line_kw).with_table(r_isco, dr, emis_r, time_r if with_time else None)
                b = capi.line_bins(**line_kw)
                flat_R = capi.response_model(spec(table_emis=emis_r, table_r_min=r_isco, table_dr=dr), 9950.0, 2.0, 64, table_time=time_r if with_time else None)
                R = capi.response_model(spec(), 9950.0, 2.0, 64)
                d_line, d_resp = zeros(api.line_words(b) + 1), zeros(api.response_words(R))
                cand = {
                    "post_line_limb (radial table)": lambda: capi.check(L, L.kr_post_line_limb_dev_f64(-SPIN, -1.0, 1, 0, 0, -PI, PI, C.byref(flat_b), C.byref(law), d, n, d_line, None), "a"),
                    "reduce_line (radial table)": lambda: capi.check(L, L.kr_reduce_line_dev_f64(C.byref(flat_b), d, n, d_line, None), "b"),
                    "post_response (radial tables)": lambda: capi.check(L, L.kr_post_response_dev_f64(-SPIN, -1.0, 1, 0, 0, -PI, PI, C.byref(flat_R), C.byref(law), d, n, d_resp, None), "c"),
                    "reduce_response (radial tables)": lambda: capi.check(L, L.kr_reduce_response_dev_f64(C.byref(flat_R), d, n, d_resp, None), "d"),
                }
                for nphi in (32, 256):
                    t = capi.illum_table(np.repeat(emis_r[:, None], nphi, axis=1) * (1 + 0.3 * np.cos(2 * PI * (np.arange(nphi) + 0.5) / nphi)), r_isco, dr, True,
                                         np.repeat(time_r[:, None], nphi, axis=1) + 3 * np.sin(2 * PI * (np.arange(nphi) + 0.5) / nphi) if with_time else None, 0.0137)
                    cand[f"post_line_illum nphi {nphi}"] = lambda t=t: capi.check(
                        L, L.kr_post_line_illum_dev_f64(-SPIN, -1.0, 1, 0, 0, -PI, PI, C.byref(b), C.byref(law), C.byref(t), d, n, d_line, None), "e")
                    cand[f"reduce_line_illum nphi {nphi}"] = lambda t=t: capi.check(L, L.kr_reduce_line_illum_dev_f64(C.byref(b), C.byref(t), d, n, d_line, None), "f")
                    cand[f"post_response_illum nphi {nphi}"] = lambda t=t: capi.check(
                        L, L.kr_post_response_illum_dev_f64(-SPIN, -1.0, 1, 0, 0, -PI, PI, C.byref(R), C.byref(law), C.byref(t), d, n, d_resp, None), "g")
                    cand[f"reduce_response_illum nphi {nphi}"] = lambda t=t: capi.check(L, L.kr_reduce_response_illum_dev_f64(C.byref(R), C.byref(t), d, n, d_resp, None), "h")
                rows["with time" if with_time else "without time"] = timed(cand)
            res["pass"] = rows
            release()
        print(json.dumps(res, indent=1))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        release()


if __name__ == "__main__":
    main()
