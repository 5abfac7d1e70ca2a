"""What the hot-spot pass costs on the device, against the streaming floor, against the obvious alternative and against its own variants, on traced
records that stay in HBM: a 4097 x 4097 image plane at 80 degrees (dist 10000, +-30, a = 0.998), RK4, traced once; a Keplerian spot at r_spot = 10,
sigma = 1, cut = 3, one period in nt samples; then, launch by launch,

  kr_post_line_dev_f64                the streaming floor: the parent's pass that reads the same bytes, one bin per ray
  kr_post_hotspot_dev_f64             nt = 256 and 1024, ne = 0 and 64, limb law 1
  kr_reduce_hotspot_dev_f64           the same without the frame evaluation, on the records the passes above left
  ray per lane + LDS atomics          scripts/microbench/hotspot_ray_per_lane.hip: one ray per lane looping over the samples; the reduce form's rule
  no sparsity test                    scripts/microbench/hotspot_variants.hip with -DKR_HOTSPOT_SPARSE_MIN_SLOTS=99, fused and reduce; and with
                                      -DKR_HOTSPOT_SPARSE_MIN_SLOTS=1, the test at every slot count (the library: from two slots)
  registers unbounded                 the same with -DKR_HOTSPOT_TWO_WAVE_SLOTS=0: the fused kernels as the compiler sizes them (one wave per SIMD with a
                                      spectrogram) instead of held to two waves per SIMD
  register bound at one slot too      -DKR_HOTSPOT_TWO_WAVE_MIN_SLOTS=1: the bound also where a lane owns one sample (the library: from two)
  spectrogram: LDS against global     nt = 256, ne = 15 and nt = 63, ne = 64 (blocks that fit kHotSpecLdsWords): the library (LDS) against the variant
                                      built with -DKR_HOTSPOT_SPEC_LDS_WORDS=0 (global adds)

  python scripts/hotspot_ab.py [--plane 4097] [--launches 10] [--warmups 2] [--build-only]

Every figure: device events (hipEventRecord either side of ONE launch on the null stream) around each of --launches launches after --warmups warm-ups, the
passes taken in turn within every round so that a drift of the clock meets them all alike; median, min and max in ms.  The passes rewrite
rays[].redshift and the wrapped phi with the values they already hold after the first launch, so every launch sees the same records; the sums only
accumulate.  used / n comes from the tallies; the fraction of (item, sample) pairs with s > 0 from the numpy rule (tests/hotspot_rules.py) on a 513 x 513
plane of the same geometry.  Prints one JSON object.  --build-only compiles the alternative and the variants (hipcc, gfx950) next to their sources and
exits: no device needed.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from raytrace_cpu_amd import _build, api, capi  # noqa: E402

vp = C.c_void_p
MB = os.path.join(ROOT, "scripts", "microbench")
ALT = (os.path.join(MB, "hotspot_ray_per_lane.hip"), os.path.join(MB, "libhotspot_alt.so"), [])
VARIANTS = {"nosparse": ["-DKR_HOTSPOT_SPARSE_MIN_SLOTS=99"], "allsparse": ["-DKR_HOTSPOT_SPARSE_MIN_SLOTS=1"], "specglobal": ["-DKR_HOTSPOT_SPEC_LDS_WORDS=0"], "onewave": ["-DKR_HOTSPOT_TWO_WAVE_SLOTS=0"], "boundone": ["-DKR_HOTSPOT_TWO_WAVE_MIN_SLOTS=1"]}


def build_all():
    jobs = []
    if not os.path.exists(ALT[1]) or os.path.getmtime(ALT[1]) < os.path.getmtime(ALT[0]):
        jobs.append([_build.hipcc(), "--offload-arch=" + _build.ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics", "-shared", "-o", ALT[1], ALT[0]])
    src = os.path.join(MB, "hotspot_variants.hip")
    kernel = os.path.join(_build.CSRC, "kr_hotspot.hip")
    for tag, defs in VARIANTS.items():
        lib = os.path.join(MB, f"libhotspot_{tag}.so")
        if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(src), os.path.getmtime(kernel)):
            jobs.append([_build.hipcc(), *_build.FLAGS, "-Wno-pass-failed", *defs, "-shared", "-Wl,-Bsymbolic", "-o", lib, src, "-L" + _build.CSRC, "-lkrtrace",
                         "-Wl,-rpath," + _build.CSRC])
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(subprocess.check_call, jobs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane", type=int, default=4097)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    build_all()
    if args.build_only:
        return
    L = capi.load()
    if L.kr_device_count() <= 0:
        sys.exit("hotspot_ab: no HIP device (there is no CPU path to time)")
    capi.check(L, L.kr_configure_process(), "kr_configure_process")
    from scripts.arrival_angles_ab import Events, plane
    ev = Events()
    alt = C.CDLL(ALT[1])
    alt.alt_hotspot.restype = C.c_int
    alt.alt_hotspot.argtypes = [C.POINTER(capi.HotSpot), vp, C.c_longlong, vp, C.c_int]
    var = {}
    for tag in VARIANTS:
        v = var[tag] = C.CDLL(os.path.join(MB, f"libhotspot_{tag}.so"))
        v.variant_post_hotspot.restype = v.variant_reduce_hotspot.restype = C.c_int
        v.variant_post_hotspot.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(capi.HotSpot), C.POINTER(capi.LimbLaw), vp,
                                           C.c_longlong, vp]
        v.variant_reduce_hotspot.argtypes = [C.POINTER(capi.HotSpot), vp, C.c_longlong, vp]
    spin, pi, r_disc, dist = 0.998, math.pi, 30.0, 10000.0
    r_isco = L.kr_kerr_isco(spin, 1)
    ip = plane(args.plane)
    n = L.kr_imageplane_count(C.byref(ip), None, None)
    period = 2 * pi * (spin + 10.0 ** 1.5)

    def spot(nt, ne):
        return capi.hot_spot(10.0, 1.0, cut=3.0, phi0=0.4, spin=spin, t0=dist, dt=period / nt, nt=nt, g_index=4.0 if ne == 0 else 3.0, line_energy=6.4, e_min=2.0,
                             de=10.0 / max(ne, 1), ne=ne, r_isco=r_isco, r_disc=r_disc)

    lb = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=r_isco, r_disc=r_disc)
    limb1 = capi.limb_law((1, 2.06))
    p = capi.copy_params(capi.default_params(-spin), integrator=capi.RK4, flags=capi.FLAG_HYBRID, r_max=11000.0, theta_max=pi / 2)
    obs = (-spin, -1.0, 1, 0)
    blocks = min((n + 255) // 256, 1024)
    max_words = 1024 * (3 + 64) + 4

    d_rays, d_line, d_out = vp(), vp(), vp()
    sizes = [(d_rays, n * 144), (d_line, (2 * lb.ne + 2) * 8), (d_out, max_words * 8)]
    try:
        for d, nbytes in sizes:
            capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
            capi.check(L, L.kr_memset(d, 0, nbytes), "kr_memset")
        st = capi.Stats()
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(ip), 0, 1, 0.0, 1, 0, d_rays, n, None), "init")
        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "trace")
        passes = [("kr_post_line_dev_f64", None, lambda: L.kr_post_line_dev_f64(*obs, 0, -pi, pi, C.byref(lb), d_rays, n, d_line, None))]
        spots = {}
        for nt, ne in ((256, 0), (256, 64), (512, 0), (1024, 0), (1024, 64)):
            h = spots[(nt, ne)] = spot(nt, ne)
            tag = f"nt={nt} ne={ne}"
            passes += [(f"kr_post_hotspot_dev_f64 {tag}", (nt, ne), lambda h=h: L.kr_post_hotspot_dev_f64(*obs, 0, -pi, pi, C.byref(h), C.byref(limb1), d_rays, n, d_out, None)),
                       (f"kr_reduce_hotspot_dev_f64 {tag}", (nt, ne), lambda h=h: L.kr_reduce_hotspot_dev_f64(C.byref(h), d_rays, n, d_out, None)),
                       (f"ray per lane + LDS atomics {tag}", (nt, ne), lambda h=h: alt.alt_hotspot(C.byref(h), d_rays, n, d_out, blocks)),
                       (f"no sparsity test, fused {tag}", (nt, ne),
                        lambda h=h: var["nosparse"].variant_post_hotspot(*obs, 0, -pi, pi, C.byref(h), C.byref(limb1), d_rays, n, d_out)),
                       (f"no sparsity test, reduce {tag}", (nt, ne), lambda h=h: var["nosparse"].variant_reduce_hotspot(C.byref(h), d_rays, n, d_out)),
                       (f"sparsity test at every slot count, fused {tag}", (nt, ne),
                        lambda h=h: var["allsparse"].variant_post_hotspot(*obs, 0, -pi, pi, C.byref(h), C.byref(limb1), d_rays, n, d_out)),
                       (f"sparsity test at every slot count, reduce {tag}", (nt, ne), lambda h=h: var["allsparse"].variant_reduce_hotspot(C.byref(h), d_rays, n, d_out)),
                       (f"register bound at one slot too, fused {tag}", (nt, ne),
                        lambda h=h: var["boundone"].variant_post_hotspot(*obs, 0, -pi, pi, C.byref(h), C.byref(limb1), d_rays, n, d_out)),
                       (f"register bound at one slot too, reduce {tag}", (nt, ne), lambda h=h: var["boundone"].variant_reduce_hotspot(C.byref(h), d_rays, n, d_out)),
                       (f"registers unbounded, fused {tag}", (nt, ne),
                        lambda h=h: var["onewave"].variant_post_hotspot(*obs, 0, -pi, pi, C.byref(h), C.byref(limb1), d_rays, n, d_out))]
        for nt, ne in ((256, 15), (63, 64)):
            h = spots[(nt, ne)] = spot(nt, ne)
            tag = f"nt={nt} ne={ne}"
            passes += [(f"spectrogram in LDS, reduce {tag}", (nt, ne), lambda h=h: L.kr_reduce_hotspot_dev_f64(C.byref(h), d_rays, n, d_out, None)),
                       (f"spectrogram by global adds, reduce {tag}", (nt, ne), lambda h=h: var["specglobal"].variant_reduce_hotspot(C.byref(h), d_rays, n, d_out)),
                       (f"spectrogram in LDS, fused {tag}", (nt, ne),
                        lambda h=h: L.kr_post_hotspot_dev_f64(*obs, 0, -pi, pi, C.byref(h), C.byref(limb1), d_rays, n, d_out, None)),
                       (f"spectrogram by global adds, fused {tag}", (nt, ne),
                        lambda h=h: var["specglobal"].variant_post_hotspot(*obs, 0, -pi, pi, C.byref(h), C.byref(limb1), d_rays, n, d_out))]
        # the tallies of one launch per spot, and every other implementation's words against the library's reduce form (the same rule on the same records)
        capi.check(L, L.kr_post_line_dev_f64(*obs, 0, -pi, pi, C.byref(lb), d_rays, n, d_line, None), "post_line")
        used, agree = {}, {}
        for key, h in spots.items():
            nw = api.hotspot_words(h)
            words = np.zeros(nw)
            others = [("lib", lambda: L.kr_reduce_hotspot_dev_f64(C.byref(h), d_rays, n, d_out, None)), ("alt", lambda: alt.alt_hotspot(C.byref(h), d_rays, n, d_out, blocks))]
            others += [(tag, lambda v=v: v.variant_reduce_hotspot(C.byref(h), d_rays, n, d_out)) for tag, v in var.items()]
            for slot, fn in others:
                capi.check(L, L.kr_memset(d_out, 0, max_words * 8), "kr_memset")
                assert fn() == 0
                capi.check(L, L.kr_synchronize(None), "sync")
                capi.check(L, L.kr_memcpy_d2h(words.ctypes.data_as(vp), d_out, words.nbytes), "d2h")
                if slot == "lib":
                    used[key], lib_words = (int(words[-4]), int(words[-3])), words[:-4].copy()
                else:
                    agree[f"{slot} nt={key[0]} ne={key[1]}"] = float(np.abs(words[:-4] - lib_words).max() / np.abs(lib_words).max())
        times = {name: [] for name, *_ in passes}
        for it in range(args.warmups + args.launches):
            for name, _, launch in passes:
                ms = ev.time_ms(launch)
                if it >= args.warmups:
                    times[name].append(ms)
        rows = []
        for name, key, _ in passes:
            t = times[name]
            row = {"pass": name, "median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
            if key:
                row["pairs"] = used[key][1] * key[0]
            rows.append(row)
    finally:
        for d, _ in sizes:
            if d:
                L.kr_free(d)
    # the fraction of (item, sample) pairs with s > 0: the numpy rule on a small plane of the same geometry
    import hotspot_rules as hr
    small = api.hotspot_lightcurve(plane(513), p, spot(256, 0), return_records=True)
    lo = hr.hotspot(spot(256, 0), small["records"])
    print(json.dumps({"plane": args.plane, "records": int(n), "trace_kernel_ms": st.kernel_ms,
                      "on_disc_used": {f"nt={k[0]} ne={k[1]}": v for k, v in used.items()},
                      "pairs_lit_fraction_513": lo["pairs"] / (lo["used"] * 256.0), "used_513": lo["used"], "records_513": int(len(small["records"])),
                      "others_minus_library_maxnorm": agree, "launches": args.launches, "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
