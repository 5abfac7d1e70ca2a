"""What the reverberation-response pass costs on the device, which of its open design questions pay, and how far it sits from its two yardsticks, on
traced records that stay in HBM: a 4097 x 4097 image plane at 80 degrees (dist 10000, +-30, a = 0.998), RK4, traced once (the configuration of
scripts/disc_spectrum_ab.py); ne = 256 energies, nt = 64 and nt = 1024 time rows over the window that holds every disc ray; then, launch by launch,

  kr_post_line_dev_f64                       the streaming floor: the same per-ray work, one bin per ray
  kr_post_spectrum_dev_f64 / kr_reduce_...   the same table, energies and records with no time axis: the floor of the arithmetic
  kr_post_response_dev_f64 / kr_reduce_...   the library: (a) a tile's items ordered by time row in LDS before phase B, (b) a contiguous run of tiles per workgroup
  no sort                                    (b) alone: the items in traced order                                } kr_response.hip compiled again with
  no chunk                                   (a) alone: the grid-stride tiles of kr_spectrum.hip                 } its A/B switches
  neither                                    traced order, grid-stride tiles                                     } (scripts/microbench/response_variants.hip)
  ray per lane + global atomics              scripts/microbench/response_ray_per_lane.hip: one global atomic per (ray, energy); the reduce form's records

  python scripts/response_ab.py [--plane 4097] [--launches 10] [--warmups 2] [--build-only]

Every figure: device events (hipEventRecord either side of ONE launch on the null stream) around each of --launches launches after --warmups warm-ups, the
passes taken in turn within every round so that a drift of the clock meets them all alike; median, min and max in ms; (ray, energy) pairs per second from
the tallies of the pass.  The fused passes rewrite rays[].redshift and the wrapped phi with the values they already hold after the first launch, so every
launch sees the same records; the responses only accumulate.  Every other implementation's response is compared with the library's reduce form.  Prints
one JSON object.  --build-only compiles the variants and the alternative (hipcc, gfx950) next to their sources and exits: no device needed.
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
from raytrace_cpu_amd import _build, api, capi  # noqa: E402

vp = C.c_void_p
MB = os.path.join(ROOT, "scripts", "microbench")
ALT = (os.path.join(MB, "response_ray_per_lane.hip"), os.path.join(MB, "libresponse_alt.so"))
VARIANTS = {"no sort": ["-DKR_RESPONSE_SORT=0"], "no chunk": ["-DKR_RESPONSE_CHUNK=0"], "neither": ["-DKR_RESPONSE_SORT=0", "-DKR_RESPONSE_CHUNK=0"]}


def variant_lib(tag):
    return os.path.join(MB, f"libresponse_{tag.replace(' ', '_')}.so")


def build_all():
    jobs = []
    if not os.path.exists(ALT[1]) or os.path.getmtime(ALT[1]) < os.path.getmtime(ALT[0]):
        jobs.append([_build.hipcc(), "--offload-arch=" + _build.ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics", "-shared", "-o", ALT[1], ALT[0]])
    src = os.path.join(MB, "response_variants.hip")
    deps = [src] + [os.path.join(_build.CSRC, f) for f in ("kr_response.hip", "kr_spectrum_dev.hpp", "kr_disc_pass.hpp")]
    for tag, defs in VARIANTS.items():
        lib = variant_lib(tag)
        if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
            jobs.append([_build.hipcc(), *_build.FLAGS, *defs, "-shared", "-Wl,-Bsymbolic", "-o", lib, src, "-L" + _build.CSRC, "-lkrtrace", "-Wl,-rpath," + _build.CSRC])
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
        sys.exit("response_ab: no HIP device (there is no CPU path to time)")
    capi.check(L, L.kr_configure_process(), "kr_configure_process")
    from scripts.arrival_angles_ab import Events, plane
    ev = Events()
    alt = C.CDLL(ALT[1])
    alt.alt_response.restype = C.c_int
    alt.alt_response.argtypes = [C.POINTER(capi.ResponseModel), vp, vp, C.c_longlong, vp, C.c_int]
    var = {}
    for tag in VARIANTS:
        v = var[tag] = C.CDLL(variant_lib(tag))
        v.variant_post_response.restype = v.variant_reduce_response.restype = C.c_int
        v.variant_post_response.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(capi.ResponseModel), C.POINTER(capi.LimbLaw),
                                            vp, C.c_longlong, vp]
        v.variant_reduce_response.argtypes = [C.POINTER(capi.ResponseModel), vp, C.c_longlong, vp]
    spin, pi, r_disc, ne = 0.998, math.pi, 30.0, 256
    r_isco = L.kr_kerr_isco(spin, 1)
    ip = plane(args.plane)
    n = L.kr_imageplane_count(C.byref(ip), None, None)
    s_ne = 2000
    s_de = math.exp(math.log(1000.0 / 0.01) / (s_ne - 1))
    nodes = 0.01 * s_de ** np.arange(s_ne)
    S = nodes ** -1.7 * np.exp(-nodes / 100.0)
    spec = capi.spectrum_model("table", 0.1, math.exp(math.log(100 / 0.1) / ne), ne, log_e=True, r_isco=r_isco, r_disc=r_disc, s=S, s_e_min=0.01, s_de=s_de)
    t_lo, t_hi = 9960.0, 10070.0                                      # holds every disc ray of this plane (`outside` is on record)
    models = {nt: capi.response_model(spec, t_lo, (t_hi - t_lo) / nt, nt) for nt in (64, 1024)}
    lb = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=r_isco, r_disc=r_disc)
    limb1 = capi.limb_law((1, 2.06))
    p = capi.copy_params(capi.default_params(-spin), integrator=capi.RK4, flags=capi.FLAG_HYBRID, r_max=11000.0, theta_max=pi / 2)
    obs = (-spin, -1.0, 1, 0)
    blocks = min((n + 255) // 256, 1024)
    max_words = 1024 * ne + 4

    d_rays, d_line, d_out, d_s = vp(), vp(), vp(), vp()
    sizes = [(d_rays, n * 144), (d_line, (2 * lb.ne + 2) * 8), (d_out, max_words * 8), (d_s, S.nbytes)]
    try:
        for d, nbytes in sizes:
            capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
            capi.check(L, L.kr_memset(d, 0, nbytes), "kr_memset")
        capi.check(L, L.kr_memcpy_h2d(d_s, S.ctypes.data_as(vp), S.nbytes), "h2d")
        st = capi.Stats()
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(ip), 0, 1, 0.0, 1, 0, d_rays, n, None), "init")
        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "trace")
        passes = [("kr_post_line_dev_f64", None, lambda: L.kr_post_line_dev_f64(*obs, 0, -pi, pi, C.byref(lb), d_rays, n, d_line, None)),
                  ("kr_post_spectrum_dev_f64", None, lambda: L.kr_post_spectrum_dev_f64(*obs, 0, -pi, pi, C.byref(spec), C.byref(limb1), d_rays, n, d_out, None)),
                  ("kr_reduce_spectrum_dev_f64", None, lambda: L.kr_reduce_spectrum_dev_f64(C.byref(spec), d_rays, n, d_out, None))]
        for nt, R in models.items():
            tag = f"nt={nt}"
            passes += [(f"kr_post_response_dev_f64 {tag}", nt, lambda R=R: L.kr_post_response_dev_f64(*obs, 0, -pi, pi, C.byref(R), C.byref(limb1), d_rays, n, d_out, None)),
                       (f"kr_reduce_response_dev_f64 {tag}", nt, lambda R=R: L.kr_reduce_response_dev_f64(C.byref(R), d_rays, n, d_out, None))]
            for name, v in var.items():
                passes += [(f"{name}, fused {tag}", nt, lambda R=R, v=v: v.variant_post_response(*obs, 0, -pi, pi, C.byref(R), C.byref(limb1), d_rays, n, d_out)),
                           (f"{name}, reduce {tag}", nt, lambda R=R, v=v: v.variant_reduce_response(C.byref(R), d_rays, n, d_out))]
            passes.append((f"ray per lane + global atomics {tag}", nt, lambda R=R: alt.alt_response(C.byref(R), d_s, d_rays, n, d_out, blocks)))
        # the tallies of one launch per model, and every other implementation's response against the library's reduce form (the same rule on the same records)
        capi.check(L, L.kr_post_line_dev_f64(*obs, 0, -pi, pi, C.byref(lb), d_rays, n, d_line, None), "post_line")
        tallies, agree, runs = {}, {}, {}
        for nt, R in models.items():
            nw = api.response_words(R)
            words = np.zeros(nw)
            others = [("lib", lambda: L.kr_reduce_response_dev_f64(C.byref(R), d_rays, n, d_out, None)), ("alt", lambda: alt.alt_response(C.byref(R), d_s, d_rays, n, d_out, blocks))]
            others += [(name, lambda v=v: v.variant_reduce_response(C.byref(R), d_rays, n, d_out)) for name, v in var.items()]
            for slot, fn in others:
                capi.check(L, L.kr_memset(d_out, 0, max_words * 8), "kr_memset")
                assert fn() == 0
                capi.check(L, L.kr_synchronize(None), "sync")
                capi.check(L, L.kr_memcpy_d2h(words.ctypes.data_as(vp), d_out, words.nbytes), "d2h")
                if slot == "lib":
                    tallies[nt], lib_words = [int(w) for w in words[-4:]], words[:-4].copy()
                else:
                    agree[f"{slot} nt={nt}"] = float(np.abs(words[:-4] - lib_words).max() / np.abs(lib_words).max())
                    if slot != "alt":
                        assert [int(w) for w in words[-4:]] == tallies[nt], (slot, nt)
        # how long the runs are: the time rows of the disc rays in traced order, from a read-back of t, r, theta, redshift, steps (host numpy)
        rec = np.zeros(n, dtype=capi.RAY_F64)
        capi.check(L, L.kr_memcpy_d2h(rec.ctypes.data_as(vp), d_rays, rec.nbytes), "d2h")
        with np.errstate(all="ignore"):
            on = (rec["steps"] > 0) & (rec["r"] * np.cos(rec["theta"]) < 1e-2) & (rec["r"] >= r_isco) & (rec["r"] < r_disc) & (rec["redshift"] > 0)
        for nt, R in models.items():
            row = np.floor((rec["t"][on] - R.t0) / R.dt)
            tile = np.flatnonzero(on) // 256
            same_tile = np.diff(tile) == 0
            runs[nt] = {"items": int(on.sum()), "row_changes_within_tiles_traced_order": int(((np.diff(row) != 0) & same_tile).sum()),
                        "distinct_rows_per_tile_mean": float(np.mean([len(np.unique(row[a:b])) for a, b in zip(*_tile_bounds(tile))]))}
        times = {name: [] for name, *_ in passes}
        for it in range(args.warmups + args.launches):
            for name, _, launch in passes:
                ms = ev.time_ms(launch)
                if it >= args.warmups:
                    times[name].append(ms)
        rows = []
        for name, nt, _ in passes:
            t = times[name]
            row = {"pass": name, "median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
            if nt:
                row["pairs"] = (tallies[nt][1] - tallies[nt][3]) * ne
                row["pairs_per_s"] = row["pairs"] / (row["median_ms"] * 1e-3)
            rows.append(row)
        print(json.dumps({"plane": args.plane, "records": int(n), "trace_kernel_ms": st.kernel_ms, "ne": ne, "window": [t_lo, t_hi],
                          "tallies_on_disc_used_bad_angle_outside": {f"nt={k}": v for k, v in tallies.items()}, "runs": {f"nt={k}": v for k, v in runs.items()},
                          "others_minus_library_maxnorm": agree, "launches": args.launches, "rows": rows}, indent=1))
    finally:
        for d, _ in sizes:
            if d:
                L.kr_free(d)


def _tile_bounds(tile):
    """(starts, ends) of the runs of equal values in the sorted array `tile`."""
    cut = np.flatnonzero(np.diff(tile) != 0) + 1
    return np.concatenate([[0], cut]), np.concatenate([cut, [len(tile)]])


if __name__ == "__main__":
    main()
