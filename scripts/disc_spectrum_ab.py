"""What the continuum-spectrum pass costs on the device, against the streaming floor and against the obvious alternative, on traced records that stay
in HBM: a 4097 x 4097 image plane at 80 degrees (dist 10000, +-30, a = 0.998), RK4, traced once; then, launch by launch,

  kr_post_line_dev_f64                          the streaming floor: the same per-ray work, one energy bin per ray
  kr_post_spectrum_dev_f64                      thermal and table model, ne = 256 and ne = 1024, limb law 1
  kr_reduce_spectrum_dev_f64                    the same without the frame evaluation, on the records the passes above left
  ray per lane + LDS atomics                    scripts/microbench/spectrum_ray_per_lane.hip: one ray per lane looping over the energies, atomicAdd into an
                                                LDS spectrum -- the line kernels' shape; the reduce form's rule and records

  python scripts/disc_spectrum_ab.py [--plane 4097] [--launches 10] [--warmups 2] [--build-only]

Every figure: device events (hipEventRecord either side of ONE launch on the null stream) around each of --launches launches after --warmups warm-ups, the
passes taken in turn within every round so that a drift of the clock meets them all alike; median, min and max in ms; (ray, energy) pairs per second from
the `used` tally of the pass; for the thermal model the implied fp64 rate, counting the inner loop's vector fp64 instructions per pair from the compiled
kernel (--ops-per-pair, default from profiles/disc_spectrum_ab.txt).  The passes rewrite rays[].redshift and the wrapped phi with the values they
already hold after the first launch, so every launch sees the same records; the spectra only accumulate.  Prints one JSON object.
--build-only compiles the alternative (hipcc, gfx950) next to its source and exits: no device needed.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytrace_cpu_amd import _build, api, capi  # noqa: E402

vp = C.c_void_p
ALT_SRC = os.path.join(ROOT, "scripts", "microbench", "spectrum_ray_per_lane.hip")
ALT_LIB = os.path.join(ROOT, "scripts", "microbench", "libspectrum_alt.so")


def build_alt():
    if not os.path.exists(ALT_LIB) or os.path.getmtime(ALT_LIB) < os.path.getmtime(ALT_SRC):
        subprocess.check_call([_build.hipcc(), "--offload-arch=" + _build.ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics", "-shared",
                               "-o", ALT_LIB, ALT_SRC])
    return ALT_LIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane", type=int, default=4097)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--ops-per-pair", type=float, default=0.0)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    build_alt()
    if args.build_only:
        return
    L = capi.load()
    if L.kr_device_count() <= 0:
        sys.exit("disc_spectrum_ab: no HIP device (there is no CPU path to time)")
    capi.check(L, L.kr_configure_process(), "kr_configure_process")
    from scripts.arrival_angles_ab import Events, plane
    ev = Events()
    alt = C.CDLL(ALT_LIB)
    alt.alt_spectrum.restype = C.c_int
    alt.alt_spectrum.argtypes = [C.POINTER(capi.SpectrumModel), vp, vp, vp, C.c_longlong, vp, C.c_int]
    spin, pi, r_disc = 0.998, math.pi, 30.0
    r_isco = L.kr_kerr_isco(spin, 1)
    ip = plane(args.plane)
    n = L.kr_imageplane_count(C.byref(ip), None, None)
    nr = 400
    dr = (r_disc / r_isco) ** (1.0 / nr)
    kt = api.thermal_kt_table(spin, r_isco, dr, nr, 10.0, 1e18)
    s_ne = 2000
    s_de = math.exp(math.log(1000.0 / 0.01) / (s_ne - 1))
    nodes = 0.01 * s_de ** np.arange(s_ne)
    S = nodes ** -1.7 * np.exp(-nodes / 100.0)

    def model(kind, ne):
        if kind == "thermal":
            return capi.spectrum_model("thermal", 0.05, math.exp(math.log(20 / 0.05) / ne), ne, log_e=True, r_isco=r_isco, r_disc=r_disc, f_col=1.7, table_r_min=r_isco,
                                       table_dr=dr, table_kt=kt)
        return capi.spectrum_model("table", 0.1, math.exp(math.log(100 / 0.1) / ne), ne, log_e=True, r_isco=r_isco, r_disc=r_disc, s=S, s_e_min=0.01, s_de=s_de)

    lb = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=r_isco, r_disc=r_disc)
    limb1 = capi.limb_law((1, 2.06))
    p = capi.copy_params(capi.default_params(-spin), integrator=capi.RK4, flags=capi.FLAG_HYBRID, r_max=11000.0, theta_max=pi / 2)
    obs = (-spin, -1.0, 1, 0)
    blocks = min((n + 255) // 256, 1024)

    d_rays, d_line, d_out, d_kt, d_s = vp(), vp(), vp(), vp(), vp()
    sizes = [(d_rays, n * 144), (d_line, (2 * lb.ne + 2) * 8), (d_out, 1028 * 8), (d_kt, kt.nbytes), (d_s, S.nbytes)]
    try:
        for d, nbytes in sizes:
            capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
            capi.check(L, L.kr_memset(d, 0, nbytes), "kr_memset")
        capi.check(L, L.kr_memcpy_h2d(d_kt, kt.ctypes.data_as(vp), kt.nbytes), "h2d")
        capi.check(L, L.kr_memcpy_h2d(d_s, S.ctypes.data_as(vp), S.nbytes), "h2d")
        st = capi.Stats()
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(ip), 0, 1, 0.0, 1, 0, d_rays, n, None), "init")
        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "trace")
        passes = [("kr_post_line_dev_f64", None, None, lambda: L.kr_post_line_dev_f64(*obs, 0, -pi, pi, C.byref(lb), d_rays, n, d_line, None))]
        models = {}
        for kind in ("thermal", "table"):
            for ne in (256, 1024):
                m = models[(kind, ne)] = model(kind, ne)
                passes.append((f"kr_post_spectrum_dev_f64 {kind} ne={ne}", kind, ne,
                               lambda m=m: L.kr_post_spectrum_dev_f64(*obs, 0, -pi, pi, C.byref(m), C.byref(limb1), d_rays, n, d_out, None)))
                passes.append((f"kr_reduce_spectrum_dev_f64 {kind} ne={ne}", kind, ne, lambda m=m: L.kr_reduce_spectrum_dev_f64(C.byref(m), d_rays, n, d_out, None)))
                passes.append((f"ray per lane + LDS atomics {kind} ne={ne}", kind, ne, lambda m=m: alt.alt_spectrum(C.byref(m), d_kt, d_s, d_rays, n, d_out, blocks)))
        # the tallies of one fused launch per model, and the alternative's spectrum against the reduce form's (the same rule on the same records)
        used, agree = {}, {}
        for key, m in models.items():
            words = np.zeros(m.ne + 4)
            for fn, slot in ((lambda: L.kr_reduce_spectrum_dev_f64(C.byref(m), d_rays, n, d_out, None), "lib"), (lambda: alt.alt_spectrum(C.byref(m), d_kt, d_s, d_rays, n, d_out, blocks), "alt")):
                if slot == "lib":
                    capi.check(L, L.kr_post_spectrum_dev_f64(*obs, 0, -pi, pi, C.byref(m), C.byref(capi.limb_law((0, 0.0))), d_rays, n, d_out, None), "post")
                capi.check(L, L.kr_memset(d_out, 0, 1028 * 8), "kr_memset")
                assert fn() == 0
                capi.check(L, L.kr_synchronize(None), "sync")
                capi.check(L, L.kr_memcpy_d2h(words.ctypes.data_as(vp), d_out, words.nbytes), "d2h")
                if slot == "lib":
                    used[key], lib_flux = int(words[m.ne + 1]), words[:m.ne].copy()
                else:
                    agree[key] = float(np.max(np.abs(words[:m.ne] / lib_flux - 1)))
        times = {name: [] for name, *_ in passes}
        for it in range(args.warmups + args.launches):
            for name, _, _, launch in passes:
                ms = ev.time_ms(launch)
                if it >= args.warmups:
                    times[name].append(ms)
        rows = []
        for name, kind, ne, _ in passes:
            t = times[name]
            row = {"pass": name, "median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
            if kind:
                row["pairs"] = used[(kind, ne)] * ne
                row["pairs_per_s"] = row["pairs"] / (row["median_ms"] * 1e-3)
                if kind == "thermal" and args.ops_per_pair > 0:
                    row["fp64_instr_per_s"] = row["pairs_per_s"] * args.ops_per_pair
            rows.append(row)
        print(json.dumps({"plane": args.plane, "records": int(n), "trace_kernel_ms": st.kernel_ms, "used": {f"{k[0]} ne={k[1]}": v for k, v in used.items()},
                          "alternative_minus_library_rel": {f"{k[0]} ne={k[1]}": v for k, v in agree.items()}, "launches": args.launches, "rows": rows}, indent=1))
    finally:
        for d, _ in sizes:
            if d:
                L.kr_free(d)


if __name__ == "__main__":
    main()
