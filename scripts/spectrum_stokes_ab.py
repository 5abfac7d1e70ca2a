"""What the Stokes spectra of the continuum cost on the device, against the passes they join and against their own variants, on the workload of
scripts/disc_spectrum_ab.py: traced records that stay in HBM -- a 4097 x 4097 image plane at 80 degrees (dist 10000, +-30, a = 0.998), RK4, traced once;
the thermal model (10 Msun, 1e18 g/s, f_col 1.7) and a 2000-node table in LDS at 256, 512 and 1024 energies; limb law 1, pol law 1.  Launch by launch,

  kr_post_spectrum_stokes_dev_f64      the fused Stokes form
  kr_reduce_spectrum_stokes_dev_f64    the Stokes reduce form (the frame again for the on-disc records), on the records the passes above left
  kr_post_spectrum_dev_f64, kr_reduce_spectrum_dev_f64, kr_polarisation_dev_f64
                                       the existing passes, from this tree's library and -- with --parent-lib -- from the parent commit's, taken in turn in
                                       the same rounds: spectrum + polarisation is a LOWER BOUND on any two-pass scheme (no existing call sequence yields
                                       Q(E) and U(E): the spectrum pass sums over rays before anyone can weight a ray), and this tree against the parent
                                       shows the existing instances unchanged
  frame_value first                    scripts/microbench/spectrum_stokes_variants.hip with -DKR_SPECTRUM_STOKES_FRAME_FIRST: frame_value for every record,
                                       polar_value for the on-disc ones (the library: polar_value in place of frame_value for every record)
  registers unbounded                  -DKR_SPECTRUM_STOKES_TWO_WAVE_SLOTS=0: every Stokes kernel as the compiler sizes it
  bound up to four / sixteen slots     -DKR_SPECTRUM_STOKES_TWO_WAVE_SLOTS=4 / 16: every Stokes kernel held to two waves per SIMD up to that many slots
                                       (the library: only the fused table forms at four slots, the ones that fall to one wave otherwise)

  python scripts/spectrum_stokes_ab.py [--plane 4097] [--launches 10] [--warmups 2] [--parent-lib PATH] [--build-only]

Every figure: device events (hipEventRecord either side of ONE launch on the null stream) around each of --launches launches after --warmups warm-ups, the
passes taken in turn within every round so that a drift of the clock meets them all alike; median, min and max in ms.  The passes rewrite
rays[].redshift and the wrapped phi with the values they already hold after the first launch, so every launch sees the same records; the sums only
accumulate.  Every variant's words are compared with the library's on the same records.  Prints one JSON object.  --build-only compiles the variants
(hipcc, gfx950) next to their source and exits: no device needed.
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
VARIANTS = {"framefirst": ["-DKR_SPECTRUM_STOKES_FRAME_FIRST"], "unbounded": ["-DKR_SPECTRUM_STOKES_TWO_WAVE_SLOTS=0"], "bound4": ["-DKR_SPECTRUM_STOKES_TWO_WAVE_SLOTS=4"],
            "bound16": ["-DKR_SPECTRUM_STOKES_TWO_WAVE_SLOTS=16"]}
LABEL = {"framefirst": "frame_value first", "unbounded": "registers unbounded", "bound4": "bound up to four slots", "bound16": "bound up to sixteen slots"}


def build_all():
    jobs = []
    src = os.path.join(MB, "spectrum_stokes_variants.hip")
    kernel = os.path.join(_build.CSRC, "kr_spectrum.hip")
    for tag, defs in VARIANTS.items():
        lib = os.path.join(MB, f"libspectrum_stokes_{tag}.so")
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
    ap.add_argument("--parent-lib", default="", help="libkrtrace.so built from the parent commit: its spectrum and polarisation passes are timed in the same rounds")
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    build_all()
    if args.build_only:
        return
    L = capi.load()
    if L.kr_device_count() <= 0:
        sys.exit("spectrum_stokes_ab: no HIP device (there is no CPU path to time)")
    capi.check(L, L.kr_configure_process(), "kr_configure_process")
    from scripts.arrival_angles_ab import Events, plane
    ev = Events()
    dbl, i32, i64 = C.c_double, C.c_int, C.c_longlong
    M, LL, PL = C.POINTER(capi.SpectrumModel), C.POINTER(capi.LimbLaw), C.POINTER(capi.PolLaw)
    var = {}
    for tag in VARIANTS:
        v = var[tag] = C.CDLL(os.path.join(MB, f"libspectrum_stokes_{tag}.so"))
        v.variant_post_spectrum_stokes.restype = v.variant_reduce_spectrum_stokes.restype = C.c_int
        v.variant_post_spectrum_stokes.argtypes = [dbl, dbl, i32, i32, dbl, dbl, dbl, M, LL, PL, vp, i64, vp]
        v.variant_reduce_spectrum_stokes.argtypes = [dbl, dbl, i32, i32, dbl, M, LL, PL, vp, i64, vp]
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        for name in ("kr_post_spectrum_dev_f64", "kr_reduce_spectrum_dev_f64", "kr_polarisation_dev_f64"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = capi.PROTOTYPES[name]
        assert not hasattr(parent, "kr_post_spectrum_stokes_dev_f64"), "--parent-lib exports the Stokes entry points: not the parent commit's library"
    spin, pi, r_disc, inc = 0.998, math.pi, 30.0, 80.0
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

    limb1, pol1 = capi.limb_law((1, 2.06)), capi.pol_law((1, 0.1171))
    p = capi.copy_params(capi.default_params(-spin), integrator=capi.RK4, flags=capi.FLAG_HYBRID, r_max=11000.0, theta_max=pi / 2)
    obs = (-spin, -1.0, 1, 0)
    max_words = 3 * 1024 + 4

    d_rays, d_out, d_pol = vp(), vp(), vp()
    sizes = [(d_rays, n * 144), (d_out, max_words * 8), (d_pol, n * 32)]
    try:
        for d, nbytes in sizes:
            capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
            capi.check(L, L.kr_memset(d, 0, nbytes), "kr_memset")
        st = capi.Stats()
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(ip), 0, 1, 0.0, 1, 0, d_rays, n, None), "init")
        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "trace")
        libs = [("this tree", L)] + ([("parent", parent)] if parent else [])
        passes = [(f"kr_polarisation_dev_f64 ({who})", None, lambda lib=lib: lib.kr_polarisation_dev_f64(*obs, 0, inc, d_rays, n, d_pol, None)) for who, lib in libs]
        models = {}
        for kind in ("thermal", "table"):
            for ne in (256, 512, 1024):
                m = models[(kind, ne)] = model(kind, ne)
                tag = f"{kind} ne={ne}"
                passes += [(f"kr_post_spectrum_stokes_dev_f64 {tag}", (kind, ne),
                            lambda m=m: L.kr_post_spectrum_stokes_dev_f64(*obs, 0, -pi, pi, inc, C.byref(m), C.byref(limb1), C.byref(pol1), d_rays, n, d_out, None)),
                           (f"kr_reduce_spectrum_stokes_dev_f64 {tag}", (kind, ne),
                            lambda m=m: L.kr_reduce_spectrum_stokes_dev_f64(*obs, inc, C.byref(m), C.byref(limb1), C.byref(pol1), d_rays, n, d_out, None))]
                for who, lib in libs:
                    passes += [(f"kr_post_spectrum_dev_f64 ({who}) {tag}", (kind, ne),
                                lambda m=m, lib=lib: lib.kr_post_spectrum_dev_f64(*obs, 0, -pi, pi, C.byref(m), C.byref(limb1), d_rays, n, d_out, None)),
                               (f"kr_reduce_spectrum_dev_f64 ({who}) {tag}", (kind, ne), lambda m=m, lib=lib: lib.kr_reduce_spectrum_dev_f64(C.byref(m), d_rays, n, d_out, None))]
                for vt, v in var.items():
                    passes += [(f"{LABEL[vt]}, fused {tag}", (kind, ne),
                                lambda m=m, v=v: v.variant_post_spectrum_stokes(*obs, -pi, pi, inc, C.byref(m), C.byref(limb1), C.byref(pol1), d_rays, n, d_out))]
                    if vt != "framefirst":                                        # (the reduce form has no frame_value to replace)
                        passes += [(f"{LABEL[vt]}, reduce {tag}", (kind, ne),
                                    lambda m=m, v=v: v.variant_reduce_spectrum_stokes(*obs, inc, C.byref(m), C.byref(limb1), C.byref(pol1), d_rays, n, d_out))]
        # the tallies of one launch per model, and every variant's words against the library's (the same rule on the same records)
        tallies, agree = {}, {}
        for key, m in models.items():
            nw, ne = api.spectrum_stokes_words(m), m.ne
            words = np.zeros(nw)
            forms = [("lib fused", lambda: L.kr_post_spectrum_stokes_dev_f64(*obs, 0, -pi, pi, inc, C.byref(m), C.byref(limb1), C.byref(pol1), d_rays, n, d_out, None)),
                     ("lib reduce", lambda: L.kr_reduce_spectrum_stokes_dev_f64(*obs, inc, C.byref(m), C.byref(limb1), C.byref(pol1), d_rays, n, d_out, None))]
            forms += [(f"{vt} fused", lambda v=v: v.variant_post_spectrum_stokes(*obs, -pi, pi, inc, C.byref(m), C.byref(limb1), C.byref(pol1), d_rays, n, d_out)) for vt, v in var.items()]
            forms += [(f"{vt} reduce", lambda v=v: v.variant_reduce_spectrum_stokes(*obs, inc, C.byref(m), C.byref(limb1), C.byref(pol1), d_rays, n, d_out)) for vt, v in var.items()]
            for slot, fn in forms:
                capi.check(L, L.kr_memset(d_out, 0, max_words * 8), "kr_memset")
                assert fn() == 0
                capi.check(L, L.kr_synchronize(None), "sync")
                capi.check(L, L.kr_memcpy_d2h(words.ctypes.data_as(vp), d_out, words.nbytes), "d2h")
                if slot == "lib fused":
                    tallies[key], lib_words = [int(w) for w in words[-4:-1]], words.copy()
                    top = np.concatenate([np.abs(words[:ne]), np.full(2 * ne, np.hypot(words[ne:2 * ne], words[2 * ne:3 * ne]).max())])
                else:
                    assert np.array_equal(words[-4:], lib_words[-4:]), (slot, key)
                    agree[f"{slot} {key[0]} ne={key[1]}"] = float((np.abs(words[:-4] - lib_words[:-4]) / top).max())
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
                row["pairs"] = tallies[key][1] * key[1]
            rows.append(row)
    finally:
        for d, _ in sizes:
            if d:
                L.kr_free(d)
    print(json.dumps({"plane": args.plane, "records": int(n), "trace_kernel_ms": st.kernel_ms, "parent_lib": bool(parent),
                      "on_disc_used_bad_pol": {f"{k[0]} ne={k[1]}": v for k, v in tallies.items()},
                      "others_minus_library_maxnorm": agree, "worst_others_minus_library": max(agree.values()), "launches": args.launches, "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
