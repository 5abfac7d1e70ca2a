"""What the disc-surface passes cost on the device, and that the flat passes cost what they did: the 4097 x 4097 image plane of scripts/plunge_ab.py
(a = 0.5 seen at 60 degrees, dist 1000, +-20), RK4, traced twice into two record buffers that stay in HBM: once to the equatorial plane and once to the
surface H = 0.1 rho between the ISCO and 20 (KR_STOP_THICKDISC).  Then, launch by launch,

  on the surface records    kr_post_image_surface_dev_f64 (the surface pass that existed), kr_angles_surface_dev_f64, kr_post_line_surface_dev_f64 (90 bins),
                            kr_post_spectrum_surface_dev_f64 (table model, 256 energies), kr_post_response_surface_dev_f64 (the same, x 64 time rows)
  on the flat records       their flat twins from this tree's library: kr_angles_dev_f64, kr_post_line_limb_dev_f64, kr_post_spectrum_dev_f64,
                            kr_post_response_dev_f64 -- the same record count, another share of it on the disc (printed)
  with --free-angles        kr_angles_surface_dev_f64 from a build without the kernel's second launch bound (-DKR_ANGLES_SURFACE_FREE)
  with --parent             the same four flat passes from the parent commit's library, loaded beside this tree's in the same process and taken in turn
                            with it, round by round, on the same flat records

  timeout -k 10 600 python scripts/surface_pass_ab.py [--parent path/to/parent/libkrtrace.so] [--plane 4097] [--launches 10] [--warmups 3]

Every figure: the host clock around ONE launch and kr_synchronize on the null stream (the passes take milliseconds, a launch and a sync some ten
microseconds), --launches launches after --warmups warm-ups, the passes taken in turn within every round so that a drift of the clock meets them all
alike; median, min and max in ms.  The fused passes rewrite rays[].redshift and the wrapped phi from fields they leave alone, so every launch sees the
same geodesics; the histograms only accumulate.  The run-to-run scatter the table reports is that of the repeated launches themselves, (max - min) /
median.  Prints the table of profiles/surface_pass_ab.txt."""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytrace_cpu_amd import capi  # noqa: E402

PI = math.pi
SPIN, INCL, DIST, HALF = 0.5, 60.0, 1000.0, 20.0


def load(path):
    """The library at `path` with the prototypes of capi for every symbol it has (an older build lacks the newest)."""
    lib = C.CDLL(path)
    for name, (res, args) in capi.PROTOTYPES.items():
        if hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
    return lib


def check(lib, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {rc} {lib.kr_last_error().decode()}")


def table(nz=2, s_ne=300, s_e_min=0.05, s_e_max=500.0):
    s_de = math.exp(math.log(s_e_max / s_e_min) / (s_ne - 1))
    e = s_e_min * s_de ** np.arange(s_ne)
    return s_de, np.array([e ** -(1.6 + 0.2 * z) * np.exp(-e / 100.0) for z in range(nz)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--free-angles", default=None, help="a build of this tree with -DKR_ANGLES_SURFACE_FREE (_build.build(extra_flags=..., tag=...)): its kr_angles_surface_dev_f64 is timed too")
    ap.add_argument("--plane", type=int, default=4097)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=3)
    a = ap.parse_args()
    lib = load(capi.LIB_PATH)
    parent = load(a.parent) if a.parent else None
    free = load(a.free_angles) if a.free_angles else None
    r_ms = lib.kr_kerr_isco(SPIN, 1)

    spec = capi.ImagePlaneSpec()
    d = 2 * HALF / (a.plane - 1)
    spec.dist, spec.inc_deg, spec.x0, spec.xmax, spec.dx, spec.y0, spec.ymax, spec.dy = DIST, INCL, -HALF, HALF, d, -HALF, HALF, d
    spec.spin, spec.phi0, spec.precision = SPIN, 0.0, 100.0
    n = lib.kr_imageplane_count(C.byref(spec), None, None)
    flat_p = capi.default_params(-SPIN)
    flat_p.precision, flat_p.integrator, flat_p.theta_max, flat_p.r_max, flat_p.stop_kind, flat_p.flags = 100.0, capi.RK4, PI / 2, 1.1 * DIST, capi.STOP_THETA, capi.FLAG_HYBRID
    surface = capi.disc_surface((r_ms, HALF, 0.1, 0.0))
    thick_p = capi.copy_params(flat_p, stop_kind=capi.STOP_THICKDISC, stop_params=(r_ms, HALF, 0.1, 0.0))

    def dev(nbytes, zero=True):
        ptr = C.c_void_p()
        check(lib, lib.kr_malloc(C.byref(ptr), nbytes), "kr_malloc")
        if zero:
            check(lib, lib.kr_memset(ptr, 0, nbytes), "kr_memset")
        return ptr

    records = {}
    for tag, p in (("flat", flat_p), ("surface", thick_p)):
        rays = dev(n * 144, zero=False)
        check(lib, lib.kr_imageplane_init_emit_dev_f64(C.byref(spec), 0, 1, 0.0, 1, 0, rays, n, None), "init")
        st = capi.Stats()
        check(lib, lib.kr_trace_dev_f64(C.byref(p), rays, n, None, C.byref(st)), f"trace {tag}")
        records[tag] = rays

    law = capi.limb_law("laor")
    s_de, S = table()
    ne = 256
    lb = capi.line_bins(line_energy=6.4, e_min=0.05, de=1.1, ne=90, log_e=True, r_isco=r_ms, r_disc=HALF)
    m = capi.spectrum_model("table", 0.05, math.exp(math.log(100.0 / 0.05) / ne), ne, log_e=True, r_isco=r_ms, r_disc=HALF, s=S, s_e_min=0.05, s_de=s_de)
    R = capi.response_model(m, DIST - 50.0, 2.0, 64)
    ib = capi.ImageBins()
    ib.x0, ib.y0, ib.img_dx, ib.img_dy, ib.r_isco, ib.r_disc = -HALF, -HALF, 2 * HALF / 1024, 2 * HALF / 1024, r_ms, HALF
    ib.q1, ib.rb1, ib.q2, ib.rb2, ib.q3, ib.img_nx, ib.img_ny, ib.flip_image, ib.pad = 3.0, 4.0, 3.0, 10.0, 3.0, 1024, 1024, 1, 0

    def buffers():
        return dict(angles=dev(n * 16, zero=False), line=dev((2 * 90 + 3) * 8), spectrum=dev((ne + 4) * 8), response=dev((64 * ne + 4) * 8))

    fr, sr_ = records["flat"], records["surface"]
    passes = {}
    o = o_surface = buffers()
    planes = dev((7 * 1024 * 1024 + 1) * 8)
    passes["image    surface"] = lambda: lib.kr_post_image_surface_dev_f64(-SPIN, 1, -PI, PI, C.byref(ib), sr_, n, planes, None)
    passes["angles   surface"] = lambda o=o: lib.kr_angles_surface_dev_f64(C.byref(surface), -SPIN, 1, sr_, n, o["angles"], None)
    passes["line     surface"] = lambda o=o: lib.kr_post_line_surface_dev_f64(C.byref(surface), -SPIN, 1, -PI, PI, C.byref(lb), C.byref(law), sr_, n, o["line"], None)
    passes["spectrum surface"] = lambda o=o: lib.kr_post_spectrum_surface_dev_f64(C.byref(surface), -SPIN, 1, -PI, PI, C.byref(m), C.byref(law), sr_, n, o["spectrum"], None)
    passes["response surface"] = lambda o=o: lib.kr_post_response_surface_dev_f64(C.byref(surface), -SPIN, 1, -PI, PI, C.byref(R), C.byref(law), sr_, n, o["response"], None)
    if free is not None:
        passes["angles   surface, no wave bound"] = lambda o=o: free.kr_angles_surface_dev_f64(C.byref(surface), -SPIN, 1, sr_, n, o["angles"], None)
    o_flat = None
    for tag, L in (("this", lib), ("parent", parent)):
        if L is None:
            continue
        o = buffers()
        o_flat = o_flat or o
        passes[f"angles   flat {tag}"] = lambda L=L, o=o: L.kr_angles_dev_f64(-SPIN, -1.0, 1, 0, 0, fr, n, o["angles"], None)
        passes[f"line     flat {tag}"] = lambda L=L, o=o: L.kr_post_line_limb_dev_f64(-SPIN, -1.0, 1, 0, 0, -PI, PI, C.byref(lb), C.byref(law), fr, n, o["line"], None)
        passes[f"spectrum flat {tag}"] = lambda L=L, o=o: L.kr_post_spectrum_dev_f64(-SPIN, -1.0, 1, 0, 0, -PI, PI, C.byref(m), C.byref(law), fr, n, o["spectrum"], None)
        passes[f"response flat {tag}"] = lambda L=L, o=o: L.kr_post_response_dev_f64(-SPIN, -1.0, 1, 0, 0, -PI, PI, C.byref(R), C.byref(law), fr, n, o["response"], None)

    times = {k: [] for k in passes}
    check(lib, lib.kr_synchronize(None), "sync")
    for rnd in range(a.warmups + a.launches):
        for k, call in passes.items():
            t0 = time.perf_counter()
            check(lib, call(), k)
            check(lib, lib.kr_synchronize(None), "sync")
            if rnd >= a.warmups:
                times[k].append((time.perf_counter() - t0) * 1e3)

    # the share of the records on the disc, from the tallies the line passes accumulated (on_disc is the first word after the 2 x 90 bins)
    def on_disc(ptr):
        words = np.zeros(2 * 90 + 3)
        check(lib, lib.kr_memcpy_d2h(words.ctypes.data_as(C.c_void_p), ptr, words.nbytes), "d2h")
        return words[180] / (a.warmups + a.launches)

    print(f"on the disc per launch: {on_disc(o_flat['line']):.0f} of the flat records, {on_disc(o_surface['line']):.0f} of the surface records")
    print(f"{n} records per buffer; {a.warmups} warm-ups, then {a.launches} launches per pass, the passes taken in turn; ms, median (min ... max), scatter = (max - min) / median")
    for k, ts in times.items():
        med = statistics.median(ts)
        print(f"{k:24s} {med:9.4f} ({min(ts):.4f} ... {max(ts):.4f})   scatter {100 * (max(ts) - min(ts)) / med:5.2f} %")
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for name in ("angles  ", "line    ", "spectrum", "response"):
        row = f"{name}: surface / flat {med[name + ' surface'] / med[name + ' flat this']:.3f}   surface / image surface {med[name + ' surface'] / med['image    surface']:.3f}"
        if parent is not None:
            row += f"   flat this / flat parent {med[name + ' flat this'] / med[name + ' flat parent']:.4f}"
        print(row)
    return 0


if __name__ == "__main__":
    sys.exit(main())
