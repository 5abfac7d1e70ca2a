"""What the polarisation passes cost on the device, against the passes they extend, on traced records that stay in HBM: a 4097 x 4097 image plane at
80 degrees (dist 10000, +-30, a = 0.998), RK4, traced once; then, launch by launch,

  kr_polarisation_dev_f64                                    144 B read + 32 B written per record
  kr_post_image_dev_f64                                      the parent of the Stokes image (4096 x 4096 pixels, seven planes)
  kr_post_image_stokes_dev_f64                               pol law 1 (0.1171), limb law 0 and 1
  kr_post_line_limb_dev_f64, kr_post_line_stokes_dev_f64     90 energy bins, no time axis, limb law 1

  python scripts/polarisation_ab.py [--plane 4097] [--pixels 4096] [--launches 20] [--warmups 3]

Every figure: device events (hipEventRecord either side of ONE launch on the null stream) around each of --launches launches after --warmups warm-ups, the
passes taken in turn within every round so that a drift of the clock meets them all alike; median, min and max in ms, the median as bytes of records
and per-record output moved per second (the planes' atomics are not counted), and for the fused passes as a ratio to their parent pass and to parent +
kr_polarisation_dev_f64 run separately.  The passes rewrite rays[].redshift and the wrapped phi with the values they already hold after the first
launch, so every launch sees the same records; the planes and histograms only accumulate.  Prints one JSON object.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytrace_cpu_amd import capi  # noqa: E402
from scripts.arrival_angles_ab import Events, plane  # noqa: E402

vp = C.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane", type=int, default=4097)
    ap.add_argument("--pixels", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    args = ap.parse_args()
    L = capi.load()
    if L.kr_device_count() <= 0:
        sys.exit("polarisation_ab: no HIP device (there is no CPU path to time)")
    capi.check(L, L.kr_configure_process(), "kr_configure_process")
    ev = Events()
    spin, pi, inc = 0.998, math.pi, 80.0
    r_isco = L.kr_kerr_isco(spin, 1)
    ip = plane(args.plane)
    n = L.kr_imageplane_count(C.byref(ip), None, None)
    ib = capi.ImageBins()
    ib.x0 = ib.y0 = -30.0
    ib.img_dx = ib.img_dy = 60.0 / args.pixels
    ib.r_isco, ib.r_disc = r_isco, 30.0
    ib.q1, ib.rb1, ib.q2, ib.rb2, ib.q3 = 3.0, 4.0, 3.0, 10.0, 3.0
    ib.img_nx = ib.img_ny = args.pixels
    ib.flip_image = 1
    npix = args.pixels * args.pixels
    lb = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=r_isco, r_disc=30.0)
    limb0, limb1, pol = capi.limb_law((0, 0.0)), capi.limb_law((1, 2.06)), capi.pol_law((1, 0.1171))
    p = capi.copy_params(capi.default_params(-spin), integrator=capi.RK4, flags=capi.FLAG_HYBRID, r_max=11000.0, theta_max=pi / 2)
    obs = (-spin, -1.0, 1, 0)

    d_rays, d_out, d_planes, d_stokes, d_line = vp(), vp(), vp(), vp(), vp()
    sizes = [(d_rays, n * 144), (d_out, n * 32), (d_planes, (7 * npix + 1) * 8), (d_stokes, (4 * npix + 2) * 8), (d_line, (4 * lb.ne + 3) * 8)]
    try:
        for d, nbytes in sizes:
            capi.check(L, L.kr_malloc(C.byref(d), nbytes), "kr_malloc")
            capi.check(L, L.kr_memset(d, 0, nbytes), "kr_memset")
        st = capi.Stats()
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(ip), 0, 1, 0.0, 1, 0, d_rays, n, None), "init")
        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "trace")
        image, line = "kr_post_image_dev_f64", "kr_post_line_limb_dev_f64 limb 1"
        passes = [
            ("kr_polarisation_dev_f64", 176, None, lambda: L.kr_polarisation_dev_f64(*obs, 0, inc, d_rays, n, d_out, None)),
            (image, 152, None, lambda: L.kr_post_image_dev_f64(*obs, 0, -pi, pi, C.byref(ib), d_rays, n, d_planes, None)),
            ("kr_post_image_stokes_dev_f64 limb 0", 152, image,
             lambda: L.kr_post_image_stokes_dev_f64(*obs, 0, -pi, pi, inc, C.byref(ib), C.byref(limb0), C.byref(pol), d_rays, n, d_stokes, None)),
            ("kr_post_image_stokes_dev_f64 limb 1", 152, image,
             lambda: L.kr_post_image_stokes_dev_f64(*obs, 0, -pi, pi, inc, C.byref(ib), C.byref(limb1), C.byref(pol), d_rays, n, d_stokes, None)),
            (line, 152, None, lambda: L.kr_post_line_limb_dev_f64(*obs, 0, -pi, pi, C.byref(lb), C.byref(limb1), d_rays, n, d_line, None)),
            ("kr_post_line_stokes_dev_f64 limb 1", 152, line,
             lambda: L.kr_post_line_stokes_dev_f64(*obs, 0, -pi, pi, inc, C.byref(lb), C.byref(limb1), C.byref(pol), d_rays, n, d_line, None)),
        ]
        ms = {k: [] for k, *_ in passes}
        for rnd in range(args.warmups + args.launches):
            for k, _, _, launch in passes:
                t = ev.time_ms(launch)
                if rnd >= args.warmups:
                    ms[k].append(t)
        res = {"library": os.environ.get("KRTRACE_LIB", capi.LIB_PATH), "launches": args.launches, "warmups": args.warmups, "rays": int(n), "rays_traced": int(st.rays_traced),
               "pixels": npix, "trace_kernel_ms": st.kernel_ms, "passes": {}}
        for k, bytes_per_ray, _, _ in passes:
            med = statistics.median(ms[k])
            res["passes"][k] = {"median_ms": med, "min_ms": min(ms[k]), "max_ms": max(ms[k]), "bytes_per_ray": bytes_per_ray, "GB_per_s": n * bytes_per_ray / med / 1e6}
        per_record = res["passes"]["kr_polarisation_dev_f64"]["median_ms"]
        for k, _, parent, _ in passes:
            if parent:
                res["passes"][k]["ratio_to_parent"] = res["passes"][k]["median_ms"] / res["passes"][parent]["median_ms"]
                res["passes"][k]["ratio_to_parent_plus_polarisation"] = res["passes"][k]["median_ms"] / (res["passes"][parent]["median_ms"] + per_record)
    finally:
        L.kr_synchronize(None)
        for d, _ in sizes:
            if d.value:
                L.kr_free(d)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
