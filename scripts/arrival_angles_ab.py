"""What the disc-frame angle passes cost on the device, against the passes they extend, on traced records that stay in HBM:

  plane   a 4097 x 4097 image plane at 80 degrees (dist 10000, +-30, a = 0.998), RK4: kr_redshift_dev_f64, kr_angles_dev_f64, kr_post_line_dev_f64 and
          kr_post_line_limb_dev_f64 at each law (90 energy bins, no time axis)
  lamp    ~1e7 rays of the lamp post (source (0, 10, 1e-3, 1.5707), a = 0.998), RK4: kr_redshift_dev_f64, kr_angles_dev_f64, kr_post_emissivity_dev_f64
          and kr_post_emissivity_mu_dev_f64 (100 radial x 10 mu bins)

  python scripts/arrival_angles_ab.py [--plane 4097] [--rays 1e7] [--launches 20] [--warmups 3]

Every figure: device events (hipEventRecord either side of ONE launch on the null stream) around each of --launches launches after --warmups warm-ups, the
passes of a workload taken in turn within every round so that a drift of the clock meets them all alike; median, min and max in ms, the median as
bytes moved per second (the records a pass reads, 144 B each, plus what it writes per record: 8 B the redshift passes, 16 B the angle pass) and, for
the fused passes, as a ratio to their parent pass and to parent + kr_angles_dev_f64 run separately.  The redshift passes rewrite rays[].redshift and
the wrapped phi with the values they already hold after the first launch, so every launch sees the same records.  Prints one JSON object.
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

vp = C.c_void_p


class Events:
    """hipEvent timing through the HIP runtime that libkrtrace.so itself is linked against (already loaded: the same instance)."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so.7")
        self.e0, self.e1 = vp(), vp()
        for e in (self.e0, self.e1):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time_ms(self, launch):
        assert self.hip.hipEventRecord(self.e0, None) == 0
        rc = launch()
        assert self.hip.hipEventRecord(self.e1, None) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        assert rc == capi.KR_OK, rc
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return float(ms.value)


def lamp(rays):
    s = capi.PointSourceSpec()
    for i, v in enumerate((0.0, 10.0, 1e-3, 1.5707)):
        s.pos[i] = v
    d = math.sqrt(1.99 * 2 * math.pi / rays)
    s.V, s.spin, s.tol, s.E = 0.0, 0.998, 100.0, 1.0
    s.cosalpha0, s.cosalphamax, s.dcosalpha = -0.995, 0.995, d
    s.beta0, s.betamax, s.dbeta = -math.pi, math.pi, d
    return s


def plane(n_side):
    s = capi.ImagePlaneSpec()
    s.dist, s.inc_deg, s.x0, s.xmax, s.y0, s.ymax = 10000.0, 80.0, -30.0, 30.0, -30.0, 30.0
    s.dx = s.dy = 60.0 / (n_side - 1)
    s.spin, s.phi0, s.precision = 0.998, 0.0, 100.0
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane", type=int, default=4097)
    ap.add_argument("--rays", type=float, default=1e7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    args = ap.parse_args()
    L = capi.load()
    if L.kr_device_count() <= 0:
        sys.exit("arrival_angles_ab: no HIP device (there is no CPU path to time)")
    capi.check(L, L.kr_configure_process(), "kr_configure_process")
    ev = Events()
    spin, pi = 0.998, math.pi
    r_isco = L.kr_kerr_isco(spin, 1)
    res = {"library": os.environ.get("KRTRACE_LIB", capi.LIB_PATH), "launches": args.launches, "warmups": args.warmups, "workloads": []}

    ip, ps = plane(args.plane), lamp(args.rays)
    lb = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=r_isco, r_disc=30.0)
    eb = capi.EmisBins()
    eb.r_isco = eb.r_min = r_isco
    eb.nr, eb.logbin, eb.gamma, eb.spin = 100, 1, 2.0, spin
    eb.dr = math.exp(math.log(500.0 / r_isco) / eb.nr)
    eb.num_primary_rays = float(int(((ps.cosalphamax - ps.cosalpha0) / ps.dcosalpha) * ((ps.betamax - ps.beta0) / ps.dbeta)))
    mb = capi.MuBins(10, 0)
    laws = [capi.limb_law((law, 2.06)) for law in (0, 1, 2)]

    for name in ("plane", "lamp"):
        if name == "plane":
            n = L.kr_imageplane_count(C.byref(ip), None, None)
            p = capi.copy_params(capi.default_params(-spin), integrator=capi.RK4, flags=capi.FLAG_HYBRID, r_max=11000.0, theta_max=pi / 2)
            obs = (-spin, -1.0, 1, 0)
        else:
            n = L.kr_pointsource_count(C.byref(ps), None, None)
            p = capi.copy_params(capi.default_params(spin), integrator=capi.RK4, flags=capi.FLAG_HYBRID, r_max=1000.0, theta_max=pi / 2)
            obs = (spin, -1.0, 0, 0)
        words = max(2 * lb.nt * lb.ne + 3, 5 * eb.nr + 1)
        mu_words = (2 * mb.nmu + 1) * eb.nr + 3
        d_rays, d_angles, d_hist, d_mu = vp(), vp(), vp(), vp()
        try:
            capi.check(L, L.kr_malloc(C.byref(d_rays), n * 144), "kr_malloc")
            capi.check(L, L.kr_malloc(C.byref(d_angles), n * 16), "kr_malloc")
            capi.check(L, L.kr_malloc(C.byref(d_hist), words * 8), "kr_malloc")
            capi.check(L, L.kr_malloc(C.byref(d_mu), mu_words * 8), "kr_malloc")
            capi.check(L, L.kr_memset(d_hist, 0, words * 8), "kr_memset")
            capi.check(L, L.kr_memset(d_mu, 0, mu_words * 8), "kr_memset")
            st = capi.Stats()
            if name == "plane":
                capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(ip), 0, 1, 0.0, 1, 0, d_rays, n, None), "init")
            else:
                capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(ps), 0, 1, 0.0, 0, 0, d_rays, n, None), "init")
            capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "trace")
            passes = [("kr_redshift_dev_f64", 152, lambda: L.kr_redshift_dev_f64(*obs, 0, d_rays, n, None)),
                      ("kr_angles_dev_f64", 160, lambda: L.kr_angles_dev_f64(*obs, 0, d_rays, n, d_angles, None))]
            if name == "plane":
                passes.append(("kr_post_line_dev_f64", 152, lambda: L.kr_post_line_dev_f64(*obs, 0, -pi, pi, C.byref(lb), d_rays, n, d_hist, None)))
                for law in laws:
                    passes.append((f"kr_post_line_limb_dev_f64 law {law.law}", 152,
                                   lambda law=law: L.kr_post_line_limb_dev_f64(*obs, 0, -pi, pi, C.byref(lb), C.byref(law), d_rays, n, d_hist, None)))
                parent = "kr_post_line_dev_f64"
            else:
                passes.append(("kr_post_emissivity_dev_f64", 152, lambda: L.kr_post_emissivity_dev_f64(*obs, 0, -pi, pi, C.byref(eb), d_rays, n, d_hist, None)))
                passes.append(("kr_post_emissivity_mu_dev_f64 100 x 10", 152,
                               lambda: L.kr_post_emissivity_mu_dev_f64(*obs, 0, -pi, pi, C.byref(eb), C.byref(mb), d_rays, n, d_hist, d_mu, None)))
                parent = "kr_post_emissivity_dev_f64"
            ms = {k: [] for k, _, _ in passes}
            for rnd in range(args.warmups + args.launches):
                for k, _, launch in passes:
                    t = ev.time_ms(launch)
                    if rnd >= args.warmups:
                        ms[k].append(t)
            row = {"workload": name, "rays": int(n), "rays_traced": int(st.rays_traced), "trace_kernel_ms": st.kernel_ms, "passes": {}}
            for k, bytes_per_ray, _ in passes:
                med = statistics.median(ms[k])
                row["passes"][k] = {"median_ms": med, "min_ms": min(ms[k]), "max_ms": max(ms[k]), "bytes_per_ray": bytes_per_ray,
                                    "GB_per_s": n * bytes_per_ray / med / 1e6}
            sep = row["passes"][parent]["median_ms"] + row["passes"]["kr_angles_dev_f64"]["median_ms"]
            for k in row["passes"]:
                if k.startswith(("kr_post_line_limb", "kr_post_emissivity_mu")):
                    row["passes"][k]["ratio_to_parent"] = row["passes"][k]["median_ms"] / row["passes"][parent]["median_ms"]
                    row["passes"][k]["ratio_to_parent_plus_angles"] = row["passes"][k]["median_ms"] / sep
            res["workloads"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        finally:
            L.kr_synchronize(None)
            for d in (d_rays, d_angles, d_hist, d_mu):
                if d.value:
                    L.kr_free(d)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
