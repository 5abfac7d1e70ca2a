"""What the disc flow KR_V_PLUNGE costs on the device, and that V = -1 costs what it did: a 4097 x 4097 image plane at a = 0.5 seen at 60 degrees
(dist 1000, +-20: a real share of the disc rays ends inside the ISCO at 4.23), RK4, traced once; the records stay in HBM.  Then, launch by launch,

  kr_redshift_dev_f64          streaming: 144 B read and 8 B written per record
  kr_angles_dev_f64            streaming: 144 B read and 16 B written per record
  kr_post_line_limb_dev_f64    the limb-darkened line, 90 energy bins
  kr_post_spectrum_dev_f64     the table model, 256 energies
  kr_post_response_dev_f64     the same table, 256 energies x 64 time rows

each with V = -1 (inner edge r_ms) and, where the library knows it, with V = KR_V_PLUNGE (inner edge 1.02 r_h).

  python scripts/plunge_ab.py --parent path/to/parent/libkrtrace.so [--limit 200] [--plane 4097] [--launches 10] [--warmups 3]
  python scripts/plunge_ab.py [--lib path/to/libkrtrace.so] [--label name] [--plane 4097] [--launches 10] [--warmups 3]

--parent: the library built from the parent commit.  The script then measures three times, each in a child process of its own under
`timeout -k 10 <limit>` (one library per process; a step that fails or runs into its limit ends the run, nothing more is started on the device): the
parent, this tree's library, the parent again -- the two parent runs give the parent's own run-to-run spread -- and prints the table of
profiles/plunge_ab.txt.  Without --parent: one measurement of --lib (default: this tree's library) in this process, one JSON object; run it under a
`timeout` of its own.  Every figure: the host clock
around ONE launch and kr_synchronize on the null stream (the passes take milliseconds, a launch and a sync some ten microseconds), --launches launches
after --warmups warm-ups, the passes taken in turn within every round so that a drift of the clock meets them all alike; median, min and max in ms,
and the achieved bytes per second of the two streaming passes.  The fused passes rewrite rays[].redshift and the wrapped phi from fields they leave
alone, so every launch sees the same geodesics; the histograms only accumulate.  Prints one JSON object."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytrace_cpu_amd import capi  # noqa: E402

PI = math.pi
SPIN, INCL, DIST, HALF = 0.5, 60.0, 1000.0, 20.0
V_PLUNGE = -2.0


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


def compare(a):
    """The three measurements, each a child under its own time limit, and the table."""
    rows = []
    for label, lib in (("parent", a.parent), ("this", capi.LIB_PATH), ("parent, again", a.parent)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--lib", lib, "--label", label, "--plane", str(a.plane), "--launches",
               str(a.launches), "--warmups", str(a.warmups)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"{label}: exit status {r.returncode}; nothing more is started")
            return r.returncode
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    P, T, P2 = rows

    def cell(r):
        return f"{r['median']:.4f} ({r['min']:.4f} ... {r['max']:.4f})"

    print(f"{T['records']} records; {a.warmups} warm-ups, then {a.launches} launches per pass, the passes taken in turn; ms, median (min ... max)")
    print(f"{'pass':12s} {'parent V=-1':>26s} {'parent V=-1, again':>26s} {'this V=-1':>26s} {'this V=-2':>26s} {'V=-2 / V=-1':>12s}")
    for name in ("redshift", "angles", "limb line", "spectrum", "response"):
        p1, p2, t1, t2 = P["ms"][name + " V=-1"], P2["ms"][name + " V=-1"], T["ms"][name + " V=-1"], T["ms"][name + " V=-2"]
        print(f"{name:12s} {cell(p1):>26s} {cell(p2):>26s} {cell(t1):>26s} {cell(t2):>26s} {t2['median'] / t1['median']:12.3f}")
    for name in ("redshift", "angles"):
        print(f"  {name:9s} GB/s: parent V=-1 {P['ms'][name + ' V=-1']['GB_per_s']:.0f} / {P2['ms'][name + ' V=-1']['GB_per_s']:.0f}   this V=-1 "
              f"{T['ms'][name + ' V=-1']['GB_per_s']:.0f}   this V=-2 {T['ms'][name + ' V=-2']['GB_per_s']:.0f}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=capi.LIB_PATH)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--plane", type=int, default=4097)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--limit", type=int, default=200)
    a = ap.parse_args()
    if a.parent:
        return compare(a)
    lib = load(a.lib)
    knows_plunge = hasattr(lib, "kr_plunge_flow")
    r_h, r_ms = lib.kr_kerr_horizon(SPIN), lib.kr_kerr_isco(SPIN, 1)

    spec = capi.ImagePlaneSpec()
    d = 2 * HALF / (a.plane - 1)
    spec.dist, spec.inc_deg, spec.x0, spec.xmax, spec.dx, spec.y0, spec.ymax, spec.dy = DIST, INCL, -HALF, HALF, d, -HALF, HALF, d
    spec.spin, spec.phi0, spec.precision = SPIN, 0.0, 100.0
    n = lib.kr_imageplane_count(C.byref(spec), None, None)
    p = capi.default_params(-SPIN)
    p.precision, p.integrator, p.theta_max, p.r_max, p.stop_kind, p.flags = 100.0, capi.RK4, PI / 2, 1.1 * DIST, capi.STOP_THETA, capi.FLAG_HYBRID

    def dev(nbytes, zero=True):
        ptr = C.c_void_p()
        check(lib, lib.kr_malloc(C.byref(ptr), nbytes), "kr_malloc")
        if zero:
            check(lib, lib.kr_memset(ptr, 0, nbytes), "kr_memset")
        return ptr

    rays = dev(n * 144, zero=False)
    check(lib, lib.kr_imageplane_init_emit_dev_f64(C.byref(spec), 0, 1, 0.0, 1, 0, rays, n, None), "init")
    st = capi.Stats()
    check(lib, lib.kr_trace_dev_f64(C.byref(p), rays, n, None, C.byref(st)), "trace")

    law = capi.limb_law("laor")
    s_de, S = table()
    ne = 256
    passes = {}
    for V in (-1.0, V_PLUNGE) if knows_plunge else (-1.0,):
        edge = r_ms if V == -1.0 else 1.02 * r_h
        tag = "V=-1" if V == -1.0 else "V=-2"
        lb = capi.line_bins(line_energy=6.4, e_min=0.05, de=1.1, ne=90, log_e=True, r_isco=edge, r_disc=HALF)
        m = capi.spectrum_model("table", 0.05, math.exp(math.log(100.0 / 0.05) / ne), ne, log_e=True, r_isco=edge, r_disc=HALF, s=S, s_e_min=0.05, s_de=s_de)
        R = capi.response_model(m, DIST - 50.0, 2.0, 64)
        angles, line = dev(n * 16, zero=False), dev((2 * 90 + 3) * 8)
        spectrum, response = dev((ne + 4) * 8), dev((64 * ne + 4) * 8)
        keep = [lb, m, R]
        passes[f"redshift {tag}"] = (lambda V=V: lib.kr_redshift_dev_f64(-SPIN, V, 1, 0, 0, rays, n, None), 152)
        passes[f"angles {tag}"] = (lambda V=V, o=angles: lib.kr_angles_dev_f64(-SPIN, V, 1, 0, 0, rays, n, o, None), 160)
        passes[f"limb line {tag}"] = (lambda V=V, b=lb, o=line: lib.kr_post_line_limb_dev_f64(-SPIN, V, 1, 0, 0, -PI, PI, C.byref(b), C.byref(law), rays, n, o, None), 0)
        passes[f"spectrum {tag}"] = (lambda V=V, b=m, o=spectrum: lib.kr_post_spectrum_dev_f64(-SPIN, V, 1, 0, 0, -PI, PI, C.byref(b), C.byref(law), rays, n, o, None), 0)
        passes[f"response {tag}"] = (lambda V=V, b=R, o=response: lib.kr_post_response_dev_f64(-SPIN, V, 1, 0, 0, -PI, PI, C.byref(b), C.byref(law), rays, n, o, None), 0)
        passes[f"_keep {tag}"] = keep
    runs = {k: v for k, v in passes.items() if not k.startswith("_keep")}
    times = {k: [] for k in runs}
    check(lib, lib.kr_synchronize(None), "sync")
    for rnd in range(a.warmups + a.launches):
        for k, (call, _) in runs.items():
            t0 = time.perf_counter()
            check(lib, call(), k)
            check(lib, lib.kr_synchronize(None), "sync")
            if rnd >= a.warmups:
                times[k].append((time.perf_counter() - t0) * 1e3)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    out = {"label": a.label, "commit_of_the_tree": commit, "records": int(n), "rays_traced": int(st.rays_traced), "launches": a.launches, "warmups": a.warmups, "ms": {}}
    for k, ts in times.items():
        row = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
        if runs[k][1]:
            row["GB_per_s"] = round(n * runs[k][1] / (statistics.median(ts) * 1e-3) / 1e9, 1)
        out["ms"][k] = row
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
