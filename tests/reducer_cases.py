"""TEST INFRASTRUCTURE: the record set and the bin structs of the reducer tests (tests/test_reducer_rules.py on the CPU, tests/test_gpu_reducers.py on
the device).  Deterministic: one default_rng seed, no trace -- the records are chosen, not computed, so that they sit where traced rays almost never do.

  bulk        4096 plausible records over and around every range the reducers test
  edges       one record per case, each otherwise "good" (on the disc, in a pixel, in a bin), so that the case alone decides the outcome
  contention  20 000 copies of one record: one bin, one pixel

Only decisions made of IEEE-exact operations sit exactly on an edge: the linear bins and the pixel quotients (x0, dx, r_min, dr are dyadic), the r
comparisons and theta >= pi/2.  What goes through cos or log may differ in the last bit between device and host, so guard_bands() asserts that no
record's z = r cos(theta) is within 1e-9 of 1e-2 and no log-bin quotient within 1e-9 of an integer (but r == r_min: log(1) = 0 is exact, bin 0).
Counts are then compared with no slack at all."""
import math

import numpy as np

import reducer_rules as rr
from raytrace_cpu_amd import capi

SEED = 20250613
R_ISCO, R_DISC, R_ESC = 1.0, 64.0, 100.0
SOURCE_R, SOURCE_PHI = 5.0, 0.25
X0 = Y0 = -4.0
R_MIN, LOG_TOP = 1.25, 50.0
N_BULK, N_CONTENTION, N_LARGE = 4096, 20000, 262144 + 321
HALF_PI = math.pi / 2
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1

EMIS_NR = (1, 4, 7, 1024, 1025, 3000)       # 4: the table of the linear rule; 1024 / 1025: either side of the LDS histogram's capacity
IMAGE_SHAPES = ((1, 1), (8, 8), (5, 13), (13, 5))
POISON_R, POISON_XY = 40.0, -3.5            # where the records with a non-finite term are put: one radial bin, one pixel


def below(x):
    return float(np.nextafter(x, -np.inf))


def above(x):
    return float(np.nextafter(x, np.inf))


# ---- the bin structs --------------------------------------------------------------------------------------------------------------------
def linear_dr(nr):
    """A dyadic width with which nr bins from R_MIN reach about R_DISC (nr = 4: the 0.25 of the table)."""
    return 0.25 if nr == 4 else 2.0 ** round(math.log2(R_DISC / nr))


def emis_bins(nr, logbin, r_min=R_MIN, dr=None):
    b = capi.EmisBins()
    b.r_min, b.r_isco, b.gamma, b.spin, b.num_primary_rays = r_min, R_ISCO, 1.7, 0.998, 1000.0
    b.dr = dr if dr is not None else (math.exp(math.log(LOG_TOP / R_MIN) / nr) if logbin else linear_dr(nr))
    b.nr, b.logbin = nr, int(logbin)
    return b


def emis_cases():
    """name -> kr_emis_bins: every nr x rule, and three sets whose quotient is NaN or infinite for every record (none may be binned, all count on the disc)."""
    c = {f"{'log' if lb else 'lin'}-nr{nr}": emis_bins(nr, lb) for nr in EMIS_NR for lb in (0, 1)}
    c["log-rmin-negative"] = emis_bins(7, 1, r_min=-1.25, dr=1.5)        # log(negative) = NaN
    c["log-rmin-zero"] = emis_bins(7, 1, r_min=0.0, dr=1.5)              # log(r / 0) = inf
    c["lin-dr-zero"] = emis_bins(7, 0, dr=0.0)                           # +-inf, and 0 / 0 = NaN at r == r_min
    return c


def image_bins(nx, ny, flip):
    b = capi.ImageBins()
    b.x0, b.y0 = X0, Y0
    b.img_dx = b.img_dy = 8.0 if (nx, ny) == (1, 1) else 1.0             # the one-pixel image covers what the 8 x 8 one does
    b.r_isco, b.r_disc = R_ISCO, R_DISC
    b.q1, b.rb1, b.q2, b.rb2, b.q3 = 3.0, 4.0, 2.5, 10.0, 3.5
    b.img_nx, b.img_ny, b.flip_image, b.pad = nx, ny, int(flip), 0
    return b


def image_cases():
    return {f"{nx}x{ny}-flip{f}": image_bins(nx, ny, f) for nx, ny in IMAGE_SHAPES for f in (0, 1)}


def return_bins(plane_iso, limb, weight_norm):
    b = capi.ReturnBins()
    b.r_isco, b.r_disc, b.r_esc, b.source_r, b.source_phi = R_ISCO, R_DISC, R_ESC, SOURCE_R, SOURCE_PHI
    b.plane_iso, b.limb, b.weight_norm, b.pad = plane_iso, limb, weight_norm, 0
    return b


def return_cases():
    return {f"iso{p}-limb{l}-norm{w}": return_bins(p, l, w) for p in (0, 1) for l in (0, 1) for w in (0, 1)}


# ---- the records ------------------------------------------------------------------------------------------------------------------------
GOOD = dict(t=10.0, r=6.0, theta=HALF_PI, phi=0.5, k=1.0, h=1.0, Q=5.0, emit=1.0, redshift=1.0, steps=5, rdot_sign=-1, thetadot_sign=1,
            alpha=0.5, beta=0.5, cosalpha=0.5)

# the two tables of the index rule: value -> what an 8 x 8 image (x0 = -4, dx = 1) / four linear bins (r_min = 1.25, dr = 0.25) make of it
PIXEL_TABLE = [(float("nan"), None), (float("inf"), None), (float("-inf"), None), (1e300, None), (-1e300, None), (2.0 ** 31 - 4, None),
               (2.0 ** 31 + 100, None), (-2.0 ** 31 - 4, None), (-4.0, 0), (-4.5, 0), (-4.999, 0), (3.999, 7), (4.0, None), (below(4.0), None),
               (-0.0, 4)]
LINEAR_TABLE = [(1.0, None), (1.2, 0), (1.25, 0), (below(1.5), 0), (1.5, 1), (below(2.25), 3), (2.25, None)]      # all on the disc


def edge_cases():
    """[(label, overrides of GOOD)]"""
    e = []
    for axis in ("alpha", "beta"):
        for v, _ in PIXEL_TABLE:
            e.append((f"{axis}={v!r}", {axis: v}))
        for top in (1.0, 9.0):                                             # the upper edges of the 5- and 13-pixel axes
            for v in (top - 1e-3, top, below(top)):
                e.append((f"{axis}={v!r}", {axis: v}))
    for v, _ in LINEAR_TABLE:
        e.append((f"r={v!r}", {"r": v}))
    for nr in EMIS_NR:                                                      # the first inner edge and the last edge of every linear histogram
        for edge in sorted({R_MIN + linear_dr(nr), R_MIN + nr * linear_dr(nr)}):
            for v in (below(edge), edge, above(edge)):
                e.append((f"r={v!r} (nr {nr})", {"r": v}))
    for name, edge in (("r_isco", R_ISCO), ("r_disc", R_DISC), ("r_esc", R_ESC)):
        for v in (below(edge), edge, above(edge)):
            for th in (HALF_PI, below(HALF_PI)):
                e.append((f"r={name}{v - edge:+.1e} theta={th!r}", {"r": v, "theta": th}))
    for th in (HALF_PI, below(HALF_PI), above(HALF_PI)):
        e.append((f"theta={th!r}", {"theta": th}))
    for g in (0.0, -0.0, float("nan"), -1.0):
        e.append((f"g={g!r}", {"redshift": g}))
    poison = {"r": POISON_R, "alpha": POISON_XY, "beta": POISON_XY}
    for g in (5e-324, float("inf")):                                       # g > 0: binned, with 1 / g or g itself infinite
        e.append((f"g={g!r}", dict(poison, redshift=g)))
    for f in ("t", "phi"):
        for v in (float("nan"), float("inf"), float("-inf")):              # binned, and the sums they enter are NaN or infinite
            e.append((f"{f}={v!r}", dict(poison, **{f: v})))
    for s in (0, -1, INT_MIN, INT_MAX):
        e.append((f"steps={s}", {"steps": s}))
    # the returning-radiation classification: |r - source_r| against 0.1 source_r and |phi - source_phi| against 0.1, the other one inside
    thr = 0.1 * SOURCE_R
    for centre in (SOURCE_R + thr, SOURCE_R - thr):
        for v in (below(centre), centre, above(centre)):
            e.append((f"r=source{v - SOURCE_R:+.17g}", {"r": v, "phi": SOURCE_PHI}))
    for centre in (SOURCE_PHI + 0.1, SOURCE_PHI - 0.1):
        for v in (below(centre), centre, above(centre)):
            e.append((f"phi=source{v - SOURCE_PHI:+.17g}", {"r": SOURCE_R, "phi": v}))
    e.append(("at the source", {"r": SOURCE_R, "phi": SOURCE_PHI}))
    for c in (1.0, -1.0, 0.0, above(1.0), float("nan")):                   # the stored cos(alpha); the last two have no acos: a NaN weight
        e.append((f"cosalpha={c!r}", {"cosalpha": c}))
    for r in (2 * R_ESC, 0.5 * R_ISCO):                                     # a NaN weight among the escaped and among the lost rays too
        e.append((f"cosalpha=nan r={r!r}", {"cosalpha": float("nan"), "r": r}))
    return e


_FIELDS = tuple(capi.RAY_F64.names)


def _records(rows):
    out = np.zeros(len(rows), dtype=capi.RAY_F64)
    cosalpha = np.zeros(len(rows))
    for i, over in enumerate(rows):
        row = dict(GOOD, **over)
        for f in _FIELDS:
            if f in row:
                out[f][i] = row[f]
        cosalpha[i] = row["cosalpha"]
    return out, cosalpha


def _bulk(rng):
    n = N_BULK
    out = np.zeros(n, dtype=capi.RAY_F64)
    out["r"] = np.exp(rng.uniform(math.log(0.5 * R_ISCO), math.log(2 * R_DISC), n))
    out["theta"] = rng.choice([HALF_PI, HALF_PI - 1e-3, HALF_PI + 1e-3, 0.3, 2.8], n, p=[0.3, 0.3, 0.3, 0.05, 0.05])
    g = np.exp(rng.uniform(math.log(1e-3), math.log(1e3), n))
    kind = rng.uniform(0, 1, n)
    out["redshift"] = np.where(kind < 0.05, 0.0, np.where(kind < 0.1, -g, g))            # a tenth of them <= 0
    out["t"], out["phi"] = rng.uniform(-50, 200, n), rng.uniform(-40, 40, n)
    out["alpha"], out["beta"] = rng.uniform(X0 - 1, X0 + 14, n), rng.uniform(Y0 - 1, Y0 + 14, n)      # the 13-pixel axis and a pixel beyond it
    out["steps"] = rng.choice([-300, -1, 0, 1, 5000], n, p=[0.05, 0.05, 0.05, 0.425, 0.425])
    out["k"], out["h"], out["Q"], out["emit"] = 1.0, rng.uniform(-3, 3, n), rng.uniform(0, 20, n), rng.uniform(0.5, 2, n)
    out["rdot_sign"], out["thetadot_sign"] = rng.choice([-1, 1], n), rng.choice([-1, 1], n)
    return out, rng.uniform(-1, 1, n)


class Records:
    """rays: the records as the emissivity and image reducers read them (alpha, beta: image coordinates); return_rays: the same with the stored
    cos(alpha) in alpha, as the returning-radiation classification reads them.  poison: records that carry a non-finite term into a sum they are
    binned in; nan_weight: records whose returning-radiation weight is NaN (no acos, or sin of an infinite beta).  labels / first_edge: the edge block."""

    def __init__(self, rays, cosalpha, labels, first_edge):
        self.rays, self.labels, self.first_edge = rays, labels, first_edge
        self.return_rays = rays.copy()
        self.return_rays["alpha"] = cosalpha
        g = rays["redshift"]
        self.poison = ~np.isfinite(rays["t"]) | ~np.isfinite(rays["phi"]) | (g == np.inf) | ((g > 0) & (g < 1e-300))
        self.nan_weight = ~np.isfinite(rr.return_weight(return_bins(1, 1, 1), self.return_rays))

    def edge(self, label):
        return self.first_edge + self.labels.index(label)

    def tiled(self, n):
        out = Records.__new__(Records)
        out.labels, out.first_edge = self.labels, self.first_edge
        for k in ("rays", "return_rays", "poison", "nan_weight"):
            setattr(out, k, np.resize(getattr(self, k), n))
        return out


_cache = {}


def small():
    """bulk + edges + contention, about 24 500 records; built once, never modified (copy before a pass that writes records)."""
    if "small" not in _cache:
        rng = np.random.default_rng(SEED)
        bulk, bulk_ca = _bulk(rng)
        edges = edge_cases()
        edge, edge_ca = _records([over for _, over in edges])
        cont, cont_ca = _records([dict(r=7.5, alpha=-1.5, beta=-2.5, t=-3.25, phi=-0.75, redshift=0.8, cosalpha=-0.3)] * N_CONTENTION)
        rec = Records(np.concatenate([bulk, edge, cont]), np.concatenate([bulk_ca, edge_ca, cont_ca]), [label for label, _ in edges], len(bulk))
        for a in (rec.rays, rec.return_rays, rec.poison, rec.nan_weight):
            a.setflags(write=False)
        _cache["small"] = rec
    return _cache["small"]


def large():
    """The small set tiled to 262 144 + 321 records: the grid-stride loops of the histogram kernels (1024 workgroups of 256) and of the return
    kernel (512) wrap, with a ragged tail."""
    if "large" not in _cache:
        _cache["large"] = small().tiled(N_LARGE)
    return _cache["large"]


def guard_bands(rays):
    """Asserts the exactness conditions of the module docstring on `rays`; returns the two smallest distances found."""
    r, theta = rays["r"], rays["theta"]
    with np.errstate(invalid="ignore"):
        z_gap = np.abs(r * np.cos(theta) - 1e-2)
    z_gap = z_gap[np.isfinite(z_gap)]
    assert z_gap.min() > 1e-9, ("z = r cos(theta) within 1e-9 of 1e-2", float(z_gap.min()))
    q_gap = np.inf
    for name, b in emis_cases().items():
        if not b.logbin:
            continue
        q = rr.emissivity_quotient(b, r)
        keep = np.isfinite(q) & (r != b.r_min)
        gap = np.abs(q[keep] - np.rint(q[keep]))
        if gap.size:
            assert gap.min() > 1e-9, (name, "log-bin quotient within 1e-9 of an integer at r =", float(r[keep][np.argmin(gap)]))
            q_gap = min(q_gap, float(gap.min()))
    return float(z_gap.min()), q_gap
