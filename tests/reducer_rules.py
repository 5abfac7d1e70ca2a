"""TEST INFRASTRUCTURE: the three reducers that turn traced records into what the programs write out -- the emissivity histogram
(emissivity.cpp:96-126), the disc image (imageplane_disc_image.cpp:122-161) and the returning-radiation classification
(disc_source_photonfrac_r.cpp:97-126) -- restated in numpy over ray records, in the manner of tests/line_rules.py and tests/caustic_rules.py.
tests/test_reducer_rules.py pins this restatement to the oracle before tests/test_gpu_reducers.py lets it judge the device kernels.  Nothing here
runs in the product path.

The index rule (include/kr_trace.h, kr_emis_bins / kr_image_bins) is stated on the floating quotient q, never on a converted integer: a record is
binned iff q is not NaN and -1 < q < n, at index trunc(q) -- so the band (-1, 0] below the first edge truncates to index 0, as the reference's
`(int) q` followed by `0 <= i < n` does, and NaN, +-inf and quotients beyond the int range are not binned (the reference converts those to INT_MIN
on x86 and rejects them).  A flipped image row is img_ny - 1 - trunc(q) of a q that passed that test.

Sums are exact per bin (math.fsum), which makes this the more precise side of every comparison; a bin that holds a non-finite term gets the plain
IEEE sum (inf, or NaN from inf - inf or a NaN term: the same whatever the order of the additions).  Beside every sum plane the per-bin sum of the
ABSOLUTE terms is returned under out["abs"][plane]: the tolerance of a signed sum (phi, time, sum_time) is taken against it."""
import math

import numpy as np

EMIS_SUMS = ("flux", "emis", "sum_redshift", "sum_time")
IMAGE_SUMS = ("flux", "r", "phi", "enshift", "time", "emis")
TWO_PI = 2 * math.pi


def bin_index(q, n):
    """(binned, index) of the floating quotients q over n bins: binned iff -1 < q < n (NaN fails), index trunc(q) (0 where not binned)."""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (q > -1) & (q < n)
    return ok, np.trunc(np.where(ok, q, 0.0)).astype(np.int64)


def powerlaw3(r, q1, rb1, q2, rb2, q3):
    """imageplane_disc_image.cpp:20-28, elementwise."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(r < rb1, r ** (-1 * q1), np.where(r < rb2, rb1 ** (q2 - q1) * r ** (-1 * q2), rb1 ** (q2 - q1) * rb2 ** (q3 - q2) * r ** (-1 * q3)))


def bin_sums(index, terms, n):
    """Per bin: (sum of terms, sum of |terms|), exact where every term of the bin is finite."""
    total, total_abs = np.zeros(n), np.zeros(n)
    order = np.argsort(index, kind="stable")
    idx, val = index[order], np.asarray(terms, dtype=np.float64)[order]
    cuts = np.flatnonzero(np.diff(idx)) + 1
    for chunk_i, chunk_v in zip(np.split(idx, cuts), np.split(val, cuts)):
        if not len(chunk_i):
            continue
        k = int(chunk_i[0])
        if np.isfinite(chunk_v).all():
            total[k], total_abs[k] = math.fsum(chunk_v), math.fsum(np.abs(chunk_v))
        else:
            with np.errstate(invalid="ignore"):
                total[k], total_abs[k] = float(np.sum(chunk_v)), float(np.sum(np.abs(chunk_v)))
    return total, total_abs


def emissivity_quotient(b, r):
    """The radial bin quotient of emissivity.cpp:106: log(r / r_min) / log(dr) with logbin, (r - r_min) / dr without."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.log(r / b.r_min) / np.log(np.float64(b.dr)) if b.logbin else (r - b.r_min) / np.float64(b.dr)


def emissivity_filter(b, rays):
    """steps > 0, z = r cos(theta) < 1e-2, g > 0, r >= r_isco (emissivity.cpp:98-104): what disc_count counts, binned or not."""
    with np.errstate(invalid="ignore"):
        return (rays["steps"] > 0) & (rays["r"] * np.cos(rays["theta"]) < 1e-2) & (rays["redshift"] > 0) & (rays["r"] >= b.r_isco)


def reduce_emissivity(b, rays):
    """api.reduce_emissivity in numpy: count (int64), flux, emis, sum_redshift, sum_time (raw sums), disc_count; plus "abs"."""
    m = emissivity_filter(b, rays)
    r, g, t = rays["r"][m], rays["redshift"][m], rays["t"][m]
    ok, ir = bin_index(emissivity_quotient(b, r), b.nr)
    ir, g, t = ir[ok], g[ok], t[ok]
    with np.errstate(all="ignore"):
        terms = {"flux": 1 / (b.num_primary_rays * g ** 1.0), "emis": 1 / g ** b.gamma, "sum_redshift": g, "sum_time": t}
    out = {"count": np.bincount(ir, minlength=b.nr).astype(np.int64), "disc_count": int(m.sum()), "abs": {}}
    for k in EMIS_SUMS:
        out[k], out["abs"][k] = bin_sums(ir, terms[k], b.nr)
    return out


def image_filter(b, rays):
    """steps > 0, z < 1e-2, r_isco <= r < r_disc, g > 0 (imageplane_disc_image.cpp:127-128), before the pixel range."""
    r = rays["r"]
    with np.errstate(invalid="ignore"):
        return (rays["steps"] > 0) & (r * np.cos(rays["theta"]) < 1e-2) & (r >= b.r_isco) & (r < b.r_disc) & (rays["redshift"] > 0)


def image_pixel(b, alpha, beta):
    """(binned, ix, iy, px) of image coordinates: px = ix img_ny + iy like the program's Array2D, iy counted from the top with flip_image."""
    with np.errstate(all="ignore"):
        okx, ix = bin_index((np.asarray(alpha, dtype=np.float64) - b.x0) / np.float64(b.img_dx), b.img_nx)
        oky, iy = bin_index((np.asarray(beta, dtype=np.float64) - b.y0) / np.float64(b.img_dy), b.img_ny)
    if b.flip_image:
        iy = b.img_ny - 1 - iy
    ok = okx & oky
    return ok, ix, iy, np.where(ok, ix * b.img_ny + iy, 0)


def reduce_image(b, rays):
    """api.reduce_image in numpy: nrays (int32), the six raw-sum planes, disc_count (rays that reached a pixel); plus "abs"."""
    npix = b.img_nx * b.img_ny
    m = image_filter(b, rays)
    ok, _, _, px = image_pixel(b, rays["alpha"][m], rays["beta"][m])
    rec = rays[m][ok]
    px = px[ok]
    r, g = rec["r"], rec["redshift"]
    e = powerlaw3(r, b.q1, b.rb1, b.q2, b.rb2, b.q3)
    with np.errstate(all="ignore"):
        terms = {"flux": e / g ** 3.0, "r": r, "phi": rec["phi"], "enshift": 1.0 / g, "time": rec["t"], "emis": e}
    out = {"nrays": np.bincount(px, minlength=npix).astype(np.int32), "disc_count": int(len(px)), "abs": {}}
    for k in IMAGE_SUMS:
        out[k], out["abs"][k] = bin_sums(px, terms[k], npix)
    return out


def range_phi(phi, steps, lo=-math.pi, hi=math.pi):
    """raytracer.cpp:603-622: repeated -+2 pi into [lo, hi); rays beyond |phi| = 1000, NaN and steps <= 0 stay as they are."""
    phi = np.array(phi, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        live = ~((np.abs(phi) > 1000) | np.isnan(phi) | ~(np.asarray(steps) > 0))
        while True:
            m = live & (phi >= hi)
            if not m.any():
                break
            phi[m] -= TWO_PI
        while True:
            m = live & (phi < lo)
            if not m.any():
                break
            phi[m] += TWO_PI
    return phi


def return_weight(b, rays):
    """|sin(alpha) sin(beta)| (plane_iso) x (1 + 2.06 |sin(alpha) sin(beta)|) (limb); rays[].alpha holds cos(alpha)."""
    with np.errstate(invalid="ignore"):
        sasb = np.abs(np.sin(np.arccos(rays["alpha"])) * np.sin(rays["beta"]))
        w = sasb if b.plane_iso else np.ones(len(rays))
        return w * (1 + 2.06 * sasb) if b.limb else w


def reduce_return(b, rays, wrap=None):
    """kr_reduce_return_f64 in numpy: [ray_count, return, escape, lost]; wrap = (lo, hi): range_phi first, as kr_post_return_dev_f64 does."""
    live = rays["steps"] > 0
    rec = rays[live]
    phi = range_phi(rec["phi"], rec["steps"], *wrap) if wrap else rec["phi"]
    w = return_weight(b, rec)
    r = rec["r"]
    with np.errstate(invalid="ignore"):
        disc = (rec["theta"] >= math.pi / 2) & (r >= b.r_isco) & (r < b.r_disc)
        away = (np.abs(r - b.source_r) > 0.1 * b.source_r) | (np.abs(phi - b.source_phi) > 0.1)
        escape = ~disc & (r > b.r_esc)
        lost = ~disc & ~escape & (r < b.r_isco)

    def total(x):
        return bin_sums(np.zeros(len(x), dtype=np.int64), x, 1)[0][0] if len(x) else 0.0
    return np.array([total(w if b.weight_norm else np.ones(len(rec))), total(w[disc & away]), total(w[escape]), total(w[lost])])


def sum_errors(got, want, keys):
    """Worst |got - want| / (per-bin sum of absolute terms) over the finite bins of `keys`, and the problems of the non-finite ones: a bin whose
    reference sum is NaN (inf) must be NaN (the same inf) in `got`, and no other bin may be non-finite.  Returns (worst, problems)."""
    worst, problems = 0.0, []
    for k in keys:
        g, w, a = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64), np.asarray(want["abs"][k], dtype=np.float64)
        fin = np.isfinite(w)
        bad = (np.isnan(w) != np.isnan(g)) | (~fin & ~np.isnan(w) & (g != w)) | (fin & ~np.isfinite(g))
        if bad.any():
            problems.append((k, "non-finite bins differ", int(np.flatnonzero(bad)[0])))
        sel = fin & np.isfinite(g)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(g[sel] == w[sel], 0.0, np.abs(g[sel] - w[sel]) / a[sel])
        if rel.size:
            worst = max(worst, float(np.nan_to_num(rel, nan=np.inf).max()))
    return worst, problems


def check_reduction(got, want, count_key, sums, rtol, label=""):
    """The bar of the reducer tests, `want` from this module: counts and disc_count exact (no slack, no bin left out), every sum within rtol of
    the per-bin sum of absolute terms, non-finite bins alike.  Returns the worst relative sum error."""
    np.testing.assert_array_equal(np.asarray(got[count_key]), want[count_key], err_msg=str(label))
    assert got["disc_count"] == want["disc_count"], (label, got["disc_count"], want["disc_count"])
    worst, problems = sum_errors(got, want, sums)
    assert problems == [] and worst <= rtol, (label, worst, problems)
    return worst


def check_return(got, want, rtol, exact_count, label=""):
    """The same for the four returning-radiation sums (every term >= 0): NaN where the rules are NaN and nowhere else, ray_count exact when it
    is unweighted.  Returns the worst relative error."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, got, want)
    fin = ~np.isnan(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(got[fin] == want[fin], 0.0, np.abs(got[fin] - want[fin]) / want[fin])
    assert (rel <= rtol).all(), (label, got, want)
    if exact_count:
        assert got[0] == want[0], (label, got, want)
    return float(rel.max()) if rel.size else 0.0
