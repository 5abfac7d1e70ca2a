"""TEST INFRASTRUCTURE: the landing map of the returning radiation (include/kr_trace.h, kr_return_map) restated in numpy over ray records, built
only from tests/reducer_rules.py: the weight, range_phi and the four sums of its returning-radiation classification (return_weight, range_phi,
reduce_return) and the quotient, index rule and per-bin sums of its emissivity histogram (emissivity_quotient, bin_index, bin_sums).
tests/test_return_map_rules.py ties this restatement to those two rule sets -- both pinned to the oracle by tests/test_reducer_rules.py -- before
tests/test_gpu_return_map.py lets it judge the device kernels.  Nothing here runs in the product path.

Per-bin sums are exact (math.fsum); a bin that holds a non-finite term gets the plain IEEE sum; beside every sum plane the per-bin sum of the
absolute terms is returned under out["abs"][plane] (reducer_rules.bin_sums)."""
import math

import numpy as np

import reducer_rules as rr
from raytrace_cpu_amd import capi

MAP_SUMS = ("weight", "flux", "emis", "time")
SCALARS = ("ray_count", "return", "escape", "lost")


def map_struct(cls, r_min, dr, nr, logbin, gamma):
    """kr_return_map from a kr_return_bins and the landing bins."""
    m = capi.ReturnMap()
    m.cls = cls
    m.r_min, m.dr, m.gamma, m.nr, m.logbin = r_min, dr, gamma, int(nr), int(logbin)
    return m


def return_class(b, rec, phi):
    """The `return` class of live records (steps > 0): theta >= pi / 2, r_isco <= r < r_disc, away from the source."""
    r = rec["r"]
    with np.errstate(invalid="ignore"):
        disc = (rec["theta"] >= math.pi / 2) & (r >= b.r_isco) & (r < b.r_disc)
        away = (np.abs(r - b.source_r) > 0.1 * b.source_r) | (np.abs(phi - b.source_phi) > 0.1)
    return disc & away


def reduce_return_map(m, rays, wrap=None):
    """kr_reduce_return_map_f64 in numpy; wrap = (lo, hi): range_phi first, as kr_post_return_map_dev_f64 does.  Returns count (int64), weight, flux,
    emis, time (raw sums), scalars = [ray_count, return, escape, lost] (reducer_rules.reduce_return), on_disc, binned; plus "abs"."""
    b, nr = m.cls, m.nr
    rec = rays[rays["steps"] > 0]
    phi = rr.range_phi(rec["phi"], rec["steps"], *wrap) if wrap else rec["phi"]
    w = rr.return_weight(b, rec)
    ret = return_class(b, rec, phi)
    rec, w = rec[ret], w[ret]
    g = rec["redshift"]
    ok, ir = rr.bin_index(rr.emissivity_quotient(m, rec["r"]), nr)
    with np.errstate(invalid="ignore"):
        ok &= g > 0
    ir, g, w, t = ir[ok], g[ok], w[ok], rec["t"][ok]
    with np.errstate(all="ignore"):
        terms = {"weight": w, "flux": w / g, "emis": w / g ** m.gamma, "time": w * t}
    out = {"count": np.bincount(ir, minlength=nr).astype(np.int64), "scalars": rr.reduce_return(b, rays, wrap), "on_disc": int(ret.sum()),
           "binned": int(ok.sum()), "abs": {}}
    for k in MAP_SUMS:
        out[k], out["abs"][k] = rr.bin_sums(ir, terms[k], nr)
    return out


def check_map(got, want, rtol, label=""):
    """The bar of the reducer tests for a landing map, `got` as api.return_map_from_words gives it and `want` from this module: count plane, on_disc and
    binned exact, every sum plane within rtol of its per-bin sum of absolute terms, non-finite bins alike, the four scalars as
    reducer_rules.check_return holds them (ray_count exact when unweighted is the caller's to add).  Returns the worst relative error."""
    count = np.asarray(got["count"], dtype=np.float64)
    assert np.isfinite(count).all() and np.array_equal(count, want["count"]), (label, "count plane")
    assert got["on_disc"] == want["on_disc"] and got["binned"] == want["binned"], (label, got["on_disc"], want["on_disc"], got["binned"], want["binned"])
    worst, problems = rr.sum_errors(got, want, MAP_SUMS)
    assert problems == [] and worst <= rtol, (label, worst, problems)
    return worst


def scalars_of(got):
    return np.array([got[k] for k in SCALARS], dtype=np.float64)
