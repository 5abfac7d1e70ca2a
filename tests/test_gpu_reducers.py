"""GPU: the three reducers of raytrace_cpu_amd/csrc/kr_post.hip -- reduce_emissivity_kernel / post_emissivity_kernel (LDS and global-atomic
instances), reduce_image_kernel / post_image_kernel, reduce_return_kernel / reduce_return_multi_kernel -- on the chosen records of
tests/reducer_cases.py against the numpy rules of tests/reducer_rules.py (which tests/test_reducer_rules.py ties to the oracle): linear and log
bins, flipped and un-flipped, square and non-square images, nr = 1 .. 3000 across the LDS capacity, records on every bin, pixel and filter edge,
non-finite fields, 20 000 records in one bin, and sizes at which the grid-stride loops wrap.

Counts and disc_count are compared exactly, with no slack and no bin left out (the generator's guard bands make that fair); every sum within
parity.BIN_RTOL of the per-bin sum of absolute terms; a bin whose reference sum is NaN or infinite must be so on the device.  The worst relative
sum error of every case goes to the margins file (parity.record_margin; profiles/reducer_edge_margins.json holds the measured figures)."""
import ctypes as C
import math

import numpy as np
import pytest

import golden_cases as gc
import parity
import reducer_cases as rc
import reducer_rules as rr
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu
vp = C.c_void_p
RTOL = parity.BIN_RTOL


@pytest.fixture
def dev(krlib):
    """Device buffers of one test, freed at its end."""
    with DeviceScope(krlib) as scope:
        yield scope


def upload(dev, a):
    """A device copy of `a`, in a buffer of at least 8 bytes."""
    a = np.ascontiguousarray(a)
    return dev.upload(a) if a.nbytes >= 8 else dev.alloc(8)


def device_words(dev, n, fill=0.0):
    return upload(dev, np.full(n, fill))


def fetch(dev, d, n, dtype=np.float64):
    capi.check(dev.lib, dev.lib.kr_synchronize(None), "sync")
    return dev.fetch(d, n, dtype)


def hist_dict(words, nr):
    """The 5 nr + 1 words of the device histogram as the dict api.reduce_emissivity returns."""
    raw = api._emissivity_layout(capi.EmisBins(nr=nr), words)                   # the planes and disc_count as they are, not yet cast
    assert np.isfinite(raw["count"]).all() and np.isfinite(raw["disc_count"])
    out = {"count": np.rint(raw["count"]).astype(np.int64), "disc_count": int(round(float(raw["disc_count"])))}
    assert np.array_equal(out["count"], raw["count"])                           # counts are whole numbers
    out.update({k: raw[k] for k in rr.EMIS_SUMS})
    return out


def image_dict(words, b):
    npix = b.img_nx * b.img_ny
    assert np.isfinite(words[:npix]).all() and np.array_equal(np.rint(words[:npix]), words[:npix])
    return api.image_planes_from_words(words, b.img_nx, b.img_ny)


def margin(test, case, n, worst, **extra):
    parity.record_margin(test, case, {"n_traced": int(n), "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(worst)}, allowed=RTOL,
                         bar="counts exact; worst_ok = worst |sum - rules| / per-bin sum of absolute terms", **extra)


def dev_emissivity(dev, b, d_rays, n, d_hist=None, first=0):
    d_hist = d_hist or device_words(dev, 5 * b.nr + 1)
    capi.check(dev.lib, dev.lib.kr_reduce_emissivity_dev_f64(C.byref(b), vp(d_rays.value + 144 * first), n, d_hist, None), "kr_reduce_emissivity_dev")
    return d_hist


def dev_image(dev, b, d_rays, n, d_planes=None, first=0):
    d_planes = d_planes or device_words(dev, 7 * b.img_nx * b.img_ny + 1)
    capi.check(dev.lib, dev.lib.kr_reduce_image_dev_f64(C.byref(b), vp(d_rays.value + 144 * first), n, d_planes, None), "kr_reduce_image_dev")
    return d_planes


def dev_return(dev, b, d_rays, n, d_out=None, first=0):
    d_out = d_out or device_words(dev, 4)
    capi.check(dev.lib, dev.lib.kr_reduce_return_dev_f64(C.byref(b), vp(d_rays.value + 144 * first), n, d_out, None), "kr_reduce_return_dev")
    return d_out


# ---- emissivity ---------------------------------------------------------------------------------------------------------------------------
EMIS_RUNS = [(case, "small") for case in sorted(rc.emis_cases())] + [(f"{rule}-nr{nr}", "large") for rule in ("lin", "log") for nr in (7, 1025)]


@pytest.mark.parametrize("case,size", EMIS_RUNS, ids=[f"{c}-{s}" for c, s in EMIS_RUNS])
def test_emissivity_reducer_matches_the_rules(dev, case, size):
    """reduce_emissivity_kernel<true> (nr <= 1024) and <false> (beyond), host form and device form; small set with and without the records
    that carry a non-finite term, large set (the 1024-workgroup grid wraps, ragged tail)."""
    b = rc.emis_cases()[case]
    rec = rc.small() if size == "small" else rc.large()
    sets = [("all", rec.rays)] + ([("finite", rec.rays[~rec.poison])] if size == "small" else [])
    for name, rays in sets:
        want = rr.reduce_emissivity(b, rays)
        label = f"{case}-{size}-{name}"
        worst = rr.check_reduction(hist_dict(fetch(dev, dev_emissivity(dev, b, upload(dev, rays), len(rays)), 5 * b.nr + 1), b.nr), want, "count",
                                   rr.EMIS_SUMS, RTOL, label + " (device form)")
        if size == "small":
            worst = max(worst, rr.check_reduction(api.reduce_emissivity(b, np.ascontiguousarray(rays)), want, "count", rr.EMIS_SUMS, RTOL, label + " (host form)"))
        print(f"emissivity {label}: binned {int(want['count'].sum())} of {want['disc_count']} on the disc, fullest bin {int(want['count'].max())}, worst sum error {worst:.3g}")
        margin("test_emissivity_reducer_matches_the_rules", label, len(rays), worst, binned=int(want["count"].sum()), on_disc=want["disc_count"])
        if name == "finite":
            assert all(np.isfinite(want[k]).all() for k in rr.EMIS_SUMS)


def test_emissivity_linear_table_on_the_device(dev):
    """The linear rule's table, row by row: one record, four bins of 0.25 from r_min = 1.25, r_isco = 1."""
    rec, b = rc.small(), rc.emis_bins(4, 0)
    for v, want_bin in rc.LINEAR_TABLE:
        ray = rec.rays[rec.edge(f"r={v!r}"):][:1]
        got = hist_dict(fetch(dev, dev_emissivity(dev, b, upload(dev, ray), 1), 21), 4)
        assert got["disc_count"] == 1 and np.flatnonzero(got["count"]).tolist() == ([] if want_bin is None else [want_bin]), (v, got["count"])


# ---- image --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(rc.image_cases()))
def test_image_reducer_matches_the_rules(dev, case):
    """reduce_image_kernel, host form and device form, flipped or not, square or not (px = ix img_ny + iy): small and large set."""
    b = rc.image_cases()[case]
    npix = b.img_nx * b.img_ny
    small, large = rc.small(), rc.large()
    for name, rays in (("all", small.rays), ("finite", small.rays[~small.poison]), ("large", large.rays)):
        want = rr.reduce_image(b, rays)
        label = f"{case}-{name}"
        worst = rr.check_reduction(image_dict(fetch(dev, dev_image(dev, b, upload(dev, rays), len(rays)), 7 * npix + 1), b), want, "nrays", rr.IMAGE_SUMS,
                                   RTOL, label + " (device form)")
        if name != "large":
            worst = max(worst, rr.check_reduction(api.reduce_image(b, np.ascontiguousarray(rays)), want, "nrays", rr.IMAGE_SUMS, RTOL, label + " (host form)"))
        print(f"image {label}: {want['disc_count']} records in {int((want['nrays'] > 0).sum())} of {npix} pixels, fullest {int(want['nrays'].max())}, worst sum error {worst:.3g}")
        margin("test_image_reducer_matches_the_rules", label, len(rays), worst, counted=want["disc_count"])
        if name == "finite":
            assert all(np.isfinite(want[k]).all() for k in rr.IMAGE_SUMS)


@pytest.mark.parametrize("shape", [(8, 8), (5, 13), (13, 5)])
@pytest.mark.parametrize("flip", [0, 1])
def test_image_edge_records_land_in_the_pixel_the_rules_name(dev, shape, flip):
    """Every record of the edge block alone: counted or not, and in which pixel -- the table of the index rule on both axes among them."""
    rec, b = rc.small(), rc.image_bins(*shape, flip)
    npix = shape[0] * shape[1]
    edges = rec.rays[rec.first_edge:rec.first_edge + len(rec.labels)]
    keep = rr.image_filter(b, edges)
    ok, _, _, px = rr.image_pixel(b, edges["alpha"], edges["beta"])
    d_rays = upload(dev, edges)
    d_planes = device_words(dev, len(edges) * (7 * npix + 1))
    for i in range(len(edges)):
        dev_image(dev, b, d_rays, 1, vp(d_planes.value + 8 * i * (7 * npix + 1)), first=i)
    words = fetch(dev, d_planes, len(edges) * (7 * npix + 1)).reshape(len(edges), 7 * npix + 1)
    for i, label in enumerate(rec.labels):
        hit = np.flatnonzero(words[i, :npix])
        want = [int(px[i])] if keep[i] and ok[i] else []
        assert hit.tolist() == want and words[i, 7 * npix] == len(want) and (not want or words[i, want[0]] == 1), (label, hit, want)
    if shape == (8, 8):                                                     # the table, literally
        for axis in ("alpha", "beta"):
            for v, pixel in rc.PIXEL_TABLE:
                i = rec.labels.index(f"{axis}={v!r}")
                hit = np.flatnonzero(words[i, :npix]).tolist()
                if pixel is None:
                    assert hit == [], (axis, v, hit)
                else:
                    assert hit == [pixel * 8 + (3 if flip else 4) if axis == "alpha" else 4 * 8 + (7 - pixel if flip else pixel)], (axis, v, hit)


# ---- returning radiation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(rc.return_cases()))
def test_return_reducer_matches_the_rules(krlib, dev, case):
    """reduce_return_kernel<false>, host and device form: with the NaN-weight records every sum they touch is NaN on both sides, without them
    every sum is finite; the large set wraps the 512-workgroup grid."""
    b = rc.return_cases()[case]
    small, large = rc.small(), rc.large()
    weighted = bool(b.plane_iso or b.limb)
    for name, rays in (("all", small.return_rays), ("without-nan-weights", small.return_rays[~small.nan_weight]),
                       ("large-without-nan-weights", large.return_rays[~large.nan_weight])):
        want = rr.reduce_return(b, rays)
        if name == "all" and weighted:
            assert np.isnan(want[1:]).all() and np.isnan(want[0]) == bool(b.weight_norm)
        else:
            assert np.isfinite(want).all() and (want > 0).all()
        label = f"{case}-{name}"
        worst = rr.check_return(fetch(dev, dev_return(dev, b, upload(dev, rays), len(rays)), 4), want, RTOL, not b.weight_norm, label + " (device form)")
        if not name.startswith("large"):
            out = (C.c_double * 4)()
            rays = np.ascontiguousarray(rays)
            capi.check(krlib, krlib.kr_reduce_return_f64(C.byref(b), rays.ctypes.data_as(vp), len(rays), C.byref(out)), "kr_reduce_return")
            worst = max(worst, rr.check_return(np.array(out[:]), want, RTOL, not b.weight_norm, label + " (host form)"))
        print(f"return {label}: {want}, worst sum error {worst:.3g}")
        margin("test_return_reducer_matches_the_rules", label, len(rays), worst)


def test_return_batch_of_33_equals_the_single_calls_and_the_rules(krlib, dev):
    """kr_post_return_batch_dev_f64 with one item more than a chunk holds (the second launch has a single item), unequal sizes, one of them 0:
    every item's sums against the rules (range_phi first) and against kr_post_return_dev_f64 on the same records; records bit for bit."""
    lib = krlib
    rec = rc.small()
    rays = rec.return_rays[~rec.nan_weight]
    k = 33
    sizes = [0 if j == 5 else 20 + 7 * j for j in range(k - 1)]
    sizes.append(len(rays) - sum(sizes))                                    # the last one takes the rest, the contention block with it
    assert len(set(sizes)) == k and sizes[-1] > rc.N_CONTENTION
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    cases = sorted(rc.return_cases())
    bins = (capi.ReturnBins * k)(*[rc.return_cases()[cases[j % 8]] for j in range(k)])
    d_single, d_batch = upload(dev, rays), upload(dev, rays)
    out_single, out_batch = device_words(dev, 4 * k), device_words(dev, 4 * k)
    for j in range(k):
        capi.check(lib, lib.kr_post_return_dev_f64(-math.pi, math.pi, C.byref(bins[j]), vp(d_single.value + 144 * int(starts[j])), sizes[j],
                                                   vp(out_single.value + 32 * j), None), "kr_post_return_dev")
    ptrs = (vp * k)(*[d_batch.value + 144 * int(starts[j]) for j in range(k)])
    outs = (vp * k)(*[out_batch.value + 32 * j for j in range(k)])
    capi.check(lib, lib.kr_post_return_batch_dev_f64(k, -math.pi, math.pi, bins, ptrs, (C.c_int64 * k)(*sizes), outs, None), "kr_post_return_batch_dev")
    single, batch = fetch(dev, out_single, 4 * k).reshape(k, 4), fetch(dev, out_batch, 4 * k).reshape(k, 4)
    worst = 0.0
    for j in range(k):
        b = bins[j]
        want = rr.reduce_return(b, rays[starts[j]:starts[j + 1]], wrap=(-math.pi, math.pi))
        for name, got in (("single", single[j]), ("batch", batch[j])):
            worst = max(worst, rr.check_return(got, want, RTOL, not b.weight_norm, (j, name)))
        worst = max(worst, rr.check_return(batch[j], single[j], RTOL, not b.weight_norm, (j, "batch against single")))
    assert (batch[5] == 0).all() and (batch[np.arange(k) != 5, 0] > 0).all()
    wrapped = rays.copy()
    wrapped["phi"] = rr.range_phi(rays["phi"], rays["steps"])
    assert (wrapped["phi"] != rays["phi"]).sum() > 1000
    for d in (d_single, d_batch):
        assert parity.same_records(fetch(dev, d, len(rays), capi.RAY_F64), wrapped)
    print(f"return batch: worst sum error {worst:.3g}")
    margin("test_return_batch_of_33_equals_the_single_calls_and_the_rules", "33 items", len(rays), worst)


# ---- accumulation -------------------------------------------------------------------------------------------------------------------------
PREFILL = 1000.0


@pytest.mark.parametrize("case", ["log-nr7", "lin-nr1024", "lin-nr1025"])
def test_emissivity_reducer_adds_into_the_callers_buffer(dev, case):
    """One call over the set == two calls over its halves into one buffer == a call into a pre-filled buffer minus the pre-fill."""
    b = rc.emis_cases()[case]
    rec = rc.small()
    rays = rec.rays[~rec.poison]
    n, half, words = len(rays), len(rays) // 2 + 1, 5 * b.nr + 1
    want = rr.reduce_emissivity(b, rays)
    d_rays = upload(dev, rays)
    halves = dev_emissivity(dev, b, d_rays, half)
    dev_emissivity(dev, b, d_rays, n - half, halves, first=half)
    filled = dev_emissivity(dev, b, d_rays, n, device_words(dev, words, PREFILL))
    for name, h in (("halves", fetch(dev, halves, words)), ("prefilled", fetch(dev, filled, words) - PREFILL)):
        got = hist_dict(h, b.nr)
        if name == "prefilled":                                             # the subtraction costs the sums up to an ulp of the pre-fill: counts only
            assert np.array_equal(got["count"], want["count"]) and got["disc_count"] == want["disc_count"]
        else:
            margin("test_emissivity_reducer_adds_into_the_callers_buffer", case, n, rr.check_reduction(got, want, "count", rr.EMIS_SUMS, RTOL, (case, name)))


@pytest.mark.parametrize("case", ["5x13-flip0", "1x1-flip1"])
def test_image_reducer_adds_into_the_callers_buffer(dev, case):
    b = rc.image_cases()[case]
    rec = rc.small()
    rays = rec.rays[~rec.poison]
    n, half, words = len(rays), len(rays) // 2 + 1, 7 * b.img_nx * b.img_ny + 1
    want = rr.reduce_image(b, rays)
    d_rays = upload(dev, rays)
    halves = dev_image(dev, b, d_rays, half)
    dev_image(dev, b, d_rays, n - half, halves, first=half)
    filled = dev_image(dev, b, d_rays, n, device_words(dev, words, PREFILL))
    for name, h in (("halves", fetch(dev, halves, words)), ("prefilled", fetch(dev, filled, words) - PREFILL)):
        got = image_dict(h, b)
        if name == "prefilled":
            assert np.array_equal(got["nrays"], want["nrays"]) and got["disc_count"] == want["disc_count"]
        else:
            margin("test_image_reducer_adds_into_the_callers_buffer", case, n, rr.check_reduction(got, want, "nrays", rr.IMAGE_SUMS, RTOL, (case, name)))


def test_return_reducer_adds_into_the_callers_buffer(dev):
    rec = rc.small()
    rays = rec.return_rays[~rec.nan_weight]
    n, half = len(rays), len(rays) // 2 + 1
    d_rays = upload(dev, rays)
    for case in ("iso0-limb0-norm0", "iso1-limb1-norm1"):
        b = rc.return_cases()[case]
        want = rr.reduce_return(b, rays)
        halves = dev_return(dev, b, d_rays, half)
        dev_return(dev, b, d_rays, n - half, halves, first=half)
        margin("test_return_reducer_adds_into_the_callers_buffer", case, n, rr.check_return(fetch(dev, halves, 4), want, RTOL, not b.weight_norm, case))
        filled = fetch(dev, dev_return(dev, b, d_rays, n, device_words(dev, 4, PREFILL)), 4) - PREFILL
        if not b.weight_norm and not b.plane_iso and not b.limb:            # whole numbers: exact
            assert np.array_equal(filled, want)


# ---- the fused post passes against the separate ones, on the code paths the golden and full-size runs do not reach ---------------------------
def fused_records(golden, run):
    """Traced records of a golden case (phi pushed out of [-pi, pi) so that range_phi has work to do) followed by the small set."""
    fin = np.load(gc.golden_path(golden))[f"final__{run}"].copy()
    fin["phi"] += 40.0
    return np.concatenate([fin, rc.small().rays])


@pytest.mark.parametrize("case", ["lin-nr7", "lin-nr1025", "log-nr1025", "log-rmin-negative"])
def test_fused_emissivity_pass_equals_the_separate_passes(krlib, dev, case):
    """kr_post_emissivity_dev_f64 == kr_range_phi_dev_f64 + kr_redshift_dev_f64 + kr_reduce_emissivity_dev_f64 with linear bins and beyond the LDS
    capacity (post_emissivity_kernel<false>): records bit for bit, counts exact, and both histograms against the rules on those records."""
    lib = krlib
    b = rc.emis_cases()[case]
    rays = fused_records("ps_h5", "rk4")
    n, words = len(rays), 5 * b.nr + 1
    d_sep, d_fused = upload(dev, rays), upload(dev, rays)
    h_sep, h_fused = device_words(dev, words), device_words(dev, words)
    capi.check(lib, lib.kr_range_phi_dev_f64(-np.pi, np.pi, d_sep, n, None), "range_phi")
    capi.check(lib, lib.kr_redshift_dev_f64(gc.SPIN, -1.0, 0, 0, 0, d_sep, n, None), "redshift")
    capi.check(lib, lib.kr_reduce_emissivity_dev_f64(C.byref(b), d_sep, n, h_sep, None), "reduce")
    capi.check(lib, lib.kr_post_emissivity_dev_f64(gc.SPIN, -1.0, 0, 0, 0, -np.pi, np.pi, C.byref(b), d_fused, n, h_fused, None), "post")
    sep, fused = fetch(dev, d_sep, n, capi.RAY_F64), fetch(dev, d_fused, n, capi.RAY_F64)
    assert parity.same_records(sep, fused)
    assert (sep["phi"] != rays["phi"]).sum() > 1000 and (sep["redshift"] > 0).sum() > rc.N_CONTENTION
    want = rr.reduce_emissivity(b, sep)
    worst = max(rr.check_reduction(hist_dict(fetch(dev, h, words), b.nr), want, "count", rr.EMIS_SUMS, RTOL, (case, name)) for name, h in (("separate", h_sep), ("fused", h_fused)))
    assert want["disc_count"] > rc.N_CONTENTION and (case == "log-rmin-negative" or want["count"].max() >= rc.N_CONTENTION)
    margin("test_fused_emissivity_pass_equals_the_separate_passes", case, n, worst, on_disc=want["disc_count"])


@pytest.mark.parametrize("case", ["5x13-flip0", "13x5-flip1"])
def test_fused_image_pass_equals_the_separate_passes(krlib, dev, case):
    """kr_post_image_dev_f64 == kr_redshift_dev_f64 + kr_range_phi_dev_f64 + kr_reduce_image_dev_f64 on non-square images, un-flipped among them."""
    lib = krlib
    b = rc.image_cases()[case]
    rays = fused_records("ip16", "rk4")
    n, words = len(rays), 7 * b.img_nx * b.img_ny + 1
    d_sep, d_fused = upload(dev, rays), upload(dev, rays)
    p_sep, p_fused = device_words(dev, words), device_words(dev, words)
    capi.check(lib, lib.kr_redshift_dev_f64(-gc.SPIN, -1.0, 1, 0, 0, d_sep, n, None), "redshift")
    capi.check(lib, lib.kr_range_phi_dev_f64(-np.pi, np.pi, d_sep, n, None), "range_phi")
    capi.check(lib, lib.kr_reduce_image_dev_f64(C.byref(b), d_sep, n, p_sep, None), "reduce")
    capi.check(lib, lib.kr_post_image_dev_f64(-gc.SPIN, -1.0, 1, 0, 0, -np.pi, np.pi, C.byref(b), d_fused, n, p_fused, None), "post")
    sep, fused = fetch(dev, d_sep, n, capi.RAY_F64), fetch(dev, d_fused, n, capi.RAY_F64)
    assert parity.same_records(sep, fused)
    assert (sep["phi"] != rays["phi"]).sum() > 1000
    want = rr.reduce_image(b, sep)
    worst = max(rr.check_reduction(image_dict(fetch(dev, p, words), b), want, "nrays", rr.IMAGE_SUMS, RTOL, (case, name)) for name, p in (("separate", p_sep), ("fused", p_fused)))
    assert want["nrays"].max() >= rc.N_CONTENTION
    margin("test_fused_image_pass_equals_the_separate_passes", case, n, worst, counted=want["disc_count"])
