"""CPU: the numpy restatement of the three reducers (tests/reducer_rules.py) against the oracle's (kro_reduce_emissivity_f64, kro_reduce_image_f64,
kro_reduce_return_f64) on the chosen records of tests/reducer_cases.py, for every bin set the device tests use; the two tables of the index rule as
literal pixels and bins; and the guard bands that allow the device tests to compare counts without slack."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import parity
import reducer_cases as rc
import reducer_rules as rr


def oracle_emissivity(b, rays):
    count = np.zeros(b.nr, dtype=np.int64)
    flux, emis, sg, stt = (np.zeros(b.nr) for _ in range(4))
    dc = C.c_int64()
    rays = np.ascontiguousarray(rays)
    ol.oracle().kro_reduce_emissivity_f64(C.byref(b), ol.ptr(rays), len(rays), ol.ptr(count), ol.ptr(flux), ol.ptr(emis), ol.ptr(sg), ol.ptr(stt), C.byref(dc))
    return {"count": count, "flux": flux, "emis": emis, "sum_redshift": sg, "sum_time": stt, "disc_count": dc.value}


def oracle_image(b, rays):
    npix = b.img_nx * b.img_ny
    nrays = np.zeros(npix, dtype=np.int32)
    planes = {k: np.zeros(npix) for k in rr.IMAGE_SUMS}
    dc = C.c_int64()
    rays = np.ascontiguousarray(rays)
    ol.oracle().kro_reduce_image_f64(C.byref(b), ol.ptr(rays), len(rays), ol.ptr(nrays), *[ol.ptr(planes[k]) for k in rr.IMAGE_SUMS], C.byref(dc))
    return dict(planes, nrays=nrays, disc_count=dc.value)


def oracle_return(b, rays):
    out = (C.c_double * 4)()
    rays = np.ascontiguousarray(rays)
    ol.oracle().kro_reduce_return_f64(C.byref(b), ol.ptr(rays), len(rays), C.byref(out))
    return np.array(out[:])


@pytest.mark.parametrize("case", sorted(rc.emis_cases()))
def test_emissivity_rules_equal_the_oracle(case):
    b = rc.emis_cases()[case]
    rec = rc.small()
    for name, rays in (("all", rec.rays), ("finite", rec.rays[~rec.poison])):
        want = rr.reduce_emissivity(b, rays)
        worst = rr.check_reduction(oracle_emissivity(b, rays), want, "count", rr.EMIS_SUMS, parity.BIN_RTOL, (case, name))
        print(f"emissivity {case} {name}: binned {int(want['count'].sum())} of {want['disc_count']} on the disc, worst sum error {worst:.3g}")
        if name == "finite":
            assert all(np.isfinite(want[k]).all() for k in rr.EMIS_SUMS)
        if case.startswith(("log-rmin", "lin-dr-zero")):
            assert want["count"].sum() == 0 and want["disc_count"] > 20000            # a NaN or infinite quotient: on the disc, not binned
        elif b.nr != 4:                                                              # (the table's four bins end at r = 2.25)
            assert want["count"].max() >= rc.N_CONTENTION


@pytest.mark.parametrize("case", sorted(rc.image_cases()))
def test_image_rules_equal_the_oracle(case):
    b = rc.image_cases()[case]
    rec = rc.small()
    for name, rays in (("all", rec.rays), ("finite", rec.rays[~rec.poison])):
        want = rr.reduce_image(b, rays)
        worst = rr.check_reduction(oracle_image(b, rays), want, "nrays", rr.IMAGE_SUMS, parity.BIN_RTOL, (case, name))
        print(f"image {case} {name}: {want['disc_count']} records in {int((want['nrays'] > 0).sum())} pixels, worst sum error {worst:.3g}")
        assert want["nrays"].max() >= rc.N_CONTENTION
        if name == "finite":
            assert all(np.isfinite(want[k]).all() for k in rr.IMAGE_SUMS)
        else:
            assert not np.isfinite(want["phi"]).all() and not np.isfinite(want["time"]).all() and not np.isfinite(want["flux"]).all()


@pytest.mark.parametrize("case", sorted(rc.return_cases()))
def test_return_rules_equal_the_oracle(case):
    b = rc.return_cases()[case]
    rec = rc.small()
    weighted = b.plane_iso or b.limb
    for name, rays in (("all", rec.return_rays), ("without the NaN weights", rec.return_rays[~rec.nan_weight])):
        got, want = oracle_return(b, rays), rr.reduce_return(b, rays)
        if name == "all" and weighted:
            # the NaN-weight records sit on the disc away from the source, beyond r_esc and inside r_isco (the beta = NaN rows at every r edge)
            assert np.isnan(want[1:]).all() and np.isnan(want[0]) == bool(b.weight_norm)
        else:
            assert np.isfinite(want).all() and (want > 0).all()
        worst = rr.check_return(got, want, parity.BIN_RTOL, not b.weight_norm, (case, name))
        print(f"return {case} {name}: {want}, worst sum error {worst:.3g}")
        if not b.weight_norm:
            assert got[0] == want[0] == (rays["steps"] > 0).sum()


def test_wrapped_phi_equals_the_oracle():
    """range_phi of the rules (what kr_post_return_dev_f64 applies before it classifies) == the oracle's, bit for bit."""
    rays = rc.small().return_rays.copy()
    want = rays.copy()
    ol.oracle().kro_range_phi_f64(-np.pi, np.pi, ol.ptr(want), len(want))
    rays["phi"] = rr.range_phi(rays["phi"], rays["steps"])
    assert parity.same_records(rays, want)
    assert (want["phi"] != rc.small().return_rays["phi"]).sum() > 1000


def test_pixel_table():
    """The first table of the index rule, as literal pixels of an 8 x 8 image (x0 = y0 = -4, one unit per pixel), on both axes, flipped or not: from the
    rules and from the oracle."""
    rec = rc.small()
    for flip in (0, 1):
        b = rc.image_bins(8, 8, flip)
        for axis in ("alpha", "beta"):
            for v, pixel in rc.PIXEL_TABLE:
                ray = rec.rays[rec.edge(f"{axis}={v!r}"):][:1]
                assert (ray[axis] == v) or (np.isnan(v) and np.isnan(ray[axis])), (axis, v)
                if pixel is None:
                    want_px = None
                elif axis == "alpha":
                    want_px = pixel * 8 + (3 if flip else 4)                # the other coordinate is 0.5: row 4, from the top row 3
                else:
                    want_px = 4 * 8 + (7 - pixel if flip else pixel)
                for got in (rr.reduce_image(b, ray), oracle_image(b, ray)):
                    hit = np.flatnonzero(got["nrays"])
                    assert got["disc_count"] == len(hit) == (0 if want_px is None else 1), (axis, v, flip)
                    assert want_px is None or (hit[0] == want_px and got["nrays"][want_px] == 1), (axis, v, flip, hit)
    # the rows the issue spells out: flipped, beta = -4.999 is row 7 and beta = 3.999 row 0
    b = rc.image_bins(8, 8, 1)
    for v, row in ((-4.999, 7), (3.999, 0)):
        got = rr.reduce_image(b, rec.rays[rec.edge(f"beta={v!r}"):][:1])
        assert np.flatnonzero(got["nrays"]).tolist() == [4 * 8 + row]


def test_linear_bin_table():
    """The second table: four linear bins from r_min = 1.25, 0.25 wide, r_isco = 1; every row is on the disc, binned or not."""
    rec = rc.small()
    b = rc.emis_bins(4, 0)
    assert (b.r_min, b.dr, b.nr, b.r_isco, b.logbin) == (1.25, 0.25, 4, 1.0, 0)
    for v, want_bin in rc.LINEAR_TABLE:
        ray = rec.rays[rec.edge(f"r={v!r}"):][:1]
        assert ray["r"] == v
        for got in (rr.reduce_emissivity(b, ray), oracle_emissivity(b, ray)):
            assert got["disc_count"] == 1, v
            assert np.flatnonzero(got["count"]).tolist() == ([] if want_bin is None else [want_bin]), (v, got["count"])


def test_non_square_images_keep_nx_and_ny_apart():
    """A record in column 2, row 9 of a 5 x 13 image is pixel 2 * 13 + 9 (un-flipped), and outside a 13 x 5 image's five rows."""
    ray = rc._records([dict(alpha=-1.5, beta=5.5)])[0]
    assert np.flatnonzero(rr.reduce_image(rc.image_bins(5, 13, 0), ray)["nrays"]).tolist() == [2 * 13 + 9]
    assert np.flatnonzero(rr.reduce_image(rc.image_bins(5, 13, 1), ray)["nrays"]).tolist() == [2 * 13 + 3]
    assert rr.reduce_image(rc.image_bins(13, 5, 0), ray)["disc_count"] == 0
    ray = rc._records([dict(alpha=5.5, beta=-1.5)])[0]
    assert np.flatnonzero(rr.reduce_image(rc.image_bins(13, 5, 0), ray)["nrays"]).tolist() == [9 * 5 + 2]
    for b in (rc.image_bins(5, 13, 0), rc.image_bins(13, 5, 1)):
        assert oracle_image(b, ray)["nrays"].tolist() == rr.reduce_image(b, ray)["nrays"].tolist()


def test_guard_bands_and_sizes():
    rec, big = rc.small(), rc.large()
    z_gap, q_gap = rc.guard_bands(rec.rays)
    print(f"guard bands: |z - 1e-2| >= {z_gap:.3g}, log-bin quotient to the nearest integer >= {q_gap:.3g}")
    assert 24000 < len(rec.rays) < 25000 and len(big.rays) == 262144 + 321 and len(big.rays) % len(rec.rays) != 0
    assert rec.poison.sum() == 8 and rec.nan_weight.sum() == 7
    assert len(set(rec.labels)) == len(rec.labels)                         # every edge case can be found by its label
    # r == r_min sits on a log bin's first edge, exactly: log(1) = 0
    b = rc.emis_bins(7, 1)
    assert rr.emissivity_quotient(b, np.array([b.r_min]))[0] == 0.0
    # the same generator twice gives the same bytes
    rc._cache.clear()
    assert rc.small().rays.tobytes() == rec.rays.tobytes()
