"""CPU: the numpy restatement of the (r, phi) illumination map (tests/illum_rules.py) on constructed records -- the azimuthal rule at and beside
every edge, literal cells; the map summed over ip against reducer_rules' emissivity histogram on the chosen records of tests/reducer_cases.py; and
api.illumination_table on a hand-made map."""
import math

import numpy as np
import pytest

import illum_rules as il
import parity
import reducer_cases as rc
import reducer_rules as rr
from raytrace_cpu_amd import api, capi

PI = math.pi
NAN, INF = float("nan"), float("inf")


def bins(nr, nphi, logbin=0, phi_shift=0.0):
    return capi.illum_bins(rc.emis_bins(nr, logbin), nphi, phi_shift)


def records(phi, **over):
    """One otherwise good record (r = 2, on the disc, g = 1: radial bin 0 of the log bins below) per phi."""
    rays, _ = rc._records([dict(dict(r=2.0, phi=p), **over) for p in phi])
    return rays


# phi -> ip with nphi = 8 and no shift (cells of pi / 4 from -pi), None: not binned.  The wrap is floating arithmetic, and the table says what it does
# next to +-pi: pi itself wraps to -pi (cell 0); one ulp above -pi stays in cell 0; one ulp BELOW -pi wraps to pi - 1 ulp, whose quotient rounds to
# nphi itself -- the last cell, by the min of the rule; pi - 1 ulp has (p + pi) round up to 2 pi, wraps to one ulp below -pi and fails q_ph >= 0: it
# is in no cell (the device tests assert that none of their records is such a record); pi - 2 ulp is in the last cell.
PHI_TABLE = [(-PI, 0), (PI, 0), (np.nextafter(-PI, 0.0), 0), (np.nextafter(-PI, -4.0), 7), (np.nextafter(PI, 0.0), None),
             (np.nextafter(np.nextafter(PI, 0.0), 0.0), 7), (0.0, 4), (-0.0, 4), (np.nextafter(0.0, -1.0), 4), (-0.5, 3), (-PI / 4, 3), (3 * PI / 4, 7),
             (2.5, 7), (-2.5, 0), (-12389.0, 5), (12389.0, 2), (NAN, None), (INF, None), (-INF, None)]


def test_azimuth_table():
    m = bins(4, 8, logbin=1)
    for phi, ip in PHI_TABLE:
        got = il.reduce_illum(m, records([phi]))
        hit = np.argwhere(got["count"])
        assert got["disc_count"] == 1, phi
        if ip is None:
            assert got["binned"] == 0 and len(hit) == 0, phi
        else:
            assert got["binned"] == 1 and hit.tolist() == [[0, ip]], (phi, hit)
    # -12389 = -1972 * 2 pi + 1.4414...: the cell of that remainder
    assert int((((-12389.0 + PI) % (2 * PI))) / (PI / 4)) == 5 and abs((-12389.0 + 1972 * 2 * PI) - 1.44142575814476) < 1e-9
    # with a shift: the same table one cell on
    shifted = bins(4, 8, logbin=1, phi_shift=PI / 4)
    for phi, ip in ((0.0, 5), (2.5, 0), (-2.5, 1), (NAN, None)):
        got = il.reduce_illum(shifted, records([phi]))
        assert np.argwhere(got["count"]).tolist() == ([] if ip is None else [[0, ip]]), phi


def test_one_azimuthal_cell_bins_every_phi():
    """nphi == 1: no phi test -- a NaN or infinite phi IS binned, and the map is the emissivity histogram."""
    m = bins(4, 1, logbin=1, phi_shift=0.3)
    rays = records([NAN, INF, -INF, 0.5, -12389.0])
    got = il.reduce_illum(m, rays)
    assert got["binned"] == got["disc_count"] == 5 and got["count"].tolist() == [[5], [0], [0], [0]]
    want = rr.reduce_emissivity(m.rad, rays)
    np.testing.assert_array_equal(got["count"][:, 0], want["count"])
    for k in il.SUMS:
        np.testing.assert_array_equal(got[k][:, 0], want[k])


def test_phi_shift_turns_the_map():
    """phi_shift = 2 pi k / nphi moves every record k cells on (cyclically); a record on an edge stays on an edge's upper side."""
    rng = np.random.default_rng(5)
    phi = rng.uniform(-PI, PI, 500)
    rays = records(phi)
    base = il.reduce_illum(bins(4, 16, logbin=1, phi_shift=0.0137), rays)
    for k in (1, 5, 15):
        turned = il.reduce_illum(bins(4, 16, logbin=1, phi_shift=0.0137 + 2 * PI * k / 16), rays)
        np.testing.assert_array_equal(turned["count"], np.roll(base["count"], k, axis=1))
    assert base["binned"] == 500 and il.edge_margin(base, 1) > 1e-9


@pytest.mark.parametrize("nr,nphi,logbin", [(7, 1, 1), (7, 16, 1), (12, 16, 0), (64, 512, 1), (1025, 3, 0)])
def test_summed_over_phi_is_the_emissivity_histogram(nr, nphi, logbin):
    rec = rc.small()
    rays = rec.rays[np.isfinite(rec.rays["phi"])]                   # (a NaN or infinite phi is binned by the histogram and, with nphi > 1, not by the map)
    m = bins(nr, nphi, logbin, phi_shift=0.0137)
    got = il.reduce_illum(m, rays)
    want = rr.reduce_emissivity(m.rad, rays)
    assert got["binned"] == want["count"].sum() > rc.N_CONTENTION and got["disc_count"] == want["disc_count"] > got["binned"]
    worst = rr.check_reduction(il.summed_over_phi(got), want, "count", rr.EMIS_SUMS, parity.BIN_RTOL, (nr, nphi, logbin))
    assert worst < 1e-12
    if nphi > 1:
        assert (got["count"] > 0).sum(axis=1).max() > 1             # the azimuth does spread the records of a ring
    # all records: those with a non-finite phi are on the disc and, with nphi > 1, in no cell
    all_rays = rec.rays
    lost = int((rr.emissivity_filter(m.rad, all_rays) & ~np.isfinite(all_rays["phi"]) & rr.bin_index(rr.emissivity_quotient(m.rad, all_rays["r"]), nr)[0]).sum())
    assert lost == 3
    full = il.reduce_illum(m, all_rays)
    assert full["binned"] == rr.reduce_emissivity(m.rad, all_rays)["count"].sum() - (lost if nphi > 1 else 0)


def test_check_illum_notices_a_moved_record():
    rays = records(np.linspace(-3, 3, 40))
    m = bins(4, 8, logbin=1)
    want = il.reduce_illum(m, rays)
    got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items() if k not in ("abs", "rays")}
    assert il.check_illum(got, want, parity.BIN_RTOL) == 0.0
    got["count"][0, 0], got["count"][0, 1] = got["count"][0, 0] - 1, got["count"][0, 1] + 1
    with pytest.raises(AssertionError):
        il.check_illum(got, want, parity.BIN_RTOL)


def test_illumination_table_on_a_hand_made_map():
    m = bins(3, 4)
    words = np.zeros(api.illum_words(m))
    assert len(words) == 5 * 12 + 2
    count = np.array([[2, 0, 1, 4], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=np.float64)
    emis = np.array([[8.0, 0, 2.0, 1.0], [0, 0, 0, 0], [4.0, 4.0, 4.0, 4.0]])
    time = np.array([[20.0, 0, 7.0, 44.0], [0, 0, 0, 0], [-3.0, 5.0, 6.0, 7.0]])
    words[0:12], words[24:36], words[48:60], words[60], words[61] = count.ravel(), emis.ravel(), time.ravel(), 15, 11
    res = api.illum_from_words(m, words)
    assert res["count"].dtype == np.int64 and res["count"].shape == (3, 4) and (res["disc_count"], res["binned"]) == (15, 11)
    np.testing.assert_array_equal(res["phi"], [-3 * PI / 4, -PI / 4, PI / 4, 3 * PI / 4])
    areas = np.array([2.0, 8.0, 16.0])
    tab = api.illumination_table(res, areas)
    np.testing.assert_array_equal(tab["emis"], [[16.0, 0, 4.0, 2.0], [0, 0, 0, 0], [1.0, 1.0, 1.0, 1.0]])              # emis_sum / (area / 4)
    np.testing.assert_array_equal(tab["time"], [[10.0, NAN, 7.0, 11.0], [NAN] * 4, [-3.0, 5.0, 6.0, 7.0]])
    assert (tab["nr"], tab["nphi"], tab["r_min"], tab["dr"], tab["logbin"], tab["phi_shift"]) == (3, 4, m.rad.r_min, m.rad.dr, 0, 0.0)
    e, t = il.table_from_map(res, areas)
    np.testing.assert_array_equal(e, tab["emis"])
    np.testing.assert_array_equal(t, tab["time"])
    with pytest.raises(capi.KrError, match="one area per annulus"):
        api.illumination_table(res, areas[:2])


def test_precondition_of_the_device_tests_on_the_oracles_trace():
    """Before any GPU run: the sources of tests/test_gpu_illum.py traced by the CPU oracle (RK4, the same parameters), through range_phi and redshift, have
    no binned record within 1e-9 of a cell edge in any shape or shift the device tests use -- so their exact comparison of counts is sound, and the
    off-axis source does light the disc unevenly."""
    import math

    import golden_cases as gc
    import oracle_lib as ol
    import test_gpu_illum as dev

    def oracle_records(name):
        spin = dev.SOURCES[name][0]
        if name == "offaxis":
            spec = dev.offaxis_source()
            rays = ol.oracle_pointsource(spec)
            ol.oracle().kro_redshift_start_f64(spin, spec.V, 0, 0, ol.ptr(rays), len(rays))
            p = dev.offaxis_params()
        else:
            rays, p = np.ascontiguousarray(np.load(gc.golden_path(name))["init"]), gc.cases()[name]["runs"]["rk4"]
        out, _ = ol.oracle_trace(p, rays)
        ol.oracle().kro_range_phi_f64(-math.pi, math.pi, ol.ptr(out), len(out))
        ol.oracle().kro_redshift_f64(spin, -1.0, 0, 0, 0, ol.ptr(out), len(out))
        return out

    def bins_for(name, nr, nphi, phi_shift):                       # dev.bins_for with the oracle's ISCO (no device library call)
        spin = dev.SOURCES[name][0]
        b = capi.EmisBins()
        b.r_isco = gc.r_isco(spin)
        b.r_min, b.dr = b.r_isco, float(np.exp(np.log(dev.R_DISC / b.r_isco) / nr))
        b.gamma, b.spin, b.num_primary_rays, b.nr, b.logbin = 2.0, spin, 12503.0, nr, 1
        return capi.illum_bins(b, nphi, phi_shift)

    for name in sorted(dev.SOURCES):
        rays = oracle_records(name)
        shapes = [(nr, nphi, dev.PHI_SHIFT) for nr, nphi in dev.SHAPES] + [(12, 16, dev.PHI_SHIFT + 2 * math.pi * 5 / 16), (64, 512, dev.PHI_SHIFT + 2 * math.pi * 131 / 512)]
        for nr, nphi, shift in shapes:
            want = il.reduce_illum(bins_for(name, nr, nphi, shift), rays)
            assert il.edge_margin(want, 1) > 1e-9, (name, nr, nphi, shift)
            assert want["binned"] > 100 and want["disc_count"] >= want["binned"]
            if name == "offaxis" and nphi > 1:
                ring = want["count"].sum(axis=0)
                assert ring.max() > 3 * max(ring.min(), 1)
