"""GPU: the equatorial-crossing recorder (kr_trace_crossings_*), its image reducer (kr_reduce_crossing_image_dev_f64), the resident pipeline
(api.order_images) and the program (kr_imageplane_orders) against the numpy rule of tests/crossing_rules.py applied to the path recorder's
write_step = 1 rows -- the recorder is pinned to the reference's own trajectory files and to the strict trace by tests/test_gpu_paths.py, the energy
shift comes from the CPU oracle.

r_c, phi_c and t_c are a handful of IEEE operations on states the path tests pin bit for bit: they are held to the rule's BITS.  g: parity.RAY_RTOL.
The shapes are the committed fixtures, free-running (theta_max = 0) so that the rays go on through the plane: ps_h5_a05 (2604 slots; RK4: 965 / 1298
/ 105 / 2 rays with 0 / 1 / 2 / 3 crossings once the marked rays are taken out, Euler up to 6) and ip16 (289 slots; 17 / 205 / 48 / 1).

Measured on MI355X: all 42 cases pass in 3.3 s; seen equal and r_c / phi_c / t_c bit for bit in every case, g EQUAL to the oracle's (worst relative
difference 0), the image sums within 2.9e-16 of the rule's (the ISCO case: the oracle ends 1042 rays on the destination, in an iteration that is a crossing).
The order-2 image of ip16 is empty (one ray crosses three times, not on the disc); orders 0, 1 and the opaque disc hold 42, 9 and 47 rays."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import crossing_rules as cr
import golden_cases as gc
import parity
import reducer_rules as rr
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu


def free_running(spin, integrator, r_max, steplim, **kw):
    return capi.copy_params(capi.default_params(spin), integrator=integrator, r_max=r_max, steplim=steplim, theta_max=0.0, flags=0, **kw)


def case_params(name, steplim=None):
    """(fixture, params, reverse) of a case of the table in the module docstring"""
    if name == "ps_rk4":
        return "ps_h5_a05", free_running(0.5, capi.RK4, 100.0, steplim or 4000), 0
    if name == "ps_euler":
        return "ps_h5_a05", free_running(0.5, capi.EULER, 100.0, steplim or 4000), 0
    if name == "ps_isco":
        return "ps_h5_a05", free_running(0.5, capi.RK4, 100.0, steplim or 4000, stop_kind=capi.STOP_DISC_ISCO, stop_params=(gc.r_isco(0.5), 400.0, np.pi / 2)), 0
    if name == "ip16_rk4":
        return "ip16", free_running(-gc.SPIN, capi.RK4, 11000.0, steplim or 20000), 1
    raise KeyError(name)


def spec_for(name, M, stop):
    return api.crossing_spec(max_crossings=M, stop_when_full=stop, V=-1.0, reverse=case_params(name)[2])


@functools.lru_cache(maxsize=None)
def recording(name):
    """(params, init, offsets, rows, traced, the strict trace's records, every crossing of the recorded paths) of a golden init with every 17th ray
    unused and one beyond the step limit; computed once, read-only"""
    fixture, p, _ = case_params(name)
    init = np.load(gc.golden_path(fixture))["init"].copy()
    init["steps"][::17] = -1
    init["steps"][5] = capi.STEPLIM + 1
    offsets, rows, traced, out, _ = api.trace_paths(p, init, write_step=1)
    want, _ = api.trace(p, init)
    assert parity.same_records(out, want)
    assert (init["emit"][traced.astype(bool)] != 0).all() and (init["status"] == 0).all()
    found = cr.all_crossings(p, init, offsets, rows, traced, want)
    for a in (init, offsets, rows, traced, want):
        a.setflags(write=False)
    return p, init, offsets, rows, traced, want, found


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


NAN_BITS = np.array([np.nan]).view(np.uint64)[0]


def check_against_rule(test, label, got, want, init, records, traced, M, window=None):
    """The assertions of case 1 on the rays window = (first, count) (all of them by default); returns the worst relative g error."""
    sl = slice(window[0], window[0] + window[1]) if window else slice(0, len(init))
    seen, rows = got["seen"], got["rows"]
    w_seen, w_rows, ended = want["seen"][sl], want["rows"][sl], want["ended"][sl]
    assert np.array_equal(seen, w_seen), (label, np.flatnonzero(seen != w_seen)[:8])
    stored = np.arange(M)[None, :] < np.minimum(seen, M)[:, None]
    # where and when: the rule's bits
    for q, what in enumerate(("r_c", "phi_c", "t_c")):
        ok = same_bits(rows[:, :, q], w_rows[:, :, q])
        assert ok[stored].all(), (label, what, np.argwhere(stored & ~ok)[:8])
    # the energy shift: the oracle's within RAY_RTOL, NaN alike
    g, wg = rows[:, :, 3][stored], w_rows[:, :, 3][stored]
    assert np.array_equal(np.isnan(g), np.isnan(wg)), label
    fin = ~np.isnan(wg)
    with np.errstate(invalid="ignore"):
        err = np.where(g[fin] == wg[fin], 0.0, np.abs(g[fin] - wg[fin]) / np.maximum(np.abs(wg[fin]), 1.0))
    worst = float(err.max()) if err.size else 0.0
    print(f"crossings {label}: rays with 0 / 1 / 2 / .. crossings {np.bincount(seen[traced[sl].astype(bool)]).tolist()}, stored rows {int(stored.sum())}, ended by the recorder "
          f"{int(ended.sum())}, worst relative g error {worst:.2e}, kernel {got['stats']['kernel_ms']:.2f} ms")
    assert worst <= parity.RAY_RTOL, (label, worst)
    # rows beyond min(seen, M) keep the pre-fill's bits
    assert (rows.view(np.uint64)[~stored] == NAN_BITS).all(), label
    # a ray the recorder did not end finishes with the flags = 0 trace's record, and seen is the increase of its crossing counter
    keep = ~ended
    assert parity.same_records(got["rays"][keep], records[sl][keep]), label
    live = traced[sl].astype(bool)
    assert np.array_equal(seen[keep & live], (records["equatorial_crossings"][sl] - init["equatorial_crossings"][sl])[keep & live]), label
    assert (seen[~live] == 0).all() and got["rays"][~live].tobytes() == init[sl][~live].tobytes(), label
    # a ray it did end made exactly M crossings and stands where that iteration left it
    assert (seen[ended] == M).all(), label
    for q, f in enumerate(cr.COLS):
        assert same_bits(got["rays"][f][ended], want["end_state"][sl][ended, q]).all(), (label, f)
    assert np.array_equal((got["rays"]["equatorial_crossings"] - init["equatorial_crossings"][sl])[live], seen[live]), label
    assert got["stats"]["rays_traced"] == int(live.sum()), label
    parity.record_margin(test, label, {"n_traced": int(live.sum()), "n_bad": 0, "frac_bad": 0.0, "worst_ok": worst}, allowed=parity.RAY_RTOL,
                         bar="seen equal, r_c / phi_c / t_c bit for bit; worst_ok = worst relative g error against the oracle", stored_rows=int(stored.sum()),
                         ended_by_recorder=int(ended.sum()))
    return worst


CASES = ["ps_rk4", "ps_euler", "ps_isco", "ip16_rk4"]


@pytest.mark.parametrize("stop", [False, True], ids=["run_on", "stop_when_full"])
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("name", CASES)
def test_rows_are_the_rule_applied_to_the_recorded_path(name, M, stop):
    p, init, offsets, rows, traced, records, found = recording(name)
    spec = spec_for(name, M, stop)
    got = api.trace_crossings(p, init, spec)
    want = cr.rule(p, spec, init, offsets, rows, traced, records, found=found)
    check_against_rule("test_rows_are_the_rule_applied_to_the_recorded_path", f"{name}-M{M}-{'stop' if stop else 'run'}", got, want, init, records, traced, M)
    # not vacuous (bounds: the oracle's crossing counts on these fixtures, less the marked rays)
    seen = got["seen"]
    if name.startswith("ps_"):
        per_ray = np.bincount(found["ray"], minlength=len(init))
        assert (per_ray >= 2).sum() >= 30
        if M == 1:
            assert (per_ray > M).sum() >= 30 and ((seen > M).sum() >= 30 or stop)
        if stop:
            assert want["ended"].sum() >= (30 if M <= 2 else 0) and (seen <= M).all()
    if name == "ps_isco":
        last = found["ordinal"] == (np.bincount(found["ray"], minlength=len(init))[found["ray"]] - 1)
        on_dest = (records["status"][found["ray"]] & capi.STATUS_DEST) != 0
        assert (last & found["in_break"] & on_dest).sum() >= 500


@pytest.mark.parametrize("start", [0, 390], ids=["leading", "from390"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_wave_edges(n, start):
    """n leading rays of ps_h5_a05 -- of which none meets the plane (they leave upwards): seen = 0 and no row written, slot for slot -- and n rays from
    slot 390 on, where the oracle has 17 / 67 / 46 rays with 0 / 1 / 2 crossings among 130 (7 with two among the first 63): M = 2 with stop_when_full ends those."""
    p, init, offsets, rows, traced, records, found = recording("ps_rk4")
    spec = spec_for("ps_rk4", 2, True)
    got = api.trace_crossings(p, init[start:start + n].copy(), spec)
    want = cr.rule(p, spec, init, offsets, rows, traced, records, found=found)
    check_against_rule("test_wave_edges", f"ps_rk4-{start}+{n}", got, want, init, records, traced, 2, window=(start, n))
    if start and n >= 63:
        assert (got["seen"] == 2).sum() >= (40 if n == 130 else 6)          # (the oracle: 7, 7, 7 and 46 rays with two crossings in these windows)


def test_lanes_are_reused():
    """The init tiled 8 x (20 832 rays, more than one pass of the launch's lanes on a wave's slots): every copy's rows and seen are bitwise those of the
    first, which a `seen`, an emit or a slab that leaked from a lane's previous ray would break."""
    p, init, *_ = recording("ps_rk4")
    tiles = 8
    for stop in (False, True):
        got = api.trace_crossings(p, np.tile(init, tiles), spec_for("ps_rk4", 2, stop))
        rows, seen = got["rows"].reshape(tiles, len(init), 2, 4), got["seen"].reshape(tiles, len(init))
        for k in range(1, tiles):
            assert rows[k].tobytes() == rows[0].tobytes() and np.array_equal(seen[k], seen[0]), (stop, k)
        assert (seen[0] >= 2).sum() >= 30 and parity.same_records(got["rays"][:len(init)], got["rays"][-len(init):])


@pytest.mark.parametrize("steplim", [300, 600])
def test_second_call_traces_only_what_the_skip_rule_lets_through(steplim):
    """Calling again on the output records of a short run.  steplim = 300 stops EVERY ray of this fixture at the limit (the oracle: 2371 of 2371), so the
    second call traces nothing; steplim = 600 leaves 1102 at the limit and lets 1269 finished rays through, which are traced from where they stand."""
    fixture, p, _ = case_params("ps_rk4", steplim=steplim)
    init = np.load(gc.golden_path(fixture))["init"].copy()
    init["steps"][::17] = -1
    spec = spec_for("ps_rk4", 4, False)
    first = api.trace_crossings(p, init, spec)
    mid = first["rays"]
    skipped = (mid["steps"] < 0) | (mid["steps"] >= steplim)
    at_limit = (mid["status"] & capi.STATUS_STEPLIM) != 0
    # (the oracle: 1 crossing within 300 steps on this fixture, 1511 within 600; a photon-sphere ray in a hundred -- parity.CHAOTIC_FRAC -- may differ)
    assert (mid["steps"][at_limit] == -steplim).all() and (first["seen"].sum() <= 25 if steplim == 300 else first["seen"].sum() >= 1511 - 25)
    assert at_limit.sum() >= 1000 and (steplim == 300 or (~skipped).sum() >= 1000)
    second = api.trace_crossings(p, mid, spec)
    want, _ = api.trace(p, mid)
    assert parity.same_records(second["rays"], want)
    assert second["stats"]["rays_traced"] == int((~skipped).sum())
    assert (second["seen"][skipped] == 0).all() and (second["rows"].view(np.uint64)[skipped] == NAN_BITS).all()
    assert second["rays"][skipped].tobytes() == mid[skipped].tobytes()
    assert np.array_equal(second["seen"], want["equatorial_crossings"] - mid["equatorial_crossings"])


# ---- the image reducer ---------------------------------------------------------------------------------------------------------------------------
PREFILL = 3.0


def image_setup():
    name = "ip16_rk4"
    p, init, *_ = recording(name)
    spec = spec_for(name, 4, True)
    got = api.trace_crossings(p, init, spec)
    bins = gc.image_bins(gc.cases()["ip16"]["source"])
    return bins, got


@pytest.mark.parametrize("order", [0, 1, -1])
def test_image_of_one_order(krlib, order):
    """ip16 (17 x 17 rays) into the 8 x 8 image of gc.image_bins, against the image rule on the device's own rows: counts exact, sums within
    parity.BIN_RTOL (the bar of tests/test_gpu_reducers.py); the reducer adds into what the buffer holds."""
    L = krlib
    bins, got = image_setup()
    rays, rows, seen = got["rays"], got["rows"], got["seen"]
    want = cr.image_rule(bins, rays, rows, seen, order)
    img = api.reduce_crossing_image(bins, rays, rows, seen, order)
    worst = rr.check_reduction(img, want, "nrays", rr.IMAGE_SUMS, parity.BIN_RTOL, f"order {order}")
    print(f"crossing image order {order}: {img['disc_count']} rays in {int((img['nrays'] > 0).sum())} of {img['nrays'].size} pixels, worst relative sum error {worst:.2e}")
    assert img["disc_count"] > 0, "the plane of this order is empty at 17 x 17 rays"
    if order == 1:
        direct = api.reduce_crossing_image(bins, rays, rows, seen, 0)
        assert img["disc_count"] < direct["disc_count"] and not np.array_equal(img["nrays"], direct["nrays"])
    parity.record_margin("test_image_of_one_order", f"ip16-order{order}", {"n_traced": int(img["disc_count"]), "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(worst)},
                         allowed=parity.BIN_RTOL, bar="counts exact; worst_ok = worst |sum - rules| / per-bin sum of absolute terms")
    # it adds: a pre-filled buffer ends as the pre-fill plus the image
    nw = api.image_words(bins)
    with DeviceScope(L) as dev:
        bufs = [dev.upload(a) for a in (rays, np.ascontiguousarray(rows), seen, np.full(nw, PREFILL))]
        capi.check(L, L.kr_reduce_crossing_image_dev_f64(C.byref(bins), rows.shape[1], order, -np.pi, np.pi, bufs[0], bufs[1], bufs[2], len(rays), bufs[3], None), "reduce")
        capi.check(L, L.kr_synchronize(None), "sync")
        words = dev.fetch(bufs[3], nw)
    filled = api.image_planes_from_words(words - PREFILL, bins.img_nx, bins.img_ny)
    assert np.array_equal(filled["nrays"], want["nrays"]) and filled["disc_count"] == want["disc_count"]
    untouched = want["nrays"] == 0
    for q in range(7):
        assert (words[q * untouched.size:(q + 1) * untouched.size][untouched] == PREFILL).all()


# ---- the pipeline and the program --------------------------------------------------------------------------------------------------------------
APPS = os.path.join(gc.ROOT, "tests", "golden", "apps")
EXE = os.path.join(gc.ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_imageplane_orders")
ORDERS = [0, 1, 2, -1]


@functools.lru_cache(maxsize=None)
def pipeline():
    """api.order_images on the ip16 plane as kr_imageplane_orders runs tests/golden/apps/imageplane_orders.par"""
    ip = gc.cases()["ip16"]["source"]
    _, p, reverse = case_params("ip16_rk4")
    spec = api.crossing_spec(max_crossings=3, stop_when_full=True, V=-1.0, reverse=reverse)
    bins = gc.image_bins(ip)
    return ip, p, spec, bins, api.order_images(ip, p, bins, spec, ORDERS)


def test_order_images_equals_the_separate_calls():
    ip, p, spec, bins, res = pipeline()
    rays = api.imageplane_init(ip)
    api.redshift_start(-1 * ip.spin, 0.0, 1, 0, rays)
    sep = api.trace_crossings(p, rays, spec)
    assert np.array_equal(res["seen_histogram"], np.bincount(sep["seen"])) and res["stats"]["steps_total"] == sep["stats"]["steps_total"]
    for order in ORDERS:
        one = api.reduce_crossing_image(bins, sep["rays"], sep["rows"], sep["seen"], order)
        img = res["images"][order]
        assert np.array_equal(img["nrays"], one["nrays"]) and img["disc_count"] == one["disc_count"], order
        assert one["disc_count"] > 0 or order == 2, order          # (one ray of this plane crosses three times, and not on the disc: the order-2 image is empty)
        for k in rr.IMAGE_SUMS:
            assert img[k].tobytes() == one[k].tobytes(), (order, k)
    assert res["images"][1]["disc_count"] > 0 and res["images"][-1]["disc_count"] >= res["images"][0]["disc_count"]


def test_program_writes_one_file_per_order():
    """kr_imageplane_orders on the ip16 geometry: every FITS plane is the pipeline's plane divided as the writer divides it (1e-12, the bar of the other
    app tests), empty pixels NaN alike; the primary header carries ORDER and MAXORD."""
    import fits_lite
    assert os.path.exists(EXE), f"{EXE} not built (make -C raytrace_cpu_amd/apps)"
    ip, p, spec, bins, res = pipeline()
    with tempfile.TemporaryDirectory() as w:
        out = os.path.join(w, "img.fits")
        r = subprocess.run([EXE, f"--parfile={os.path.join(APPS, 'imageplane_orders.par')}", f"--outfile={out}", "--timing"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "timing: rays" in r.stdout
        assert sorted(os.listdir(w)) == ["img_n0.fits", "img_n1.fits", "img_n2.fits", "img_opaque.fits"]
        files = {order: fits_lite.read(os.path.join(w, "img_opaque.fits" if order < 0 else f"img_n{order}.fits")) for order in ORDERS}
    nx, ny = bins.img_nx, bins.img_ny
    for order, hdus in files.items():
        assert [h["name"] for h in hdus] == ["PRIMARY", "FLUX", "RADIUS", "PHI", "ENSHIFT", "TIME", "EMIS"]
        head = hdus[0]["header"]
        img = res["images"][order]
        assert int(float(head["ORDER"])) == order and int(float(head["MAXORD"])) == 2 and int(float(head["DISCRAYS"])) == img["disc_count"]
        assert int(float(head["NRAYS"])) == 16 * 16 and float(head["SPIN"]) == gc.SPIN
        hits = img["nrays"].reshape(nx, ny)
        empty = hits == 0
        assert not empty.all() or order == 2
        for name, key in zip(("FLUX", "RADIUS", "PHI", "ENSHIFT", "TIME", "EMIS"), rr.IMAGE_SUMS):
            got = np.asarray({h["name"]: h for h in hdus}[name]["data"], dtype=np.float64).T          # (fits_lite gives [iy][ix])
            assert got.shape == (nx, ny)
            with np.errstate(invalid="ignore", divide="ignore"):
                want = img[key].reshape(nx, ny) / hits
            if key == "flux":
                # (the writer divides the flux only where rays arrived: an empty pixel keeps its 0)
                assert (got[empty] == 0).all(), (order, name)
            else:
                assert np.isnan(got[empty]).all(), (order, name)
            np.testing.assert_allclose(got[~empty], want[~empty], rtol=1e-12, atol=0, err_msg=f"{order} {name}")
