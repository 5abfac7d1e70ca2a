"""GPU: the landing map of the returning radiation (raytrace_cpu_amd/csrc/kr_return_map.hip: return_map_kernel<USE_LDS, FUSED>,
return_map_multi_kernel) against the numpy rule of tests/return_map_rules.py, which tests/test_return_map_rules.py ties to the return and emissivity
rule sets: the reducing forms on the chosen records of tests/reducer_cases.py (nr on either side of the LDS capacity, both bin kinds, all eight
weight cases, a size at which the grid-stride loop wraps, a pre-filled buffer), the fused pass against the separate passes, a batch of 49 against 49
single calls, the resident pipeline api.return_radiation against its own records, the oracle's records and the rules, and the kr_return_radiation
program against the pipeline.

The bar is the one of tests/test_gpu_reducers.py: count planes, on_disc and binned exact; every sum within parity.BIN_RTOL of its per-bin sum of
absolute terms; non-finite bins alike; the worst relative sum error of every case goes to the margins file (parity.record_margin)."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fits_lite
import golden_cases as gc
import oracle_lib as ol
import parity
import reducer_cases as rc
import reducer_rules as rr
import return_map_rules as rm
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope
from test_gpu_reducers import device_words, fetch, upload

pytestmark = pytest.mark.gpu
vp = C.c_void_p
RTOL = parity.BIN_RTOL
REORDER_RTOL = 1e-12               # the same terms added in another order (tests/test_gpu_batch_passes.py)
NRS = (1, 7, 1024, 1025)
WRAP = (-math.pi, math.pi)
PASS = (gc.SPIN, -1.0, 0, 0, 0) + WRAP


@pytest.fixture
def dev(krlib):
    """Device buffers of one test, freed at its end."""
    with DeviceScope(krlib) as scope:
        yield scope


def landing_map(case, nr, logbin):
    eb = rc.emis_bins(nr, logbin)
    return rm.map_struct(rc.return_cases()[case], eb.r_min, eb.dr, nr, logbin, eb.gamma)


def margin(test, case, n, worst, **extra):
    parity.record_margin(test, case, {"n_traced": int(n), "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(worst)}, allowed=RTOL,
                         bar="counts exact; worst_ok = worst |sum - rules| / per-bin sum of absolute terms", **extra)


def check(got, want, m, label):
    """One landing map (api.return_map_from_words) against the rules: the bar of the module docstring; returns the worst relative sum error."""
    worst = rm.check_map(got, want, RTOL, label)
    return max(worst, rr.check_return(rm.scalars_of(got), want["scalars"], RTOL, not m.cls.weight_norm, label))


def dev_reduce(dev, m, d_rays, n, d_out=None, first=0):
    d_out = d_out or device_words(dev, 5 * m.nr + 6)
    capi.check(dev.lib, dev.lib.kr_reduce_return_map_dev_f64(C.byref(m), vp(d_rays.value + 144 * first), n, d_out, None), "kr_reduce_return_map_dev")
    return d_out


def fetch_map(dev, m, d_out):
    return api.return_map_from_words(m, fetch(dev, d_out, 5 * m.nr + 6))


# ---- the reducing forms ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_on_device(krlib):
    with DeviceScope(krlib) as scope:
        yield upload(scope, rc.small().return_rays)


REDUCE_CASES = [(case, nr, lb) for case in sorted(rc.return_cases()) for nr in NRS for lb in (0, 1)]


@pytest.mark.parametrize("case,nr,logbin", REDUCE_CASES, ids=[f"{c}-{'log' if lb else 'lin'}-nr{nr}" for c, nr, lb in REDUCE_CASES])
def test_reduce_forms_match_the_rules(dev, small_on_device, case, nr, logbin):
    """return_map_kernel<true, false> (nr <= 1024) and <false, false> (1025), device form and host form, on every record of the small set: the
    NaN-weight and poison records make the sums they enter NaN or infinite on both sides."""
    rays = rc.small().return_rays
    m = landing_map(case, nr, logbin)
    want = rm.reduce_return_map(m, rays)
    label = f"{case}-{'log' if logbin else 'lin'}-nr{nr}"
    worst = check(fetch_map(dev, m, dev_reduce(dev, m, small_on_device, len(rays))), want, m, label + " (device form)")
    worst = max(worst, check(api.reduce_return_map(m, np.ascontiguousarray(rays)), want, m, label + " (host form)"))
    print(f"return map {label}: on_disc {want['on_disc']}, binned {want['binned']}, fullest bin {int(want['count'].max())}, worst sum error {worst:.3g}")
    margin("test_reduce_forms_match_the_rules", label, len(rays), worst, on_disc=want["on_disc"], binned=want["binned"])


def test_reduce_form_on_the_large_set(dev):
    """262 465 records: the 1024-workgroup grid wraps, with a ragged tail."""
    large = rc.large()
    rays = large.return_rays[~large.nan_weight]
    assert len(rays) > 1024 * 256 and len(rays) % 256
    m = landing_map("iso1-limb1-norm1", 7, 1)
    want = rm.reduce_return_map(m, rays)
    worst = check(fetch_map(dev, m, dev_reduce(dev, m, upload(dev, rays), len(rays))), want, m, "large")
    assert want["binned"] > 10 * rc.N_CONTENTION
    margin("test_reduce_form_on_the_large_set", "iso1-limb1-norm1-log-nr7", len(rays), worst, binned=want["binned"])


@pytest.mark.parametrize("nr", [7, 1025])
def test_reduce_form_adds_into_the_callers_buffer(dev, nr):
    """Two calls over the halves of the set into one buffer == the rules on the whole; a call into a pre-filled buffer adds to the pre-fill."""
    rec = rc.small()
    rays = rec.return_rays[~rec.nan_weight & ~rec.poison]
    m = landing_map("iso0-limb0-norm0", nr, 1)
    n, half, words, prefill = len(rays), len(rays) // 2 + 1, 5 * nr + 6, 1000.0
    want = rm.reduce_return_map(m, rays)
    d_rays = upload(dev, rays)
    halves = dev_reduce(dev, m, d_rays, half)
    dev_reduce(dev, m, d_rays, n - half, halves, first=half)
    margin("test_reduce_form_adds_into_the_callers_buffer", f"nr{nr}", n, check(fetch_map(dev, m, halves), want, m, "halves"))
    filled = api.return_map_from_words(m, fetch(dev, dev_reduce(dev, m, d_rays, n, device_words(dev, words, prefill)), words) - prefill)
    assert np.array_equal(filled["count"], want["count"]) and np.array_equal(filled["weight"], want["count"])     # unit weights: whole numbers, exact
    assert filled["on_disc"] == want["on_disc"] and filled["binned"] == want["binned"] and np.array_equal(rm.scalars_of(filled), want["scalars"])


# ---- the fused pass --------------------------------------------------------------------------------------------------------------------------
def records_with_a_poisoned_redshift():
    rays = rc.small().return_rays.copy()
    rays["redshift"] = np.where(np.arange(len(rays)) % 2, -7.0, np.nan)
    return rays


FUSED_CASES = [("iso1-limb0-norm1", 7, 1), ("iso1-limb1-norm0", 1024, 0), ("iso0-limb0-norm1", 1025, 1), ("iso1-limb1-norm1", 1025, 0)]


@pytest.mark.parametrize("case,nr,logbin", FUSED_CASES, ids=[f"{c}-{'log' if lb else 'lin'}-nr{nr}" for c, nr, lb in FUSED_CASES])
def test_fused_pass_equals_the_separate_passes(krlib, dev, case, nr, logbin):
    """kr_post_return_map_dev_f64 == kr_range_phi_dev_f64 + kr_redshift_dev_f64(V = -1) + kr_reduce_return_map_dev_f64: records bit for bit, counts
    exact, sums up to the order of the additions, and both maps against the rules on those records."""
    lib = krlib
    m = landing_map(case, nr, logbin)
    rays = records_with_a_poisoned_redshift()
    n = len(rays)
    d_sep, d_fused = upload(dev, rays), upload(dev, rays)
    capi.check(lib, lib.kr_range_phi_dev_f64(*WRAP, d_sep, n, None), "range_phi")
    capi.check(lib, lib.kr_redshift_dev_f64(gc.SPIN, -1.0, 0, 0, 0, d_sep, n, None), "redshift")
    o_sep = dev_reduce(dev, m, d_sep, n)
    o_fused = device_words(dev, 5 * nr + 6)
    capi.check(lib, lib.kr_post_return_map_dev_f64(*PASS, C.byref(m), d_fused, n, o_fused, None), "kr_post_return_map_dev")
    sep, fused = fetch(dev, d_sep, n, capi.RAY_F64), fetch(dev, d_fused, n, capi.RAY_F64)
    assert parity.same_records(sep, fused)
    live = rays["steps"] > 0
    assert (sep["phi"] != rays["phi"]).sum() > 1000 and (sep["redshift"][live] > 0).sum() > rc.N_CONTENTION
    got_sep, got_fused = fetch_map(dev, m, o_sep), fetch_map(dev, m, o_fused)
    assert np.array_equal(got_sep["count"], got_fused["count"]) and got_sep["on_disc"] == got_fused["on_disc"] and got_sep["binned"] == got_fused["binned"]
    for k in rm.MAP_SUMS + rm.SCALARS:
        np.testing.assert_allclose(got_fused[k], got_sep[k], rtol=REORDER_RTOL, atol=0, equal_nan=True, err_msg=k)
    want = rm.reduce_return_map(m, sep)
    assert want["binned"] > rc.N_CONTENTION
    worst = max(check(got, want, m, (case, name)) for name, got in (("separate", got_sep), ("fused", got_fused)))
    margin("test_fused_pass_equals_the_separate_passes", f"{case}-nr{nr}", n, worst, binned=want["binned"])


# ---- the batch -------------------------------------------------------------------------------------------------------------------------------
def test_batch_of_49_equals_the_single_calls(krlib, dev):
    """kr_post_return_map_batch_dev_f64 with two full chunks of 24 and a remainder of one, unequal sizes, item 5 empty, nr cycling through 7, 100 and
    1025 inside every chunk (LDS and global workgroups in one launch), limb alternating: records bit for bit, counts identical, sums at 1e-12."""
    lib = krlib
    rec = rc.small()
    rays = records_with_a_poisoned_redshift()[~rec.nan_weight & ~rec.poison]
    k = 49
    sizes = [0 if j == 5 else 5 + 3 * j for j in range(k - 1)]
    sizes.append(len(rays) - sum(sizes))                                    # the last one takes the rest, the contention block with it
    assert sizes[-1] > rc.N_CONTENTION and len(set(sizes)) == k
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    cases = sorted(rc.return_cases())
    maps = []
    for j in range(k):
        m = landing_map(cases[j % 8], (7, 100, 1025)[j % 3], j % 2)
        m.cls.limb = j % 2
        maps.append(m)
    offs = np.concatenate([[0], np.cumsum([5 * m.nr + 6 for m in maps])]).astype(int)
    d_single, d_batch = upload(dev, rays), upload(dev, rays)
    o_single, o_batch = device_words(dev, int(offs[-1])), device_words(dev, int(offs[-1]))
    for j in range(k):
        capi.check(lib, lib.kr_post_return_map_dev_f64(*PASS, C.byref(maps[j]), vp(d_single.value + 144 * int(starts[j])), sizes[j],
                                                       vp(o_single.value + 8 * int(offs[j])), None), "kr_post_return_map_dev")
    ptrs = (vp * k)(*[d_batch.value + 144 * int(starts[j]) for j in range(k)])
    outs = (vp * k)(*[o_batch.value + 8 * int(offs[j]) for j in range(k)])
    capi.check(lib, lib.kr_post_return_map_batch_dev_f64(k, *PASS, (capi.ReturnMap * k)(*maps), ptrs, (C.c_int64 * k)(*sizes), outs, None), "kr_post_return_map_batch_dev")
    single, batch = fetch(dev, o_single, int(offs[-1])), fetch(dev, o_batch, int(offs[-1]))
    assert parity.same_records(fetch(dev, d_single, len(rays), capi.RAY_F64), fetch(dev, d_batch, len(rays), capi.RAY_F64))
    worst, binned = 0.0, 0
    for j in range(k):
        m = maps[j]
        s, b = (api.return_map_from_words(m, w[offs[j]:offs[j + 1]]) for w in (single, batch))
        assert np.array_equal(s["count"], b["count"]) and s["on_disc"] == b["on_disc"] and s["binned"] == b["binned"], j
        for key in rm.MAP_SUMS + rm.SCALARS:
            np.testing.assert_allclose(b[key], s[key], rtol=REORDER_RTOL, atol=0, equal_nan=True, err_msg=f"item {j} {key}")
        binned += b["binned"]
        if j == 5:
            assert not single[offs[j]:offs[j + 1]].any() and not batch[offs[j]:offs[j + 1]].any()
        else:
            assert b["ray_count"] > 0
    # the last item (the contention block) and a small one of each nr against the rules as well
    sep = fetch(dev, d_batch, len(rays), capi.RAY_F64)
    for j in (0, 1, 2, k - 1):
        want = rm.reduce_return_map(maps[j], sep[starts[j]:starts[j + 1]])
        worst = max(worst, check(api.return_map_from_words(maps[j], batch[offs[j]:offs[j + 1]]), want, maps[j], (j, "batch against the rules")))
    assert binned > rc.N_CONTENTION
    margin("test_batch_of_49_equals_the_single_calls", "49 items", len(rays), worst, binned=binned)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
E2E_RADII = [1.3, 2.0, 3.7, 6.0, 11.0, 40.0, 150.0]
E2E = dict(dcosalpha=0.04, dbeta=0.04 * math.pi, r_disc=500.0, r_esc=500.0, nr=32, logbin=True)
E2E_RETURNING = [530, 370, 260, 198, 132, 50, 18]          # computed with the oracle: returning rays per radius


def e2e_params():
    p = capi.default_params(gc.SPIN)
    p.integrator, p.theta_max, p.r_max, p.stop_kind, p.flags = capi.EULER, math.pi / 2, 1.1 * E2E["r_esc"], capi.STOP_THETA, 0
    return p


def e2e_map(r_s, nr=None, r_min=None):
    r_min = gc.r_isco() if r_min is None else r_min
    nr = E2E["nr"] if nr is None else nr
    return api.return_map_struct(gc.r_isco(), E2E["r_disc"], E2E["r_esc"], r_s, 1.5707, r_min, math.exp(math.log(E2E["r_disc"] / r_min) / nr), nr, 1)


def oracle_records(r_s):
    """disc_source_photonfrac_r.cpp:89-94 with the oracle: PointSource, redshift_start, Euler to theta = pi / 2 or 1.1 r_esc, range_phi, redshift(-1)."""
    V = ol.oracle().kro_disc_velocity(r_s, gc.SPIN, 1)
    spec = ol.pointsource_spec([0.0, r_s, math.pi / 2 - 1e-6, 1.5707], V, gc.SPIN, E2E["dcosalpha"], E2E["dbeta"], cosalpha0=-0.995, cosalphamax=0.995, beta0=0.0,
                               betamax=math.pi)
    init = ol.oracle_pointsource(spec)
    ol.oracle().kro_redshift_start_f64(gc.SPIN, V, 0, 0, ol.ptr(init), len(init))
    out, _ = ol.oracle_trace(e2e_params(), init)
    ol.oracle().kro_range_phi_f64(*WRAP, ol.ptr(out), len(out))
    ol.oracle().kro_redshift_f64(gc.SPIN, -1.0, 0, 0, 0, ol.ptr(out), len(out))
    return out


def test_pipeline_against_its_records_the_oracle_and_the_rules(krlib):
    """api.return_radiation at the smallest grids that still show every class: (i) the map is the rules applied to the device's own records;
    (ii) those records meet the strict bar against the oracle's; (iii) against the rules on the oracle's records each count plane differs by at
    most the number of rays (ii) found different -- 0 on every PointSource fixture so far, and then the comparison is exact."""
    res = api.return_radiation(gc.SPIN, E2E_RADII, flags=0, return_records=True, **E2E)
    assert res["r_isco"] == gc.r_isco() and res["count"].shape == (7, 32) and res["stats"]["rays_traced"] == 7 * 1250
    p = e2e_params()
    for i, r_s in enumerate(E2E_RADII):
        m, rec = res["maps"][i], res["records"][i]
        assert len(rec) == 1319 and (rec["steps"] != -1).sum() == 1250
        got = {k: res[k][i] for k in api.RETURN_MAP_PLANES}
        got.update({k: float(res[k][i]) for k in rm.SCALARS}, on_disc=int(res["on_disc"][i]), binned=int(res["binned"][i]))
        worst = check(got, rm.reduce_return_map(m, rec), m, (r_s, "the device's own records"))                       # (i)
        want_rec = oracle_records(r_s)
        cmp = parity.compare_rays(rec, want_rec, rtol=parity.RAY_RTOL, check_redshift=True, steps_slack=0)             # (ii)
        allowed = parity.allowed_bad_frac_strict(p, cmp["n_traced"])
        parity.record_margin("test_pipeline_against_its_records_the_oracle_and_the_rules", f"r_s={r_s}", cmp, allowed=allowed, map_worst_sum_error=worst)
        assert cmp["frac_bad"] <= allowed, (r_s, cmp)
        want = rm.reduce_return_map(m, want_rec)                                                                       # (iii)
        assert want["on_disc"] == E2E_RETURNING[i] and want["scalars"][1] > 0 and want["scalars"][2] > 0
        assert np.abs(got["count"] - want["count"]).max() <= cmp["n_bad"], (r_s, cmp["n_bad"])
        assert abs(got["on_disc"] - want["on_disc"]) <= cmp["n_bad"] and abs(got["binned"] - want["binned"]) <= cmp["n_bad"]
        if cmp["n_bad"] == 0:
            rm.check_map(got, want, RTOL, (r_s, "the oracle's records"))
            rr.check_return(rm.scalars_of(got), want["scalars"], RTOL, False, (r_s, "the oracle's records"))
        print(f"return radiation r_s = {r_s}: return fraction {got['return'] / got['ray_count']:.4g}, on_disc {got['on_disc']}, binned {got['binned']}, "
              f"rays beyond the bar {cmp['n_bad']}, worst sum error {worst:.3g}")
    assert (res["lost"][:4] > 0).all() and res["binned"].sum() == sum(E2E_RETURNING) - 1            # every class; one returning ray with g <= 0 (r_s = 2.0)
    frac = res["return"] / res["ray_count"]
    assert (np.diff(frac) < 0).all() and 0.4 < frac[0] < 0.6 and frac[-1] < 0.01


# ---- the program -----------------------------------------------------------------------------------------------------------------------------
APPS = os.path.join(gc.ROOT, "tests", "golden", "apps")
EXE = os.path.join(gc.ROOT, "raytrace_cpu_amd", "apps", "_build", "kr_return_radiation")


def test_program_writes_the_table_and_the_landing_map(krlib):
    """kr_return_radiation on three radii: the table's fractions are the rules' on the pipeline's records (1e-6, the bar of the app tests); the five
    FITS planes are the planes of api.return_radiation divided as the program divides them (1e-12), NaN where nothing landed."""
    assert os.path.exists(EXE), f"{EXE} not built (make -C raytrace_cpu_amd/apps)"
    nr = 3
    with tempfile.TemporaryDirectory() as w:
        dat, fits = os.path.join(w, "out.dat"), os.path.join(w, "map.fits")
        par = os.path.join(w, "return_radiation.par")
        with open(par, "w") as f:
            f.write(open(os.path.join(APPS, "return_radiation.par")).read().replace("unused.fits", fits))
        r = subprocess.run([EXE, f"--parfile={par}", f"--outfile={dat}", "--arithmetic=strict", "--timing"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "timing: radii 3" in r.stdout
        table = np.array([[float(x) for x in line.split()] for line in open(dat) if line.strip()])
        hdus = fits_lite.read(fits)
    r_min = gc.r_isco()
    dr = math.exp(math.log(500.0 / r_min) / nr)
    radii = [r_min * math.pow(dr, ir) for ir in range(nr)]
    res = api.return_radiation(gc.SPIN, radii, 0.04, 0.12566370614359174, r_disc=500.0, r_esc=500.0, nr=nr, logbin=True, flags=0, return_records=True)
    assert table.shape == (nr, 4)
    np.testing.assert_allclose(table[:, 0], radii, rtol=1e-8)               # (the table holds nine digits)
    for i in range(nr):
        s = rm.reduce_return_map(res["maps"][i], res["records"][i])["scalars"]
        np.testing.assert_allclose(table[i, 1:], [s[2] / s[0], s[1] / s[0], s[3] / s[0]], rtol=1e-6)
    by_name = {h["name"]: h for h in hdus}
    assert [h["name"] for h in hdus] == ["PRIMARY", "COUNT", "FRACTION", "ENSHIFT", "EMIS", "DELAY"]
    head = by_name["PRIMARY"]["header"]
    head = {k: float(head[k]) for k in ("SPIN", "RMIN", "DR", "LOGBIN", "NR", "GAMMA", "PLANEISO", "LIMB", "WGTNORM")}      # (cards are read as text)
    assert head["SPIN"] == gc.SPIN and head["LOGBIN"] == 1 and head["GAMMA"] == 2 and head["NR"] == nr
    assert (head["PLANEISO"], head["LIMB"], head["WGTNORM"]) == (1, 0, 1)
    assert abs(head["RMIN"] - r_min) <= 1e-12 * r_min and abs(head["DR"] - dr) <= 1e-12 * dr
    empty = res["count"] == 0
    assert not empty.all()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = {"COUNT": res["count"], "FRACTION": res["weight"] / res["ray_count"][:, None], "ENSHIFT": res["flux"] / res["weight"],
                "EMIS": res["emis"] / res["ray_count"][:, None], "DELAY": res["time"] / res["weight"]}
    for name, plane in want.items():
        got = np.asarray(by_name[name]["data"], dtype=np.float64).T          # fits_lite gives [j_land][i_src]: the file holds data[i_src][j_land] like Array2D
        if name == "COUNT":
            assert np.array_equal(got, plane)
            continue
        assert np.array_equal(np.isnan(got), empty), name
        np.testing.assert_allclose(got[~empty], plane[~empty], rtol=1e-12, atol=0, err_msg=name)
