"""CPU: what the C entry points answer to bad arguments -- return code and the full kr_last_error() text -- against the table
tests/golden/capi_errors.json.  Rows recorded as KR_EINVAL are asserted everywhere: validation comes before any device work.  Every other
row (valid arguments with dummy pointers, errors that are only found after require_device()) was recorded without a GPU, where it ends in
KR_ENODEVICE; with a device visible such a call would run real kernels on dummy pointers, so those rows are then not executed at all.

The table is recorded by running this file (python tests/test_capi_errors.py --record) on a machine without a GPU; the tests never write it."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from raytrace_cpu_amd import capi  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "capi_errors.json")
SENTINEL = "kr_stream_create: null argument"      # set before every call: a row that fails without a message of its own records this

# every entry point of kr_capi.hip that checks a pointer, a count, bins or a spec before it does anything else
NULL_CHECKED = """kr_pointsource_tables kr_trace_async_f64 kr_trace_async_f32 kr_trace_wait_many kr_trace_f64 kr_trace_f32 kr_trace_progress_f64
kr_trace_progress_f32 kr_redshift_start_f64 kr_redshift_f64 kr_redshift_dest_f64 kr_range_phi_f64 kr_calculate_momentum_f64 kr_redshift_start_f32
kr_redshift_f32 kr_redshift_dest_f32 kr_range_phi_f32 kr_calculate_momentum_f32 kr_pointsource_init_dev_f64 kr_pointsource_init_f64
kr_imageplane_init_dev_f64 kr_imageplane_init_f64 kr_pointsource_init_strided_dev_f64 kr_imageplane_init_strided_dev_f64
kr_pointsource_init_emit_dev_f64 kr_pointsource_init_emit_batch_dev_f64 kr_post_emissivity_dev_f64 kr_imageplane_init_emit_dev_f64
kr_imageplane_init_emit_runs_dev_f64 kr_post_image_dev_f64 kr_reduce_emissivity_dev_f64 kr_reduce_emissivity_f64 kr_reduce_image_dev_f64
kr_reduce_image_f64 kr_reduce_line_dev_f64 kr_post_line_dev_f64 kr_line_from_image_dev_f64 kr_reduce_line_f64 kr_bundles_init_emit_dev_f64
kr_post_caustic_disc_dev_f64 kr_caustic_suppress_dev_f64 kr_reduce_return_dev_f64 kr_post_return_dev_f64 kr_post_return_batch_dev_f64
kr_reduce_return_f64 kr_debug_arith_f64 kr_host_attach kr_malloc kr_host_alloc kr_stream_create""".split()


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        from raytrace_cpu_amd import _build
        _build.build()
    return capi.load()


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)
    return obj


def build_cases():
    """[(symbol, case, args)]; the objects the arguments point to are kept alive by the returned list."""
    nan = float("nan")
    rays = np.zeros(4, dtype=capi.RAY_F64)
    rays32 = np.zeros(4, dtype=capi.RAY_F32)
    h, h32 = rays.ctypes.data_as(C.c_void_p), rays32.ctypes.data_as(C.c_void_p)
    buf = np.zeros(4096)
    out = buf.ctypes.data_as(C.c_void_p)
    dummy = C.c_void_p(16)            # a "device pointer": never dereferenced on a machine without a device
    stats = capi.Stats()
    p = C.byref(capi.default_params(0.998))
    keep = [rays, rays32, buf, stats]

    def ps_spec(**kw):
        s = capi.PointSourceSpec()
        s.pos[0], s.pos[1], s.pos[2], s.pos[3] = 0.0, 5.0, 1e-3, 0.0
        _set(s, V=0.0, spin=0.998, tol=0.0, dcosalpha=0.05, dbeta=0.05, cosalpha0=-0.995, cosalphamax=0.995, beta0=-math.pi, betamax=math.pi, E=1.0)
        return _set(s, **kw)

    def ip_spec(**kw):
        s = capi.ImagePlaneSpec()
        _set(s, dist=10000.0, inc_deg=80.0, x0=-30.0, xmax=30.0, dx=3.75, y0=-30.0, ymax=30.0, dy=3.75, spin=0.998, phi0=0.0, precision=100.0)
        return _set(s, **kw)

    def emis(**kw):
        return _set(_set(capi.EmisBins(), r_min=1.2, dr=1.1, r_isco=1.237, gamma=2.0, spin=0.998, num_primary_rays=1e6, nr=10, logbin=1), **kw)

    def img(**kw):
        b = _set(capi.ImageBins(), x0=-30.0, y0=-30.0, img_dx=15.0, img_dy=15.0, r_isco=1.237, r_disc=100.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0,
                 img_nx=4, img_ny=4)
        return _set(b, **kw)

    def ret():
        return _set(capi.ReturnBins(), r_isco=1.237, r_disc=400.0, r_esc=900.0, source_r=5.0, source_phi=0.0, plane_iso=1, limb=0, weight_norm=0)

    def line(**kw):
        return _set(capi.line_bins(e_min=1.0, de=0.1, ne=20, r_isco=1.237, r_disc=30.0), **kw)

    def cmap(**kw):
        return _set(_set(capi.CausticMap(), r_isco=1.237, r_disc=100.0, eps_x=0.1, eps_y=0.1, nx=4, ny=4, bundles=1), **kw)

    cases = []

    def add(symbol, case, *args):
        keep.append(args)
        cases.append((symbol, case, args))

    def ref(x):
        keep.append(x)
        return C.byref(x)

    PS, IP = ref(ps_spec()), ref(ip_spec())        # 5167 rays (40 x 126), 289 rays (17 x 17)

    # ---- trace: only the checks of kr_capi.hip itself (the launch path behind them belongs to kr_trace.hip)
    add("kr_pointsource_tables", "null_spec", None, out, out, out)
    for t in ("f64", "f32"):
        add(f"kr_trace_async_{t}", "null_ticket", p, dummy, 4, None, None)
    add("kr_trace_wait_many", "negative_count", -1, None, None, None)
    add("kr_trace_wait_many", "null_tickets", 2, None, None, None)
    for t, hr in (("f64", h), ("f32", h32)):
        add(f"kr_trace_{t}", "null_params", None, hr, 4, None)
        add(f"kr_trace_{t}", "null_rays", p, None, 4, C.byref(stats))
        add(f"kr_trace_{t}", "negative_n", p, hr, -1, None)
        add(f"kr_trace_{t}", "valid", p, hr, 4, C.byref(stats))
        add(f"kr_trace_{t}", "valid_n0", p, None, 0, None)
        cb = capi.PROGRESS_FN(0)
        add(f"kr_trace_progress_{t}", "null_params", None, hr, 4, None, 2, cb, None)
        add(f"kr_trace_progress_{t}", "null_rays", p, None, 4, None, 2, cb, None)
        add(f"kr_trace_progress_{t}", "negative_n", p, hr, -3, None, 2, cb, None)
        add(f"kr_trace_progress_{t}", "valid", p, hr, 4, None, 2, cb, None)

    # ---- the five O(N) passes, f64 / f32, device / host
    passes = {"redshift_start": (0.998, -1.0, 0, 0), "redshift": (0.998, -1.0, 0, 0, 0), "redshift_dest": (0.998, 1), "range_phi": (-math.pi, math.pi),
              "calculate_momentum": (0.998,)}
    for name, scalars in passes.items():
        for t, hr in (("f64", h), ("f32", h32)):
            add(f"kr_{name}_dev_{t}", "valid", *scalars, dummy, 4, None)
            add(f"kr_{name}_dev_{t}", "null_rays", *scalars, None, 4, None)
            add(f"kr_{name}_{t}", "null_rays", *scalars, None, 4)
            add(f"kr_{name}_{t}", "negative_n", *scalars, hr, -1)
            add(f"kr_{name}_{t}", "valid", *scalars, hr, 4)
            add(f"kr_{name}_{t}", "valid_n0", *scalars, None, 0)

    # ---- sources
    for kind, S in (("pointsource", PS), ("imageplane", IP)):
        add(f"kr_{kind}_init_dev_f64", "null_spec", None, dummy, 6000, None)
        add(f"kr_{kind}_init_dev_f64", "n_too_small", S, dummy, 8, None)
        add(f"kr_{kind}_init_dev_f64", "valid", S, dummy, 6000, None)
        add(f"kr_{kind}_init_f64", "null_spec", None, h, 4)
        add(f"kr_{kind}_init_f64", "null_rays", S, None, 4)
        add(f"kr_{kind}_init_f64", "negative_n", S, h, -1)
        add(f"kr_{kind}_init_f64", "n_too_small", S, h, 4)
        add(f"kr_{kind}_init_strided_dev_f64", "null_spec", None, 0, 1, dummy, 4, None)
        add(f"kr_{kind}_init_strided_dev_f64", "bad_stride", S, 0, 0, dummy, 4, None)
        add(f"kr_{kind}_init_strided_dev_f64", "negative_first", S, -1, 2, dummy, 4, None)
        add(f"kr_{kind}_init_strided_dev_f64", "valid", S, 1, 2, dummy, 4, None)
        add(f"kr_{kind}_init_emit_dev_f64", "null_spec", None, 0, 1, -1.0, 0, 0, dummy, 4, None)
        add(f"kr_{kind}_init_emit_dev_f64", "bad_stride", S, 0, 0, -1.0, 0, 0, dummy, 4, None)
        add(f"kr_{kind}_init_emit_dev_f64", "valid", S, 0, 1, -1.0, 0, 0, dummy, 4, None)
    add("kr_imageplane_init_emit_runs_dev_f64", "null_spec", None, 0, 4, 2, 0.0, 1, 0, dummy, 4, None)
    add("kr_imageplane_init_emit_runs_dev_f64", "run_above_stride", IP, 0, 2, 4, 0.0, 1, 0, dummy, 4, None)
    add("kr_imageplane_init_emit_runs_dev_f64", "valid", IP, 0, 4, 2, 0.0, 1, 0, dummy, 4, None)

    specs = (capi.PointSourceSpec * 2)(ps_spec(), ps_spec())
    ptrs = (C.c_void_p * 2)(16, 32)
    ptrs_hole = (C.c_void_p * 2)(16, None)
    counts = (C.c_int64 * 2)(4, 4)
    counts_zero = (C.c_int64 * 2)(4, 0)
    keep += [specs, ptrs, ptrs_hole, counts, counts_zero]
    B = "kr_pointsource_init_emit_batch_dev_f64"
    add(B, "negative_count", -1, specs, None, 0, 0, ptrs, counts, None)
    add(B, "null_specs", 2, None, None, 0, 0, ptrs, counts, None)
    add(B, "null_buffers", 2, specs, None, 0, 0, None, counts, None)
    add(B, "null_counts", 2, specs, None, 0, 0, ptrs, None, None)
    add(B, "null_ray_buffer", 2, specs, None, 0, 0, ptrs_hole, counts, None)
    add(B, "null_buffer_of_empty_item", 2, specs, None, 0, 0, ptrs_hole, counts_zero, None)
    add(B, "valid", 2, specs, None, 0, 0, ptrs, counts, None)
    add(B, "valid_count0", 0, None, None, 0, 0, None, None, None)

    # ---- fused epilogues and reducers
    post = (0.998, -1.0, 0, 0, 0, -math.pi, math.pi)
    E, E0, I, I0 = ref(emis()), ref(emis(nr=0)), ref(img()), ref(img(img_nx=0))
    for sym, bins, bad, lead in (("kr_post_emissivity_dev_f64", E, E0, post), ("kr_post_image_dev_f64", I, I0, post),
                                 ("kr_reduce_emissivity_dev_f64", E, E0, ()), ("kr_reduce_image_dev_f64", I, I0, ())):
        add(sym, "null_bins", *lead, None, dummy, 4, dummy, None)
        add(sym, "null_output", *lead, bins, dummy, 4, None, None)
        add(sym, "bad_size", *lead, bad, dummy, 4, dummy, None)
        add(sym, "valid", *lead, bins, dummy, 4, dummy, None)
    dc = C.c_int64()
    keep.append(dc)
    emis_out = [out] * 5
    add("kr_reduce_emissivity_f64", "null_bins", None, h, 4, *emis_out, C.byref(dc))
    for k in range(5):
        add("kr_reduce_emissivity_f64", f"null_output_{k}", E, h, 4, *[None if j == k else out for j in range(5)], None)
    add("kr_reduce_emissivity_f64", "nr0", E0, h, 4, *emis_out, None)
    add("kr_reduce_emissivity_f64", "null_rays", E, None, 4, *emis_out, None)
    add("kr_reduce_emissivity_f64", "negative_n", E, h, -1, *emis_out, None)
    add("kr_reduce_emissivity_f64", "valid", E, h, 4, *emis_out, C.byref(dc))
    img_out = [out] * 7
    add("kr_reduce_image_f64", "null_bins", None, h, 4, *img_out, None)
    for k in range(7):
        add("kr_reduce_image_f64", f"null_output_{k}", I, h, 4, *[None if j == k else out for j in range(7)], None)
    add("kr_reduce_image_f64", "nx0", I0, h, 4, *img_out, None)
    add("kr_reduce_image_f64", "ny_negative", ref(img(img_ny=-2)), h, 4, *img_out, None)
    add("kr_reduce_image_f64", "null_rays", I, None, 4, *img_out, None)
    add("kr_reduce_image_f64", "valid", I, h, 4, *img_out, C.byref(dc))

    R = ref(ret())
    out4 = (C.c_double * 4)()
    keep.append(out4)
    for sym, lead in (("kr_reduce_return_dev_f64", ()), ("kr_post_return_dev_f64", (-math.pi, math.pi))):
        add(sym, "null_bins", *lead, None, dummy, 4, dummy, None)
        add(sym, "null_output", *lead, R, dummy, 4, None, None)
        add(sym, "valid", *lead, R, dummy, 4, dummy, None)
    add("kr_reduce_return_f64", "null_bins", None, h, 4, C.byref(out4))
    add("kr_reduce_return_f64", "null_output", R, h, 4, None)
    add("kr_reduce_return_f64", "null_rays", R, None, 4, C.byref(out4))
    add("kr_reduce_return_f64", "negative_n", R, h, -1, C.byref(out4))
    add("kr_reduce_return_f64", "valid", R, h, 4, C.byref(out4))
    rb = (capi.ReturnBins * 2)(ret(), ret())
    keep.append(rb)
    B = "kr_post_return_batch_dev_f64"
    add(B, "negative_count", -2, 0.0, 1.0, rb, ptrs, counts, ptrs, None)
    add(B, "null_bins", 2, 0.0, 1.0, None, ptrs, counts, ptrs, None)
    add(B, "null_buffers", 2, 0.0, 1.0, rb, None, counts, ptrs, None)
    add(B, "null_counts", 2, 0.0, 1.0, rb, ptrs, None, ptrs, None)
    add(B, "null_outputs", 2, 0.0, 1.0, rb, ptrs, counts, None, None)
    add(B, "null_ray_buffer", 2, 0.0, 1.0, rb, ptrs_hole, counts, ptrs, None)
    add(B, "null_output_buffer", 2, 0.0, 1.0, rb, ptrs, counts, ptrs_hole, None)
    add(B, "null_buffer_of_empty_item", 2, 0.0, 1.0, rb, ptrs_hole, counts_zero, ptrs_hole, None)
    add(B, "valid", 2, 0.0, 1.0, rb, ptrs, counts, ptrs, None)

    # ---- emission line: the bins first, then the pointers, then the device
    L = ref(line())
    bad_lines = {"null_bins": None, "ne0": ref(line(ne=0)), "nan_emin": ref(line(e_min=nan)), "log_de1": ref(line(log_e=1, de=1.0)),
                 "nt2_dt0": ref(line(nt=2, dt=0.0)), "too_many_bins": ref(line(ne=4097, nt=4097, dt=1.0))}
    for case, b in bad_lines.items():
        add("kr_reduce_line_dev_f64", case, b, dummy, 4, dummy, None)
        add("kr_post_line_dev_f64", case, *post, b, dummy, 4, dummy, None)
        add("kr_line_from_image_dev_f64", case, b, I, dummy, dummy, None)
        add("kr_reduce_line_f64", case, b, h, 4, out)
    add("kr_reduce_line_dev_f64", "null_output", L, dummy, 4, None, None)
    add("kr_reduce_line_dev_f64", "null_rays", L, None, 4, dummy, None)
    add("kr_reduce_line_dev_f64", "bad_bins_and_null_output", bad_lines["ne0"], dummy, 4, None, None)
    add("kr_reduce_line_dev_f64", "valid", L, dummy, 4, dummy, None)
    add("kr_reduce_line_dev_f64", "valid_n0_null_rays", L, None, 0, dummy, None)
    add("kr_post_line_dev_f64", "null_output", *post, L, dummy, 4, None, None)
    add("kr_post_line_dev_f64", "null_rays", *post, L, None, 4, dummy, None)
    add("kr_post_line_dev_f64", "valid", *post, L, dummy, 4, dummy, None)
    add("kr_line_from_image_dev_f64", "null_image_bins", L, None, dummy, dummy, None)
    add("kr_line_from_image_dev_f64", "null_planes", L, I, None, dummy, None)
    add("kr_line_from_image_dev_f64", "null_output", L, I, dummy, None, None)
    add("kr_line_from_image_dev_f64", "nx0", L, I0, dummy, dummy, None)
    add("kr_line_from_image_dev_f64", "valid", L, I, dummy, dummy, None)
    add("kr_reduce_line_f64", "null_output", L, h, 4, None)
    add("kr_reduce_line_f64", "null_rays", L, None, 4, out)
    add("kr_reduce_line_f64", "negative_n", L, h, -1, out)
    add("kr_reduce_line_f64", "valid", L, h, 4, out)

    # ---- critical-curve maps
    Bn = "kr_bundles_init_emit_dev_f64"
    add(Bn, "null_spec", None, 0.1, 0.0, 1, 0, dummy, 1445, None)
    add(Bn, "eps_half", IP, 0.5, 0.0, 1, 0, dummy, 1445, None)
    add(Bn, "eps_zero", IP, 0.0, 0.0, 1, 0, dummy, 1445, None)
    add(Bn, "eps_nan", IP, nan, 0.0, 1, 0, dummy, 1445, None)
    add(Bn, "empty_grid", ref(ip_spec(xmax=-60.0)), 0.1, 0.0, 1, 0, dummy, 1445, None)
    add(Bn, "n_too_small", IP, 0.1, 0.0, 1, 0, dummy, 1444, None)
    add(Bn, "null_rays", IP, 0.1, 0.0, 1, 0, None, 1445, None)
    add(Bn, "valid", IP, 0.1, 0.0, 1, 0, dummy, 1445, None)
    M, MG = ref(cmap()), ref(cmap(bundles=0))
    bad_maps = {"null_map": None, "nx0": ref(cmap(nx=0)), "eps_zero": ref(cmap(eps_x=0.0)), "eps_inf": ref(cmap(eps_y=float("inf"))),
                "nan_r_isco": ref(cmap(r_isco=nan))}
    for case, m in bad_maps.items():
        add("kr_post_caustic_disc_dev_f64", case, -0.998, 1, m, dummy, 80, dummy, None)
        add("kr_caustic_suppress_dev_f64", case, m, dummy, None)
    add("kr_post_caustic_disc_dev_f64", "n_too_small_bundles", -0.998, 1, M, dummy, 79, dummy, None)
    add("kr_post_caustic_disc_dev_f64", "n_too_small_grid", -0.998, 1, MG, dummy, 15, dummy, None)
    add("kr_post_caustic_disc_dev_f64", "null_rays", -0.998, 1, M, None, 80, dummy, None)
    add("kr_post_caustic_disc_dev_f64", "null_maps", -0.998, 1, M, dummy, 80, None, None)
    add("kr_post_caustic_disc_dev_f64", "valid_bundles", -0.998, 1, M, dummy, 80, dummy, None)
    add("kr_post_caustic_disc_dev_f64", "valid_grid", -0.998, 1, MG, dummy, 16, dummy, None)
    add("kr_caustic_suppress_dev_f64", "null_maps", M, None, None)
    add("kr_caustic_suppress_dev_f64", "valid", M, dummy, None)

    # ---- diagnostics, attached arrays, memory helpers
    add("kr_debug_arith_f64", "null_a", 0, None, out, out, 4)
    add("kr_debug_arith_f64", "null_b", 0, out, None, out, 4)
    add("kr_debug_arith_f64", "null_out", 0, out, out, None, 4)
    add("kr_debug_arith_f64", "negative_n", 0, out, out, out, -1)
    add("kr_debug_arith_f64", "valid", 0, out, out, out, 4)
    add("kr_debug_arith_f64", "valid_n0", 0, out, out, out, 0)
    add("kr_host_attach", "null_rays", None, 4, 144)
    add("kr_host_attach", "n0", h, 0, 144)
    add("kr_host_attach", "bad_ray_bytes", h, 4, 100)
    add("kr_host_attach", "valid_f64", h, 4, 144)
    add("kr_host_attach", "valid_f32", h32, 4, 84)
    vp = C.c_void_p()
    keep.append(vp)
    for sym in ("kr_malloc", "kr_host_alloc"):
        add(sym, "null_pointer", None, 64)
        add(sym, "negative_bytes", C.byref(vp), -1)
        add(sym, "valid", C.byref(vp), 64)
    add("kr_stream_create", "null_pointer", None)
    add("kr_stream_create", "valid", C.byref(vp))
    assert len({(s, c) for s, c, _ in cases}) == len(cases)
    return cases, keep


def run_case(lib, symbol, args):
    assert lib.kr_stream_create(None) == capi.KR_EINVAL and lib.kr_last_error().decode() == SENTINEL
    rc = getattr(lib, symbol)(*args)
    return rc, (lib.kr_last_error().decode() if rc != capi.KR_OK else "")


def load_table():
    with open(TABLE) as f:
        return {(r["symbol"], r["case"]): r for r in json.load(f)}


CASES, _KEEP = build_cases()
ROWS = load_table() if os.path.exists(TABLE) else {}
EINVAL_IDS = sorted(f"{s}:{c}" for (s, c), r in ROWS.items() if r["rc"] == capi.KR_EINVAL)


@pytest.fixture(scope="module")
def lib():
    return _lib()


def test_table_and_cases_agree():
    assert ROWS, "tests/golden/capi_errors.json is missing"
    assert set(ROWS) == {(s, c) for s, c, _ in CASES}
    for r in ROWS.values():
        assert r["rc"] != capi.KR_OK and r["error"] and (r["error"] != SENTINEL or r["symbol"] == "kr_stream_create"), r


def test_einval_rows_cover_every_null_checked_entry_point():
    covered = {s for (s, _), r in ROWS.items() if r["rc"] == capi.KR_EINVAL}
    assert sorted(set(NULL_CHECKED) - covered) == []
    for s in NULL_CHECKED:
        assert s in capi.PROTOTYPES, s
    assert len(EINVAL_IDS) >= 2 * len(NULL_CHECKED)


@pytest.mark.parametrize("row", EINVAL_IDS)
def test_bad_arguments_are_refused_before_any_device_work(lib, row):
    symbol, case = row.split(":")
    args = next(a for s, c, a in CASES if (s, c) == (symbol, case))
    want = ROWS[(symbol, case)]
    rc, msg = run_case(lib, symbol, args)
    assert (rc, msg) == (want["rc"], want["error"]), row


def test_rows_that_reach_the_device_check_answer_as_recorded(lib):
    """Rows recorded with another code than KR_EINVAL (all of them KR_ENODEVICE: recorded without a GPU).  With a device visible none of
    them is executed."""
    others = [(s, c, a) for s, c, a in CASES if ROWS[(s, c)]["rc"] != capi.KR_EINVAL]
    assert others and all(ROWS[(s, c)]["rc"] == capi.KR_ENODEVICE for s, c, _ in others)
    share = f"{len(others)} of {len(CASES)} rows ({100.0 * len(others) / len(CASES):.0f} %)"
    if lib.kr_device_count() > 0:
        print(f"capi_errors: a device is visible, {share} not executed (they would launch kernels on dummy pointers)")
        pytest.skip(f"a GPU is visible: {share} of tests/golden/capi_errors.json not executed")
    print(f"capi_errors: no device, {share} executed besides the KR_EINVAL rows")
    for s, c, a in others:
        want = ROWS[(s, c)]
        assert run_case(lib, s, a) == (want["rc"], want["error"]), (s, c)


if __name__ == "__main__":
    assert "--record" in sys.argv, "usage: python tests/test_capi_errors.py --record   (on a machine without a GPU)"
    lib_ = _lib()
    assert lib_.kr_device_count() <= 0, "record the table on a machine without a GPU"
    rows = []
    for s_, c_, a_ in CASES:
        rc_, msg_ = run_case(lib_, s_, a_)
        rows.append({"symbol": s_, "case": c_, "rc": rc_, "error": msg_})
    with open(TABLE, "w") as f_:
        f_.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows, {sum(r['rc'] == capi.KR_EINVAL for r in rows)} of them KR_EINVAL -> {TABLE}")
