"""GPU: the line, the continuum, the response and the per-record angles of rays that landed on the surface of a disc (kr_disc_surface;
kr_angles_surface_dev_f64, kr_post_/kr_reduce_line_surface_dev_f64, kr_post_/kr_reduce_spectrum_surface_dev_f64, kr_post_/kr_reduce_response_surface_dev_f64,
api.arrival_angles / line_profile / disc_spectrum / disc_response with surface=, the disc_slope key of kr_line_profile, kr_disc_spectrum and
kr_reverb_response) against the numpy rule of tests/surface_pass_rules.py, the surface image pass, the flat rules fed rho, and each other.

Records: the three reference-pinned sets of tests/golden/thick_disc/ (5168 records each: 20 tiles of 256 and a ragged one; spin 0.5, reverse 0) pushed to
the device, the first 100 records of one of them (less than a tile; none of them lands: every sum and tally stays 0), 100 records from its first landed
one on, and a 33 x 33 image plane traced on the device to the surface (0.1, 0) between the ISCO and 30 (stored spin -0.5, 75 degrees, RK4, reverse 1).

Bars: mu and chi per record within max(16 x noise, 1e-12), noise the rule's own float64-vs-longdouble difference on those records (the convention of
tests/test_gpu_angles.py and test_gpu_plunge.py); counts and tallies exact; line sums within parity.BIN_RTOL; the spectrum and the response within the
max(16 x noise, floor) of tests/test_gpu_disc_spectrum.py and test_gpu_reverb_response.py, whose comparisons run here on flat_equivalent() records.  The
worst margins go through parity.record_margin (a copy: profiles/surface_pass_parity.json)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import fits_lite
import line_rules as lr
import oracle_lib as ol
import parity
import spectrum_rules as sr
import surface_pass_rules as sp
import surface_rules as su
import test_gpu_disc_spectrum as ds
import test_gpu_reverb_response as rv
from raytrace_cpu_amd import api, capi
from raytrace_cpu_amd.devmem import DeviceScope

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPS = os.path.join(ROOT, "tests", "golden", "apps")
PI = math.pi
FLOOR = 1e-12
R_DISC = 30.0
SETS = ["rk4_s005_m1", "rk4_s01_m0", "rk4_thin", "first100", "tile100", "plane"]
LAWS = sorted(capi.LIMB_LAWS)
EMIS40 = np.linspace(2.0, 0.1, 40)
TIME40 = 3.0 + 9.0 * np.sqrt(np.arange(40) / 40.0)          # a source -> disc delay that grows outwards


def margin(name, worst, allowed, **extra):
    parity.record_margin("test_gpu_surface_passes", name, {"n_traced": 0, "n_bad": 0, "frac_bad": 0.0, "worst_ok": float(worst)}, allowed=float(allowed), **extra)
    print(f"{name}: worst {worst:.3e}, allowed {allowed:.3e} {extra}")
    assert worst <= allowed, (name, worst, allowed)


def r_isco():
    """The inner edge of every model here: the ISCO of a = 0.5 as the fixtures carry it (it is their r_in)."""
    return su.r_in()


# ---- records and the rule on them, once per session -------------------------------------------------------------------------------------------
def plane_spec():
    return ol.imageplane_spec(1000.0, 75.0, -16.0, 16.0, 1.0, -16.0, 16.0, 1.0, 0.5)


def plane_params():
    p = capi.default_params(-0.5)
    p.precision, p.integrator, p.theta_max, p.r_max, p.flags = 100.0, capi.RK4, PI / 2, 1100.0, capi.FLAG_HYBRID
    return api.thick_disc_params(p, api.lib().kr_kerr_isco(0.5, 1), R_DISC, 0.1, 0.0)


_SETS = {}


def record_set(name):
    """dict(rays, spin as the passes take it, reverse, surface, r_isco) of a name of SETS.  The plane's records come back from api.surface_image, whose
    pass rewrote only redshift and phi, which every pass under test computes again from the fields it left alone."""
    if name not in _SETS:
        if name == "plane":
            spec, p = plane_spec(), plane_params()
            edge = float(p.stop_params[0])
            b = api.default_image_bins(spec, capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=edge, r_disc=R_DISC))
            res = api.surface_image(spec, p, b, return_records=True)
            assert len(res["records"]) == 33 * 33
            _SETS[name] = dict(rays=np.ascontiguousarray(res["records"]), spin=-0.5, reverse=1, surface=(edge, R_DISC, 0.1, 0.0), r_isco=edge)
        else:
            run = {"first100": "rk4_s005_m1", "tile100": "rk4_s005_m1"}.get(name, name)
            rays = su.load_records(run)
            if name == "first100":
                rays = rays[:100]
            elif name == "tile100":
                first = int(np.flatnonzero(su.landed(rays))[0])
                rays = rays[first:first + 100]
            slope, scale, _ = su.RUNS[run]
            _SETS[name] = dict(rays=np.ascontiguousarray(rays), spin=su.SPIN, reverse=0, surface=(su.r_in(), su.R_OUT, slope, scale), r_isco=su.r_in())
    return _SETS[name]


_RULE = {}


def rule(name):
    """The float64 rule on a record set: frame, angles, bad-angle, the records as a fused pass leaves them, the surface filter to R_DISC and the noise
    of g, mu, chi."""
    if name not in _RULE:
        S = record_set(name)
        rays, spin, reverse = S["rays"], S["spin"], S["reverse"]
        f = sp.frame(rays, spin, reverse)
        an = sp.angles(rays, spin, reverse, S["surface"], f=f)
        rec = sp.records_after(rays, spin, reverse)
        on = sp.on_surface(rec, S["r_isco"], R_DISC)
        _RULE[name] = dict(f=f, an=an, bad=sp.bad_angle(f, an), rec=rec, on=on, noise=sp.noise(rays, spin, reverse, S["surface"]))
        print(f"{name}: {len(rays)} records, {int(on.sum())} landed between r_isco and {R_DISC}, {int((_RULE[name]['bad'] & on).sum())} of them bad-angle")
    return _RULE[name]


def bar(noise):
    return max(16 * float(noise), FLOOR)


def surface_ref(name):
    return capi.disc_surface(record_set(name)["surface"])


def image_pass_records(name):
    """rays[] after kr_post_image_surface_dev_f64: what every fused surface pass must leave, byte for byte."""
    S = record_set(name)
    L = api.lib()
    b = capi.ImageBins()
    b.x0, b.y0, b.img_dx, b.img_dy, b.r_isco, b.r_disc = -20.0, -20.0, 10.0, 10.0, S["r_isco"], R_DISC
    b.q1, b.rb1, b.q2, b.rb2, b.q3, b.img_nx, b.img_ny, b.flip_image, b.pad = 3.0, 4.0, 3.0, 10.0, 3.0, 4, 4, 1, 0
    with DeviceScope(L) as dev:
        d, h = dev.upload(S["rays"]), dev.zeros(api.image_words(b) * 8)
        capi.check(L, L.kr_post_image_surface_dev_f64(S["spin"], S["reverse"], -PI, PI, C.byref(b), d, len(S["rays"]), h, None), "kr_post_image_surface")
        capi.check(L, L.kr_synchronize(None), "sync")
        return dev.fetch(d, len(S["rays"]), S["rays"].dtype)


_AFTER = {}


def after_image_pass(name):
    if name not in _AFTER:
        _AFTER[name] = image_pass_records(name)
    return _AFTER[name]


def flat_of(name):
    """The device's own records after the image pass as the flat rules must see them, and the surface filter on them."""
    post = after_image_pass(name)
    return sp.flat_equivalent(post), sp.on_surface(post, record_set(name)["r_isco"], R_DISC)


@pytest.mark.parametrize("name", SETS)
def test_redshift_and_phi_of_the_fused_passes(krlib, name):
    """What kr_post_image_surface_dev_f64 leaves -- the bytes every fused pass below must leave -- against the rule: the redshift within the bar, phi
    wrapped, nothing else touched, and the same records landed."""
    S, R = record_set(name), rule(name)
    post = after_image_pass(name)
    for f in post.dtype.names:
        if f not in ("redshift", "phi"):
            assert post[f].tobytes() == S["rays"][f].tobytes(), f
    assert np.array_equal(post["phi"], R["rec"]["phi"], equal_nan=True)
    on = sp.on_surface(post, S["r_isco"], R_DISC)
    assert np.array_equal(on, R["on"]) and int(on.sum()) == landed_count(name)
    if on.any():
        worst = float((np.abs(post["redshift"] - R["rec"]["redshift"])[on] / np.abs(R["rec"]["redshift"][on])).max())
        margin(f"redshift/{name}", worst, bar(R["noise"]["g"][on].max()), records=int(on.sum()), noise=float(R["noise"]["g"][on].max()))


def run_pass(name, call, nw, fused, rays=None, calls=1):
    """call(L, surface ref, d_rays, n, d_out) `calls` times into nw zeroed words, each on a fresh device copy of the records: (words, records after)."""
    L = api.lib()
    S = record_set(name)
    rays = S["rays"] if rays is None else rays
    sf = surface_ref(name)
    with DeviceScope(L) as dev:
        h = dev.zeros(nw * 8)
        after = rays
        for _ in range(calls):
            with DeviceScope(L) as one:
                d = one.upload(rays)
                capi.check(L, call(L, C.byref(sf), d, len(rays), h), "surface pass")
                capi.check(L, L.kr_synchronize(None), "sync")
                after = one.fetch(d, len(rays), rays.dtype)
        return dev.fetch(h, nw), after


def landed_count(name):
    """DEST records with r_isco <= rho < R_DISC, counted from the records."""
    S = record_set(name)
    rho = sp.rho_of(S["rays"])
    with np.errstate(invalid="ignore"):
        return int((sp.dest(S["rays"]) & (rho >= S["r_isco"]) & (rho < R_DISC)).sum())


def test_the_traced_plane_lands_on_the_surface(krlib):
    R = rule("plane")
    S = record_set("plane")
    assert R["on"].sum() >= 1 and landed_count("plane") == int(R["on"].sum())
    z = R["an"]["z"][R["on"]]
    print(f"plane: landed {int(R['on'].sum())}, bad-angle {int((R['bad'] & R['on']).sum())}, above the plane {int((z > 0).sum())}, below {int((z < 0).sum())}")
    assert S["surface"][0] == krlib.kr_kerr_isco(0.5, 1)


# ---- 1. the angles, record by record -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_angles_per_record(krlib, name):
    S, R = record_set(name), rule(name)
    rays, n = S["rays"], len(S["rays"])
    L = api.lib()
    sf = surface_ref(name)
    with DeviceScope(L) as dev:
        d, a = dev.upload(rays), dev.upload(np.full(2 * n, 7.0))
        capi.check(L, L.kr_angles_surface_dev_f64(C.byref(sf), S["spin"], S["reverse"], d, n, a, None), "kr_angles_surface_dev")
        capi.check(L, L.kr_synchronize(None), "sync")
        out, after = dev.fetch(a, 2 * n), dev.fetch(d, n, rays.dtype)
    assert after.tobytes() == rays.tobytes()                                             # the call reads the records and never writes them
    mu, chi = out[0::2], out[1::2]
    dead = rays["steps"] <= 0
    assert np.isnan(mu[dead]).all() and np.isnan(chi[dead]).all()
    want_mu, want_chi = R["an"]["mu"], R["an"]["chi"]
    on = sp.dest(rays)                                                                   # every record that landed, whatever its radius
    assert np.isfinite(want_mu[on]).all() and np.isfinite(want_chi[on]).all() and np.isfinite(mu[on]).all() and np.isfinite(chi[on]).all()
    with np.errstate(invalid="ignore"):
        bad_dev = on & ((mu > 1) | (mu < 0))
    assert np.array_equal(bad_dev, R["bad"] & on)
    if on.any():
        margin(f"angles-mu/{name}", np.abs(mu - want_mu)[on].max(), bar(R["noise"]["mu"][on].max()), records=int(on.sum()), noise=float(R["noise"]["mu"][on].max()))
        margin(f"angles-chi/{name}", np.abs(chi - want_chi)[on].max(), bar(R["noise"]["chi"][on].max()), records=int(on.sum()), noise=float(R["noise"]["chi"][on].max()))
    rest = ~on & ~dead & np.isfinite(want_mu) & np.isfinite(want_chi) & np.isfinite(mu) & np.isfinite(chi)
    if rest.any():
        print(f"{name}: off the surface, {int(rest.sum())} records: |mu - rule| <= {np.abs(mu - want_mu)[rest].max():.2e}, |chi - rule| <= {np.abs(chi - want_chi)[rest].max():.2e}")
    # the host-array form and the api's two forms give the same bits
    h_mu, h_chi = api.arrival_angles(rays, S["spin"], reverse=S["reverse"], surface=S["surface"])
    with DeviceScope(L) as dev:
        d_mu, d_chi = api.arrival_angles((dev.upload(rays), n), S["spin"], reverse=S["reverse"], surface=sf)
    for got in (h_mu, d_mu):
        assert got.tobytes() == np.ascontiguousarray(mu).tobytes()
    for got in (h_chi, d_chi):
        assert got.tobytes() == np.ascontiguousarray(chi).tobytes()


def test_angles_of_no_records(krlib):
    L = api.lib()
    sf = surface_ref("rk4_thin")
    with DeviceScope(L) as dev:
        a = dev.upload(np.full(4, 7.0))
        capi.check(L, L.kr_angles_surface_dev_f64(C.byref(sf), 0.5, 0, None, 0, a, None), "kr_angles_surface_dev")
        capi.check(L, L.kr_angles_surface_dev_f64(C.byref(sf), 0.5, 0, None, 0, None, None), "kr_angles_surface_dev")
        assert (dev.fetch(a, 4) == 7.0).all()
    mu, chi = api.arrival_angles(np.zeros(0, dtype=capi.RAY_F64), 0.5, surface=(4.2, 30.0, 0.1, 0.0))
    assert len(mu) == 0 and len(chi) == 0


# ---- 2. the line -------------------------------------------------------------------------------------------------------------------------------
def line_bins(name, nt=1, table=False):
    """90 linear energy bins over every landed ray's g; nt = 8: time rows over the arrival times, a few rays outside."""
    S = record_set(name)
    t = rule(name)["rec"]["t"][rule(name)["on"]]
    t0 = float(np.floor(t.min())) - 0.37 if len(t) else 0.0
    dt = ((float(t.max()) - t0) / 8.3 if len(t) else 1.0) if nt > 1 else 0.0
    b = capi.line_bins(line_energy=6.4, e_min=3.0, de=0.083, ne=90, t0=t0 if nt > 1 else 0.0, dt=dt, nt=nt, r_isco=S["r_isco"], r_disc=R_DISC, q1=3.0, rb1=6.0, q2=2.5,
                       rb2=12.0, q3=3.0, g_index=3.0)
    if table:
        b.with_table(S["r_isco"], (R_DISC / S["r_isco"]) ** (1.0 / 40), EMIS40, TIME40)
    return b


def fused_line(name, b, law, calls=1):
    S = record_set(name)
    lw = capi.limb_law(law)
    nw = api.line_words(b) + 1
    words, after = run_pass(name, lambda L, s, d, n, h: L.kr_post_line_surface_dev_f64(s, S["spin"], S["reverse"], -PI, PI, C.byref(b), C.byref(lw), d, n, h, None), nw, True,
                            calls=calls)
    out = api.line_from_words(b, words[:-1])
    out["bad_angle"], out["words"] = int(words[-1]), words
    return out, after


def reduced_line(name, b, rec):
    nw = api.line_words(b) + 1
    words, after = run_pass(name, lambda L, s, d, n, h: L.kr_reduce_line_surface_dev_f64(s, C.byref(b), d, n, h, None), nw, False, rays=rec)
    out = api.line_from_words(b, words[:-1])
    out["bad_angle"], out["words"] = int(words[-1]), words
    return out, after


def check_line(label, got, want):
    assert (got["on_disc"], got["binned"], got["bad_angle"]) == (want["on_disc"], want["binned"], want["bad_angle"]), label
    assert np.array_equal(got["count"], want["count"]), label
    problems, m = lr.compare_line(got, want, rtol=parity.BIN_RTOL, slack=0, max_excluded=0)
    assert problems == [], (label, problems, m)
    nz = want["flux"] != 0
    worst = float((np.abs(got["flux"] - want["flux"])[nz] / np.abs(want["flux"][nz])).max()) if nz.any() else 0.0
    margin(f"line/{label}", worst, parity.BIN_RTOL, binned=int(got["binned"]))


@pytest.mark.parametrize("nt", [1, 8])
@pytest.mark.parametrize("name", SETS)
def test_line_against_the_rule(krlib, name, nt):
    S, R = record_set(name), rule(name)
    b = line_bins(name, nt=nt, table=nt == 8)
    post = after_image_pass(name)
    iso = None
    for law_name in LAWS:
        law_id, coeff = capi.LIMB_LAWS[law_name]
        got, after = fused_line(name, b, law_name)
        assert after.tobytes() == post.tobytes(), (name, law_name)                       # rays[] exactly as after kr_post_image_surface_dev_f64
        want = sp.line_rule(b, law_id, coeff, post, mu=R["an"]["mu"], bad=R["bad"])
        assert got["on_disc"] == landed_count(name), (name, law_name)
        check_line(f"{name}-nt{nt}-{law_name}", got, want)
        if law_id == 0:
            iso = got
    # the reduce form on the records the fused pass left equals the fused isotropic form
    red, after = reduced_line(name, b, post)
    assert after.tobytes() == post.tobytes()
    assert red["bad_angle"] == 0 and (red["on_disc"], red["binned"]) == (iso["on_disc"], iso["binned"]) and np.array_equal(red["count"], iso["count"])
    check_line(f"{name}-nt{nt}-reduce", red, sp.line_rule(b, 0, 0.0, post))
    problems, m = lr.compare_line(red, iso, rtol=parity.BIN_RTOL, slack=0, max_excluded=0)
    assert problems == [], (name, problems, m)
    if name in ("first100",):
        assert not iso["words"].any()
    elif name != "plane":
        assert iso["binned"] > 30
    twice, _ = fused_line(name, b, "laor", calls=2)                                      # the call adds
    once, _ = fused_line(name, b, "laor")
    assert np.array_equal(twice["words"][-3:], 2 * once["words"][-3:]) and np.array_equal(twice["count"], 2 * once["count"])
    assert np.allclose(twice["flux"], 2 * once["flux"], rtol=parity.BIN_RTOL, atol=0)


def test_line_beyond_the_lds(krlib):
    """ne nt above the kernel's LDS budget: the instance that adds into the global histogram, against the rule and the LDS instance's marginal."""
    name = "rk4_s01_m0"
    R = rule(name)
    post = after_image_pass(name)
    small, big = line_bins(name), line_bins(name)
    big.ne, big.de = 90 * 30, 0.083 / 30
    assert api.line_words(small) + 1 <= 4096 < api.line_words(big) + 1
    got, after = fused_line(name, big, "laor")
    assert after.tobytes() == post.tobytes()
    check_line("global-histogram", got, sp.line_rule(big, 1, 2.06, post, mu=R["an"]["mu"], bad=R["bad"]))
    ref, _ = fused_line(name, small, "laor")
    assert (got["on_disc"], got["binned"], got["bad_angle"]) == (ref["on_disc"], ref["binned"], ref["bad_angle"])
    red, _ = reduced_line(name, big, post)
    check_line("global-histogram-reduce", red, sp.line_rule(big, 0, 0.0, post))


# ---- 3. the continuum --------------------------------------------------------------------------------------------------------------------------
def kt_table(name, nr=60):
    edge = record_set(name)["r_isco"]
    dr = (R_DISC / edge) ** (1.0 / nr)
    return edge, dr, api.thermal_kt_table(0.5, edge, dr, nr, 10.0, 1e18)


def spectrum_model(name, kind, ne, tables=False):
    edge = record_set(name)["r_isco"]
    if kind == "thermal":
        r_min, dr, kt = kt_table(name)
        return capi.spectrum_model("thermal", 0.1, (12.0 / 0.1) ** (1.0 / ne) if ne % 2 else 11.9 / ne, ne, log_e=ne % 2 == 1, r_isco=edge, r_disc=R_DISC, f_col=1.7,
                                   table_r_min=r_min, table_dr=dr, table_kt=kt)
    s_de, S = ds.smooth_table(2, 600)
    extra = dict(table_emis=EMIS40, table_r_min=edge, table_dr=(R_DISC / edge) ** (1.0 / 40)) if tables else {}
    return capi.spectrum_model("table", 0.05, (40.0 / 0.05) ** (1.0 / ne) if ne % 2 else 39.95 / ne, ne, log_e=ne % 2 == 1, r_isco=edge, r_disc=R_DISC, q1=3.0, rb1=6.0, q2=2.5,
                               rb2=12.0, q3=3.0, s=S, s_e_min=0.01, s_de=s_de, **extra)


def fused_spectrum(name, m, law, calls=1):
    S = record_set(name)
    lw = capi.limb_law(law)
    return run_pass(name, lambda L, s, d, n, h: L.kr_post_spectrum_surface_dev_f64(s, S["spin"], S["reverse"], -PI, PI, C.byref(m), C.byref(lw), d, n, h, None),
                    api.spectrum_words(m), True, calls=calls)


def reduced_spectrum(name, m, rec):
    return run_pass(name, lambda L, s, d, n, h: L.kr_reduce_spectrum_surface_dev_f64(s, C.byref(m), d, n, h, None), api.spectrum_words(m), False, rays=rec)


@pytest.mark.parametrize("ne", [4, 257])
@pytest.mark.parametrize("kind", ["table", "thermal"])
@pytest.mark.parametrize("name", SETS)
def test_spectrum_against_the_rule(krlib, name, kind, ne):
    R = rule(name)
    m = spectrum_model(name, kind, ne, tables=ne == 257)
    post, (flat, on) = after_image_pass(name), flat_of(name)
    assert np.array_equal(sr.disc_filter(m, flat), on)
    floor = ds.shape_floor(m, flat)
    words, after = fused_spectrum(name, m, "laor")
    assert after.tobytes() == post.tobytes()                                             # rays[] exactly as after kr_post_image_surface_dev_f64
    assert int(words[-4]) == landed_count(name)
    ds.against_the_rule("test_surface_spectrum", f"{name}-{kind}-ne{ne}-fused-laor", m, words, flat, (1, 2.06), R["an"]["mu"], R["bad"], floor=floor)
    iso, after = fused_spectrum(name, m, "isotropic")
    assert after.tobytes() == post.tobytes()
    ds.against_the_rule("test_surface_spectrum", f"{name}-{kind}-ne{ne}-fused-isotropic", m, iso, flat, (0, 0.0), R["an"]["mu"], R["bad"], floor=floor)
    red, after = reduced_spectrum(name, m, post)
    assert after.tobytes() == post.tobytes()                                             # the reduce form only reads
    ds.against_the_rule("test_surface_spectrum", f"{name}-{kind}-ne{ne}-reduce", m, red, flat, floor=floor)
    assert np.array_equal(red[-4:-2], iso[-4:-2]) and np.array_equal(red[:-4] == 0, iso[:-4] == 0)
    if name == "first100":
        assert not words.any() and not red.any()
    host = api.spectrum_from_words(m, red)
    L = api.lib()
    out = np.zeros(api.spectrum_words(m))
    sf = surface_ref(name)
    capi.check(L, L.kr_reduce_spectrum_surface_f64(C.byref(sf), C.byref(m), post.ctypes.data_as(C.c_void_p), len(post), out.ctypes.data_as(C.c_void_p)), "kr_reduce_spectrum_surface")
    assert np.array_equal(out[-4:], red[-4:]) and sr.rel_diff(out[:-4], host["flux"]) <= 1e-12      # the host-record form: the same kernel


@pytest.mark.parametrize("kind", ["table", "thermal"])
def test_spectrum_limb_laws_and_additivity(krlib, kind):
    name = "rk4_s005_m1"
    R = rule(name)
    m = spectrum_model(name, kind, 65)
    flat, _ = flat_of(name)
    res = {}
    for law_name in LAWS:
        words, _ = fused_spectrum(name, m, law_name)
        ds.against_the_rule("test_surface_spectrum_laws", f"{kind}-{law_name}", m, words, flat, capi.LIMB_LAWS[law_name], R["an"]["mu"], R["bad"], floor=ds.shape_floor(m, flat))
        res[law_name] = words
    assert not np.array_equal(res["laor"][:-4], res["isotropic"][:-4]) and not np.array_equal(res["brightening"][:-4], res["isotropic"][:-4])
    twice, _ = fused_spectrum(name, m, "laor", calls=2)
    assert np.array_equal(twice[-4:], 2 * res["laor"][-4:]) and sr.rel_diff(twice[:-4], 2 * res["laor"][:-4]) <= parity.BIN_RTOL


# ---- 4. the response ---------------------------------------------------------------------------------------------------------------------------
def response_model(name, ne, nt, tables):
    """nt = 1: one row that holds every landed ray; nt = 8: rows over the arrival times (with the delay column when `tables`), a few rays outside."""
    R = rule(name)
    t = R["rec"]["t"][R["on"]]
    lo, hi = (float(t.min()), float(t.max())) if len(t) else (0.0, 1.0)
    t0 = math.floor(lo) - 0.37
    dt = (hi + 13.0 - t0) * 1.01 if nt == 1 else (hi + (7.0 if tables else 0.0) - t0) / (nt + 0.3)
    return capi.response_model(spectrum_model(name, "table", ne, tables=tables), t0, dt, nt, table_time=TIME40 if tables else None)


def fused_response(name, Rm, law):
    S = record_set(name)
    lw = capi.limb_law(law)
    return run_pass(name, lambda L, s, d, n, h: L.kr_post_response_surface_dev_f64(s, S["spin"], S["reverse"], -PI, PI, C.byref(Rm), C.byref(lw), d, n, h, None),
                    api.response_words(Rm), True)


def reduced_response(name, Rm, rec):
    return run_pass(name, lambda L, s, d, n, h: L.kr_reduce_response_surface_dev_f64(s, C.byref(Rm), d, n, h, None), api.response_words(Rm), False, rays=rec)


@pytest.mark.parametrize("ne", [4, 257])
@pytest.mark.parametrize("nt", [1, 8])
@pytest.mark.parametrize("name", SETS)
def test_response_against_the_rule(krlib, name, nt, ne):
    R = rule(name)
    tables = nt == 8
    Rm = response_model(name, ne, nt, tables)
    post, (flat, _) = after_image_pass(name), flat_of(name)
    words, after = fused_response(name, Rm, "laor")
    assert after.tobytes() == post.tobytes()                                             # rays[] exactly as after kr_post_image_surface_dev_f64
    assert int(words[-4]) == landed_count(name)
    lo = rv.against_the_rule("test_surface_response", f"{name}-nt{nt}-ne{ne}-fused-laor", Rm, words, flat, (1, 2.06), R["an"]["mu"], R["bad"])
    if nt == 1:
        assert lo["outside"] == 0
    elif name not in ("first100", "tile100", "plane"):
        assert len(set(lo["row"][lo["row"] >= 0])) >= nt - 1                          # the rows change all through the launch
    iso, after = fused_response(name, Rm, "isotropic")
    assert after.tobytes() == post.tobytes()
    rv.against_the_rule("test_surface_response", f"{name}-nt{nt}-ne{ne}-fused-isotropic", Rm, iso, flat, (0, 0.0), R["an"]["mu"], R["bad"])
    red, after = reduced_response(name, Rm, post)
    assert after.tobytes() == post.tobytes()
    rv.against_the_rule("test_surface_response", f"{name}-nt{nt}-ne{ne}-reduce", Rm, red, flat)
    assert np.array_equal(red[-4:-2], iso[-4:-2]) and red[-1] == iso[-1] and np.array_equal(red[:-4] == 0, iso[:-4] == 0)
    if name == "first100":
        assert not words.any() and not red.any()
    # the rows summed are the surface spectrum of the same model
    spec_words, _ = fused_spectrum(name, Rm.spec, "laor")
    got, want = api.response_from_words(Rm, words), api.spectrum_from_words(Rm.spec, spec_words)
    assert (got["on_disc"], got["used"], got["bad_angle"]) == (want["on_disc"], want["used"], want["bad_angle"])
    if got["outside"] == 0:
        worst = sr.rel_diff(got["resp"].sum(axis=0), want["flux"])
        margin(f"response-rows-sum-to-the-spectrum/{name}-nt{nt}-ne{ne}", worst, parity.BIN_RTOL)
    L = api.lib()
    out = np.zeros(api.response_words(Rm))
    sf = surface_ref(name)
    capi.check(L, L.kr_reduce_response_surface_f64(C.byref(sf), C.byref(Rm), post.ctypes.data_as(C.c_void_p), len(post), out.ctypes.data_as(C.c_void_p)), "kr_reduce_response_surface")
    assert np.array_equal(out[-4:], red[-4:]) and np.array_equal(out[:-4] == 0, red[:-4] == 0) and sr.rel_diff(out[:-4], red[:-4]) <= 1e-12


@pytest.mark.parametrize("tables", [False, True], ids=["powerlaw3", "emis+time"])
@pytest.mark.parametrize("name", ["rk4_s005_m1", "rk4_thin", "plane"])
def test_flat_table_response_equals_the_surface_line_per_time_row(krlib, name, tables):
    """S = 1 and one energy: resp[:, 0] is the surface line's flux plane (g_index = 3) summed over its energies, row by row."""
    S, R = record_set(name), rule(name)
    edge = S["r_isco"]
    t = R["rec"]["t"][R["on"]]
    t0 = math.floor(float(t.min())) - 0.37
    nt = 12
    dt = (float(t.max()) - t0) / (nt + 0.6)                                              # the latest rays fall outside
    b = capi.line_bins(line_energy=1.0, e_min=1e-3, de=1.2, ne=80, log_e=True, t0=t0, dt=dt, nt=nt, r_isco=edge, r_disc=R_DISC, q1=3.0, rb1=6.0, q2=2.5, rb2=12.0, q3=3.0,
                       g_index=3.0)
    kw = {}
    if tables:
        b.with_table(edge, (R_DISC / edge) ** (1.0 / 40), EMIS40, TIME40)
        kw = dict(table_emis=EMIS40, table_r_min=edge, table_dr=(R_DISC / edge) ** (1.0 / 40))
    line, post = fused_line(name, b, "isotropic")
    spec = capi.spectrum_model("table", 1.0, 0.5, 1, r_isco=edge, r_disc=R_DISC, q1=3.0, rb1=6.0, q2=2.5, rb2=12.0, q3=3.0, s=np.ones(64), s_e_min=1e-3, s_de=1.3, **kw)
    Rm = capi.response_model(spec, t0, dt, nt, table_time=TIME40 if tables else None)
    g = post["redshift"][flat_of(name)[1]]
    E = sr.energies(spec)[0]
    assert g.min() * E >= 1e-3 and g.max() * E <= sr.last_node(spec) and g.min() > 1e-3 and g.max() < 1e-3 * 1.2 ** 80      # every ray inside both energy ranges
    words, after = fused_response(name, Rm, "isotropic")
    assert after.tobytes() == post.tobytes()
    got = api.response_from_words(Rm, words)
    assert got["on_disc"] == line["on_disc"] == got["used"] >= 1 and line["binned"] == got["used"] - got["outside"]
    want = line["flux"].sum(axis=1)
    assert np.array_equal(want == 0, got["resp"][:, 0] == 0) and np.array_equal(line["count"].sum(axis=1) > 0, got["resp"][:, 0] != 0)
    worst = sr.rel_diff(got["resp"][:, 0], want)
    margin(f"flat-table-response-is-the-line/{name}-{'tables' if tables else 'powerlaw3'}", worst, parity.BIN_RTOL, used=int(got["used"]), outside=int(got["outside"]))


# ---- 5. api and programs -----------------------------------------------------------------------------------------------------------------------
def test_api_equals_the_c_abi_sequence(krlib):
    """api.line_profile / disc_spectrum / disc_response with surface= on the traced plane: the tallies of the rule on the records they return."""
    S, R = record_set("plane"), rule("plane")
    spec, p = plane_spec(), plane_params()
    b = line_bins("plane")
    line = api.line_profile(spec, p, b, limb="laor", surface=S["surface"])
    want = sp.line_rule(b, 1, 2.06, after_image_pass("plane"), mu=R["an"]["mu"], bad=R["bad"])
    check_line("api-plane-laor", line, want)
    assert line["surface"] == S["surface"] and line["stats"]["rays_traced"] > 0
    m = spectrum_model("plane", "table", 65)
    res = api.disc_spectrum(spec, p, m, limb="laor", surface=capi.disc_surface(S["surface"]), return_records=True)
    assert res["records"].tobytes() == after_image_pass("plane").tobytes()
    words = np.concatenate([res["flux"], [res["on_disc"], res["used"], res["bad_angle"], 0.0]])
    flat, _ = flat_of("plane")
    ds.against_the_rule("test_surface_api", "plane-spectrum", m, words, flat, (1, 2.06), R["an"]["mu"], R["bad"], floor=ds.shape_floor(m, flat))
    Rm = response_model("plane", 65, 8, True)
    resp = api.disc_response(spec, p, Rm, limb="laor", surface=S["surface"])
    words = np.concatenate([resp["resp"].ravel(), [resp["on_disc"], resp["used"], resp["bad_angle"], resp["outside"]]])
    rv.against_the_rule("test_surface_api", "plane-response", Rm, words, flat, (1, 2.06), R["an"]["mu"], R["bad"])
    flat = api.line_profile(spec, p, b, limb="laor")                                      # without surface=: the flat pass, which sees none of these rays as the rule does
    assert "surface" not in flat


def program(name):
    exe = os.path.join(ROOT, "raytrace_cpu_amd", "apps", "_build", name)
    assert os.path.exists(exe), f"{name} not built (__graft_entry__.build())"
    return exe


def run_program(name, par, out, extra=()):
    r = subprocess.run([program(name), f"--parfile={os.path.join(APPS, par)}", f"--outfile={out}", *extra], capture_output=True, text=True, timeout=300, cwd=APPS)
    return r


SURFACE_KEYS = ["--disc_slope=0.1"]


def program_surface(r_disc=30.0):
    """What the programs make of disc_slope = 0.1 in the fixtures' geometry (a = 0.998): the surface and the trace to it."""
    edge = api.lib().kr_kerr_isco(ds.SPIN, 1)
    return (edge, r_disc, 0.1, 0.0), api.thick_disc_params(ds.image_params(), edge, r_disc, 0.1, 0.0)


def test_line_profile_program(krlib, tmp_path):
    out, plain = tmp_path / "line.dat", tmp_path / "plain.dat"
    keys = ["--line_mode=rays", "--e_min=1", "--e_max=10", "--ne=90", "--limb=1"]
    r = run_program("kr_line_profile", "imageplane_rk4.par", out, keys + SURFACE_KEYS)
    assert r.returncode == 0, r.stdout + r.stderr
    surface, p = program_surface()
    b = capi.line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, r_isco=surface[0], r_disc=30.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0)
    d = 60.0 / 31
    spec = ol.imageplane_spec(10000.0, 80.0, -30.0, 30.0, d, -30.0, 30.0, d, ds.SPIN)
    want = api.line_profile(spec, p, b, limb=(1, 2.06), surface=surface)
    assert want["binned"] > 30
    text = open(out).read()
    assert text.splitlines()[0].split()[:2] == ["#", "DISCSLOP"] and text.splitlines()[2].split()[:2] == ["#", "DISCRIN"]
    assert text == api.line_text(want, b, limb=(1, 2.06))
    # without the keys: the file of the flat entry points, byte for byte
    r = run_program("kr_line_profile", "imageplane_rk4.par", plain, keys)
    assert r.returncode == 0, r.stdout + r.stderr
    flat = api.line_profile(spec, ds.image_params(), b, limb=(1, 2.06))
    assert open(plain).read() == api.line_text(flat, b, limb=(1, 2.06)) and "DISCSLOP" not in open(plain).read()
    assert not np.array_equal(flat["count"], want["count"])
    for bad, word in ((["--plunge=1"], "plunge"), (["--pol_law=1"], "pol_law"), (["--line_mode=pixels"], "line_mode")):
        extra = [k for k in keys if not (bad[0].startswith("--line_mode") and k.startswith("--line_mode")) and not (bad[0].startswith("--line_mode") and k == "--limb=1")]
        r = run_program("kr_line_profile", "imageplane_rk4.par", tmp_path / "x.dat", extra + SURFACE_KEYS + bad)
        assert r.returncode == 1 and word in r.stderr, (bad, r.stderr)


def test_disc_spectrum_program(krlib, tmp_path):
    out, plain = tmp_path / "spec.dat", tmp_path / "plain.dat"
    r = run_program("kr_disc_spectrum", "disc_spectrum_table.par", out, SURFACE_KEYS + ["--disc_scale=0.5"])
    assert r.returncode == 0, r.stdout + r.stderr
    edge = api.lib().kr_kerr_isco(ds.SPIN, 1)
    surface = (edge, 30.0, 0.1, 0.5)
    p = api.thick_disc_params(ds.image_params(), *surface)
    e, c = np.loadtxt(os.path.join(APPS, "powerlaw.spec"), unpack=True)
    s_e_min, s_de, S = api.resample_spectrum(e, c, 64)
    m = capi.spectrum_model("table", 0.5, math.exp(math.log(200 / 0.5) / 40), 40, log_e=True, r_isco=edge, r_disc=30.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0,
                            s=np.array([S, S]), s_e_min=s_e_min, s_de=s_de)
    want = api.disc_spectrum(ds.plane(80.0, 16), p, m, surface=surface)
    assert want["used"] > 30
    assert open(out).read() == api.spectrum_text(want)
    r = run_program("kr_disc_spectrum", "disc_spectrum_table.par", plain)
    assert r.returncode == 0, r.stdout + r.stderr
    flat = api.disc_spectrum(ds.plane(80.0, 16), ds.image_params(), m)
    assert open(plain).read() == api.spectrum_text(flat) and "DISCSLOP" not in open(plain).read()
    for bad, word in ((["--plunge=1"], "plunge"), (["--pol_law=1"], "pol_law")):
        r = run_program("kr_disc_spectrum", "disc_spectrum_table.par", tmp_path / "x.dat", SURFACE_KEYS + bad)
        assert r.returncode == 1 and word in r.stderr, (bad, r.stderr)


def test_reverb_response_program(krlib, tmp_path):
    out, plain = tmp_path / "resp.fits", tmp_path / "plain.fits"
    r = run_program("kr_reverb_response", "reverb_response.par", out, SURFACE_KEYS)
    assert r.returncode == 0, r.stdout + r.stderr
    surface, p = program_surface()
    e, c = np.loadtxt(os.path.join(APPS, "powerlaw.spec"), unpack=True)
    s_e_min, s_de, S = rv.program_rest_spectrum(e, c, 64)
    table = np.loadtxt(os.path.join(APPS, "emissivity.dat"))
    radius, emis, delay = table[:, 0], table[:, 4], table[:, 6]
    dr = float(np.exp(np.log(radius[-1] / radius[0]) / (len(radius) - 1)))
    spec = capi.spectrum_model("table", 0.5, math.exp(math.log(200 / 0.5) / 24), 24, log_e=True, r_isco=surface[0], r_disc=30.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0,
                               s=np.array([S, S]), s_e_min=s_e_min, s_de=s_de, table_emis=emis, table_r_min=float(radius[0]), table_dr=dr)
    Rm = capi.response_model(spec, 10000.0, 2.5, 32, table_time=delay)
    for path, params, kw in ((out, p, dict(surface=surface)), (plain, ds.image_params(), {})):
        if path is plain:
            r = run_program("kr_reverb_response", "reverb_response.par", plain)
            assert r.returncode == 0, r.stdout + r.stderr
        res = api.disc_response(ds.plane(80.0, 15), params, Rm, **kw)                     # 16 x 16 = 256 records: one tile, so every cell is summed in one order
        hdus = fits_lite.read(str(path))
        assert res["used"] > 30 and res["resp"].any()
        assert hdus[0]["data"].shape == (32, 24) and hdus[0]["data"].tobytes() == res["resp"].tobytes()
        assert hdus[1]["data"].tobytes() == res["energy"].tobytes() and hdus[2]["data"].tobytes() == res["time"].tobytes()
        head = hdus[0]["header"]
        assert (int(head["ON_DISC"]), int(head["USED"]), int(head["BADANGLE"]), int(head["OUTSIDE"])) == (res["on_disc"], res["used"], res["bad_angle"], res["outside"])
        if path is out:
            assert float(head["DISCSLOP"]) == 0.1 and float(head["DISCSCAL"]) == 0.0 and abs(float(head["DISCRIN"]) / surface[0] - 1) < 1e-14
        else:
            assert not any(k.startswith("DISC") for k in head)
    for bad, word in ((["--plunge=1"], "plunge"), (["--pol_law=1"], "pol_law")):
        r = run_program("kr_reverb_response", "reverb_response.par", tmp_path / "x.fits", SURFACE_KEYS + bad)
        assert r.returncode == 1 and word in r.stderr, (bad, r.stderr)
