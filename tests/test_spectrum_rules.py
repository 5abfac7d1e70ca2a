"""CPU: the continuum-spectrum rule (tests/spectrum_rules.py, the numpy restatement of kr_spectrum_model in include/kr_trace.h) held to identities
that need no device, and the Novikov-Thorne helpers of the api (api.novikov_thorne_flux, api.thermal_kt_table) held to the closed forms they implement.
The api's result layout and text form are checked here too."""
import numpy as np
import pytest

import spectrum_rules as sr
from raytrace_cpu_amd import api, capi


def circular_orbit_energy(r, a):
    """E-dagger of a prograde circular geodesic (Bardeen, Press & Teukolsky 1972)."""
    return (r ** 1.5 - 2 * r ** 0.5 + a) / (r ** 0.75 * np.sqrt(r ** 1.5 - 3 * r ** 0.5 + 2 * a))


# ---- Novikov-Thorne -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [0.0, 0.5, 0.9, 0.998])
def test_flux_vanishes_exactly_at_the_isco_and_is_nan_inside(spin):
    r_isco = api.isco_radius(spin)
    assert api.novikov_thorne_flux(r_isco, spin) == 0.0
    assert np.isnan(api.novikov_thorne_flux(0.999 * r_isco, spin))
    assert api.novikov_thorne_flux(1.5 * r_isco, spin) > 0
    assert api.novikov_thorne_flux(r_isco, spin, r_isco=r_isco) == 0.0


def test_isco_radius_is_the_double_precision_one():
    assert api.isco_radius(0.0) == 6.0
    assert abs(api.isco_radius(0.998) - 1.2369706551751847) < 1e-14
    assert abs(api.isco_radius(0.998) - api.lib().kr_kerr_isco(0.998, 1)) < 1e-6          # (the reference's keeps float intermediates)


def test_schwarzschild_flux_peaks_at_9_55():
    r = np.linspace(9.0, 10.0, 100001)
    peak = r[np.argmax(api.novikov_thorne_flux(r, 0.0))]
    print(f"a = 0: the flux peaks at r = {peak:.5f}")
    assert abs(peak - 9.55) <= 0.01


@pytest.mark.parametrize("spin,efficiency", [(0.0, 0.0571910), (0.5, 0.0821180), (0.998, 0.3209942)])
def test_luminosity_identity(spin, efficiency):
    """Both faces radiate what the accreting gas loses: the integral of 4 pi r^2 E-dagger F over ln r from r_isco to R equals 1 - E-dagger(r_isco) up to
    the Newtonian tail beyond R that is cut off, 3 / (2 R)."""
    r_isco = api.isco_radius(spin)
    R = 1e7 * r_isco
    u = np.linspace(np.log(r_isco), np.log(R), 2000001)
    r = np.exp(u)
    r[0] = r_isco
    f = 4 * np.pi * r * r * circular_orbit_energy(r, spin) * api.novikov_thorne_flux(r, spin)
    total = float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(u)))
    want = 1 - circular_orbit_energy(r_isco, spin)
    print(f"a = {spin}: integral {total:.10f}, 1 - E(r_isco) {want:.10f}, miss {abs(total - want):.2e}, bar {3 / (2 * R) + 1e-8:.2e}")
    assert abs(want - efficiency) < 5e-8
    assert abs(total - want) <= 3 / (2 * R) + 1e-8


def test_thermal_kt_table_peak_is_the_closed_form_of_the_maximum_flux():
    mass, mdot = 10.0, 1e18
    r_min, dr, nr = 6.0, 1.0005, 8000                     # bins 0.05 % wide: the centre nearest the maximum misses it by (2.5e-4)^2 in F at most
    kt = api.thermal_kt_table(0.0, r_min, dr, nr, mass, mdot, f_col=1.0)
    assert kt.shape == (nr,) and np.isfinite(kt).all() and (kt > 0).all()
    r = np.linspace(9.0, 10.0, 100001)
    f_max = api.novikov_thorne_flux(r, 0.0).max()
    want = api.K_B_KEV_PER_K * (f_max * mdot * api.C_CGS ** 6 / (api.G_CGS ** 2 * (mass * api.M_SUN_G) ** 2) / api.SIGMA_SB_CGS) ** 0.25
    print(f"10 Msun, 1e18 g/s: peak kT {kt.max():.6f} keV, closed form {want:.6f} keV")
    assert abs(kt.max() / want - 1) <= 1e-7
    centres = r_min * dr ** (np.arange(nr) + 0.5)
    assert abs(centres[np.argmax(kt)] - 9.55) <= 0.01
    inside = api.thermal_kt_table(0.0, 3.0, 1.1, 12, mass, mdot)                           # bins whose centre lies inside the ISCO: NaN
    c = 3.0 * 1.1 ** (np.arange(12) + 0.5)
    assert np.array_equal(np.isnan(inside), c < 6.0) and np.isnan(inside).any() and np.isfinite(inside).any()
    lin = api.thermal_kt_table(0.0, 6.0, 0.5, 10, mass, mdot, logbin=False)
    assert np.allclose(lin, api.K_B_KEV_PER_K * (api.novikov_thorne_flux(6.0 + 0.5 * (np.arange(10) + 0.5), 0.0) * mdot * api.C_CGS ** 6 /
                                                (api.G_CGS ** 2 * (mass * api.M_SUN_G) ** 2) / api.SIGMA_SB_CGS) ** 0.25, rtol=1e-14)
    with pytest.raises(api.KrError):
        api.thermal_kt_table(0.0, 6.0, 1.1, 4, mass, mdot, f_col=0.0)


# ---- the rule on synthetic records --------------------------------------------------------------------------------------------------
def thermal_model(kt, ne=40, e_min=0.05, de=0.1, log_e=False, f_col=1.7, **kw):
    return capi.spectrum_model("thermal", e_min, de, ne, log_e=log_e, r_isco=2.0, r_disc=100.0, f_col=f_col, table_r_min=2.0, table_dr=1.5, table_kt=kt, **kw)


def table_model(S, s_e_min=0.5, s_de=2.0, ne=30, e_min=1.0, de=0.1, log_e=False, **kw):
    return capi.spectrum_model("table", e_min, de, ne, log_e=log_e, r_isco=2.0, r_disc=100.0, s=S, s_e_min=s_e_min, s_de=s_de, **kw)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("log_e", [False, True])
def test_records_at_one_radius_with_g_1_give_n_planck_functions(dtype, log_e):
    kt = np.array([0.3, 0.5, 0.8, 1.1, 0.9, 0.6, 0.4, 0.2, 0.1, 0.05])
    m = thermal_model(kt, log_e=log_e, de=1.1 if log_e else 0.1)
    n = 37
    rays = sr.synthetic_records(np.full(n, 5.0), 1.0)                                       # log(5 / 2) / log(1.5) = 2.26: bin 2
    got = sr.spectrum(m, rays, dtype=dtype)
    E = sr.energies(m, np.float64)
    want = n * 1.7 ** -4 * E ** 3 / np.expm1(E / (1.7 * 0.8))
    assert (got["on_disc"], got["used"], got["bad_angle"]) == (n, n, 0)
    assert got["flux"].dtype == dtype and sr.rel_diff(got["flux"], want) <= 1e-13
    if log_e:
        assert np.allclose(E, 0.05 * np.sqrt(1.1) * 1.1 ** np.arange(40), rtol=1e-14)       # geometric centres
    else:
        assert np.allclose(E, 0.05 + 0.1 * (np.arange(40) + 0.5), rtol=1e-15)


def test_rays_outside_the_kt_table_or_with_a_bad_kt_are_counted_but_not_used():
    kt = np.array([0.3, np.nan, 0.0, -1.0, np.inf, 0.7])
    m = thermal_model(kt)
    r = 2.0 * 1.5 ** (np.arange(8) + 0.5)                                                    # bins 0 ... 7: two of them beyond the table
    got = sr.spectrum(m, sr.synthetic_records(r, 0.9))
    assert got["on_disc"] == 8 and got["used"] == 2 and list(got["used_index"]) == [0, 5]
    assert np.isfinite(got["flux"]).all() and (got["flux"] > 0).all()


def test_flat_table_gives_the_sum_of_emis_over_g_cubed():
    g = np.array([0.4, 0.7, 1.0, 1.3])
    r = np.array([3.2, 5.0, 9.0, 40.0])
    m = table_model(np.ones(8), s_e_min=0.5, s_de=2.0, ne=30, e_min=1.0, de=2.0)             # nodes 0.5 ... 64; E_i = 2, 4, ..., 60
    got = sr.spectrum(m, sr.synthetic_records(r, g))
    E = sr.energies(m)
    all_inside = (g.min() * E >= 0.5) & (g.max() * E <= 64.0)
    assert 5 < all_inside.sum() < m.ne
    import line_rules as lr
    want = np.sum(lr.powerlaw3(r, 3.0, 4.0, 3.0, 10.0, 3.0) * g ** -3.0)
    assert np.allclose(got["flux"][all_inside], want, rtol=1e-14)
    assert (got["flux"][~all_inside] < want * (1 - 1e-6)).all()                                # some ray has left the grid there
    # with an emissivity table instead of the power law
    emis = np.array([5.0, 4.0, np.nan, 2.0, 1.0, 0.5, 0.25, 0.125])
    mt = table_model(np.ones(8), ne=30, e_min=1.0, de=2.0, table_emis=emis, table_r_min=2.0, table_dr=1.5)
    got = sr.spectrum(mt, sr.synthetic_records(r, g))
    inside, ir = sr.table_index(mt, r)
    assert list(ir) == [1, 2, 3, 7] and inside.all()
    assert got["on_disc"] == 4 and got["used"] == 3 and list(got["used_index"]) == [0, 2, 3]      # bin 2 holds the NaN: the ray at r = 5 drops out
    keep = np.array([0, 2, 3])
    assert np.allclose(got["flux"][all_inside], np.sum(emis[ir[keep]] * g[keep] ** -3.0), rtol=1e-14)


def test_the_last_node_is_inside_and_one_ulp_above_it_is_not():
    S = np.array([1.0, 2.0, 4.0, 8.0, 16.0])                                                  # nodes 0.5, 1, 2, 4, 8
    m = table_model(S, s_e_min=0.5, s_de=2.0, ne=1, e_min=3.0, de=2.0)                        # E_0 = 4
    assert sr.last_node(m) == 8.0 and sr.energies(m)[0] == 4.0
    on = sr.spectrum(m, sr.synthetic_records([5.0], 2.0))                                     # g E = 8: the last node itself
    above = sr.spectrum(m, sr.synthetic_records([5.0], np.nextafter(2.0, 3.0)))
    below = sr.spectrum(m, sr.synthetic_records([5.0], np.nextafter(0.125, 0.0)))             # g E just under the first node
    first = sr.spectrum(m, sr.synthetic_records([5.0], 0.125))
    emis = 5.0 ** -3.0 * 4.0 ** 0                                                             # powerlaw3 at r = 5: rb1^(q2 - q1) r^-q2
    assert on["flux"][0] == pytest.approx(emis * 2.0 ** -3 * 16.0, rel=1e-14) and on["used"] == 1
    assert above["flux"][0] == 0.0 and above["used"] == 1
    assert below["flux"][0] == 0.0
    assert first["flux"][0] == pytest.approx(emis * 0.125 ** -3 * 1.0, rel=1e-14)
    mid = sr.spectrum(m, sr.synthetic_records([5.0], 2.0 ** -0.5))                            # half-way between the nodes 2 and 4 in log E
    assert mid["flux"][0] == pytest.approx(emis * 2.0 ** 1.5 * 6.0, rel=1e-13)


@pytest.mark.parametrize("nz", [1, 3, 7])
def test_zone_edges(nz):
    m = table_model(np.ones((nz, 4)))
    assert (m.nz, m.s_ne) == (nz, 4)
    z = sr.zone_of(m, np.array([2.0, np.nextafter(100.0, 0.0), 99.0, 2.0 * 50.0 ** (1 / nz) * 1.001]))
    assert z[0] == 0 and z[1] == nz - 1 and z[2] == nz - 1
    assert z[3] == min(1, nz - 1)
    # each zone's own spectrum is the one a ray in it sees
    S = np.arange(1, nz + 1, dtype=np.float64)[:, None] * np.ones((nz, 4))
    mz = table_model(S, ne=1, e_min=0.5, de=1.0)                                              # E_0 = 1: inside the grid 0.5 ... 4 at g = 1
    edges = 2.0 * 50.0 ** (np.arange(nz) / nz)
    for k in range(nz):
        r = edges[k] * 1.01
        got = sr.spectrum(mz, sr.synthetic_records([r], 1.0))
        import line_rules as lr
        assert got["flux"][0] == pytest.approx((k + 1) * float(lr.powerlaw3(r, 3.0, 4.0, 3.0, 10.0, 3.0)), rel=1e-14), k


def test_limb_law_and_bad_angles_in_the_rule():
    m = thermal_model(np.full(10, 0.5))
    rays = sr.synthetic_records(np.full(4, 5.0), 1.0)
    mu = np.array([0.2, 0.9, np.nan, 0.5])
    bad = np.array([False, False, True, False])
    iso = sr.spectrum(m, rays, law=0, mu=mu, bad=bad)
    laor = sr.spectrum(m, rays, law=1, coeff=2.06, mu=mu, bad=bad)
    assert (iso["used"], iso["bad_angle"], laor["used"], laor["bad_angle"]) == (4, 1, 3, 1)
    one = sr.spectrum(m, rays[:1])["flux"]
    assert np.allclose(iso["flux"], 4 * one, rtol=1e-14)
    assert np.allclose(laor["flux"], (3 + 2.06 * (0.2 + 0.9 + 0.5)) * one, rtol=1e-14)


def test_noise_is_a_few_ulp_times_the_exponent():
    m = thermal_model(np.full(10, 0.5), ne=64, e_min=0.1, de=1.0, f_col=1.0)
    rng = np.random.default_rng(5)
    rays = sr.synthetic_records(rng.uniform(3.0, 50.0, 300), rng.uniform(0.3, 1.4, 300))
    noise, lo, hi = sr.noise(m, rays)
    x_max = 1.4 * sr.energies(m)[-1] / 0.5
    print(f"noise {noise:.2e} at x up to {x_max:.0f}")
    assert 0 < noise <= 4 * 1.2e-16 * x_max


# ---- the api's layout and text ------------------------------------------------------------------------------------------------------
def test_words_layout_and_text():
    m = thermal_model(np.full(4, 0.5), ne=3, e_min=1.0, de=2.0)
    assert api.spectrum_words(m) == 7
    res = api.spectrum_from_words(m, np.array([1.5, 2.5, 0.0, 10.0, 8.0, 2.0, 0.0]))
    assert list(res["flux"]) == [1.5, 2.5, 0.0] and (res["on_disc"], res["used"], res["bad_angle"]) == (10, 8, 2)
    assert list(res["energy"]) == [2.0, 4.0, 6.0] and np.array_equal(res["energy"], sr.energies(m))
    text = api.spectrum_text(res)
    assert text.splitlines() == ["           # ON_DISC                  10", "              # USED                   8", "         # BAD_ANGLE                   2",
                                 "      2.00000000e+00      1.50000000e+00", "      4.00000000e+00      2.50000000e+00", "      6.00000000e+00      0.00000000e+00"]
    ml = thermal_model(np.full(4, 0.5), ne=5, e_min=0.5, de=2.0, log_e=True)
    assert np.array_equal(api.spectrum_energies(ml), sr.energies(ml))


def test_resample_spectrum_reproduces_a_power_law_in_log_energy():
    e = np.array([0.1, 0.3, 1.0, 2.0, 7.0, 50.0])
    s_e_min, s_de, S = api.resample_spectrum(e, np.log(e), 33)
    nodes = s_e_min * s_de ** np.arange(33)
    assert s_e_min == 0.1 and abs(nodes[-1] / 50.0 - 1) < 1e-12 and S.shape == (33,)
    assert np.allclose(S, np.log(nodes), rtol=1e-12, atol=1e-12)                             # linear in log E: exact for counts = log E
    with pytest.raises(api.KrError):
        api.resample_spectrum([1.0, 0.5], [1.0, 1.0], 8)
