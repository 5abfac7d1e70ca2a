"""CPU: the lag layer on top of an energy-time response (api.lag_spectra, api.lag_energy, api.gravitational_time) against closed forms.  Host numpy
only: no library call."""
import numpy as np

from raytrace_cpu_amd import api

NT, NE, DT = 64, 10, 0.5
J0, I0, A, C_BAND, C_REF, REFL = 9, 6, 3.0, 2.0, 5.0, 0.7
TAU0 = (J0 + 0.5) * DT
WIDTHS = np.linspace(0.5, 1.4, NE)
BAND, REF = np.arange(5, 8), np.arange(0, 3)


def delta_response():
    """Zero except one cell in row J0, energy I0 (inside BAND); the continuum puts C_BAND into BAND and C_REF into REF."""
    resp = np.zeros((NT, NE))
    resp[J0, I0] = A / WIDTHS[I0]                                  # r_band[J0] = A
    cont = np.zeros(NE)
    cont[BAND] = C_BAND / (3 * WIDTHS[BAND])
    cont[REF] = C_REF / (3 * WIDTHS[REF])
    return resp, cont


def closed_form(f):
    s, w = np.sinc(f * DT), 2 * np.pi * f
    return np.arctan2(REFL * A * s * np.sin(w * TAU0), C_BAND + REFL * A * s * np.cos(w * TAU0)) / w


def test_delta_response_has_the_closed_form_lag_through_the_phase_wrap():
    resp, cont = delta_response()
    f = np.geomspace(1e-3, 0.9 / DT, 400)
    assert (f > 1 / (2 * TAU0)).sum() > 100 and (f < 1 / (2 * TAU0)).sum() > 100
    res = api.lag_spectra(resp, DT, WIDTHS, f, BAND, REF, cont=cont, refl=REFL)
    want = closed_form(f)
    assert (want < 0).any() and (want > 0).any()                   # the wrap above f = 1 / (2 tau0)
    assert np.abs(res["lag"] - want).max() <= 1e-12
    assert np.abs(res["H_ref"] - C_REF).max() <= 1e-14 and np.abs(res["cross"] - np.conj(res["H_ref"]) * res["H_band"]).max() == 0
    assert np.abs(res["H_band"] - (C_BAND + REFL * A * np.sinc(f * DT) * np.exp(-2j * np.pi * f * TAU0))).max() <= 1e-13


def test_low_frequency_limit_is_the_diluted_delay():
    resp, cont = delta_response()
    f = np.array([1e-7, 1e-6])
    res = api.lag_spectra(resp, DT, WIDTHS, f, BAND, REF, cont=cont, refl=REFL)
    want = REFL * A * TAU0 / (C_BAND + REFL * A)
    assert np.abs(res["lag"] / want - 1).max() <= 1e-9
    # without a continuum the lag is the delay itself (the reference band needs something to be measured against: a response at row 0)
    resp[0, 1] = 1.0
    undiluted = api.lag_spectra(resp, DT, WIDTHS, f, BAND, REF)
    assert np.abs(undiluted["lag"] / (TAU0 - 0.5 * DT) - 1).max() <= 1e-9


def test_swapping_band_and_reference_negates_the_lag():
    rng = np.random.default_rng(11)
    resp, cont = rng.uniform(0, 1, (NT, NE)) * np.exp(-np.arange(NT) / 9.0)[:, None], rng.uniform(0.5, 2, NE)
    f = np.geomspace(1e-3, 0.4 / DT, 60)
    a = api.lag_spectra(resp, DT, WIDTHS, f, BAND, REF, cont=cont, refl=REFL)
    b = api.lag_spectra(resp, DT, WIDTHS, f, REF, BAND, cont=cont, refl=REFL)
    assert np.abs(a["lag"]).max() > 1e-3 and np.abs(a["lag"] + b["lag"]).max() <= 1e-13
    assert np.abs(a["cross"] - np.conj(b["cross"])).max() <= 1e-12 * np.abs(a["cross"]).max()
    mask = np.zeros(NE, dtype=bool)
    mask[BAND] = True
    assert np.array_equal(api.lag_spectra(resp, DT, WIDTHS, f, mask, slice(0, 3), cont=cont, refl=REFL)["lag"], a["lag"])


def test_lag_energy_of_an_energy_independent_response_is_flat():
    row = np.exp(-np.arange(NT) / 7.0)
    resp = np.repeat(row[:, None], NE, axis=1) / WIDTHS[None, :]   # resp[j, i] widths[i] the same for every i
    cont = 0.8 / WIDTHS
    f = np.linspace(0.01, 0.05, 9)
    res = api.lag_energy(resp, DT, WIDTHS, f, REF, cont=cont, refl=REFL)
    assert res["lag"].shape == (NE,) and res["H"].shape == (9, NE)
    assert np.abs(res["lag"] - res["lag"][0]).max() <= 1e-13
    # every energy carries a third of the reference band's cross-spectrum with itself, whose argument is 0: no lag at all
    assert np.abs(res["lag"]).max() <= 1e-13
    # one energy delayed by whole rows lags by about that much more at low frequency
    resp[:, 8] = np.roll(resp[:, 8], 4)
    resp[:4, 8] = 0
    shifted = api.lag_energy(resp, DT, WIDTHS, np.array([1e-4]), REF, refl=1.0)
    flat = np.delete(shifted["lag"], 8)
    assert np.abs(flat - flat[0]).max() <= 1e-9 and 0.8 * 4 * DT < shifted["lag"][8] - flat[0] < 1.2 * 4 * DT
    # each energy as its own band of lag_spectra, frequency by frequency
    one = api.lag_spectra(resp, DT, WIDTHS, np.array([0.03]), np.array([8]), REF, cont=cont, refl=REFL)
    same = api.lag_energy(resp, DT, WIDTHS, np.array([0.03]), REF, cont=cont, refl=REFL)
    assert abs(one["lag"][0] - same["lag"][8]) <= 1e-14 and abs(one["cross"][0] - same["cross"][8]) <= 1e-13 * abs(one["cross"][0])


def test_gravitational_time():
    assert abs(api.gravitational_time(1.0) / 4.9255e-6 - 1) <= 1e-4
    assert abs(api.gravitational_time(1e7) / (1e7 * api.gravitational_time(1.0)) - 1) < 1e-15          # linear in the mass
