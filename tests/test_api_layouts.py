"""CPU: every result-buffer layout of api.py -- the length function and the dict made of the words -- at the smallest shape where every axis length
differs, on words = 0, 1, 2, ..  The expected values are sliced out by hand here: key order, dtype, shape and content are all pinned."""
import numpy as np
import pytest

from raytrace_cpu_amd import api, capi


def words_of(nw, lead=()):
    return np.arange(int(np.prod(lead + (nw,))), dtype=float).reshape(lead + (nw,))


def same(got, want):
    assert list(got) == list(want), "keys and their order"
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True), k
        else:
            assert type(g) is type(w) and (g == w or (w != w and g != g)), k


def image_bins(nx=2, ny=3):
    b = capi.ImageBins()
    b.img_nx, b.img_ny = nx, ny
    return b


def want_image(w, npix=6):
    return {"nrays": np.arange(npix, dtype=np.int32), "disc_count": 7 * npix, "flux": w[6:12], "r": w[12:18], "phi": w[18:24], "enshift": w[24:30],
            "time": w[30:36], "emis": w[36:42]}


def test_image():
    w = words_of(43)
    same(api.image_planes_from_words(w, 2, 3), want_image(w))


def test_image_words():
    assert api.image_words(image_bins()) == 43


@pytest.mark.parametrize("logbin", [False, True])
def test_return_map(logbin):
    m = api.return_map_struct(1.3, 50.0, 100.0, 6.0, 1.5, 2.0, 1.5, 3, logbin)
    assert api.return_map_words(m) == 21
    w = words_of(21)
    same(api.return_map_from_words(m, w),
         {"count": w[0:3], "weight": w[3:6], "flux": w[6:9], "emis": w[9:12], "time": w[12:15], "ray_count": 15.0, "return": 16.0, "escape": 17.0, "lost": 18.0,
          "on_disc": 19, "binned": 20, "r_edges": 2.0 * 1.5 ** np.arange(4) if logbin else 2.0 + 1.5 * np.arange(4)})


def test_return_radiation_planes():
    """The (nsrc, nr) planes and per-radius scalars of return_radiation(): two radii of three bins."""
    w = words_of(21, (2,))
    same(api.return_radiation_from_words(3, w),
         {"count": w[:, 0:3], "weight": w[:, 3:6], "flux": w[:, 6:9], "emis": w[:, 9:12], "time": w[:, 12:15], "ray_count": w[:, 15], "return": w[:, 16],
          "escape": w[:, 17], "lost": w[:, 18], "on_disc": w[:, 19], "binned": w[:, 20]})
    same(api.return_radiation_from_words(3, np.zeros((0, 21))), {k: np.zeros((0, 3)) for k in api.RETURN_MAP_PLANES} | {k: np.zeros(0) for k in api.RETURN_MAP_SCALARS})


@pytest.mark.parametrize("log_e,time_axis", [(False, True), (True, True), (False, False)])
def test_line(log_e, time_axis):
    nt, ne = (2, 3) if time_axis else (1, 3)
    b = capi.line_bins(e_min=2.0, de=1.5, ne=ne, log_e=log_e, t0=10.0, dt=5.0 if time_axis else 0.0, nt=nt)
    nw = 2 * nt * ne + 2
    assert api.line_words(b) == nw
    w = words_of(nw)
    same(api.line_from_words(b, w),
         {"count": w[:nt * ne].reshape(nt, ne), "flux": w[nt * ne:2 * nt * ne].reshape(nt, ne), "on_disc": nw - 2, "binned": nw - 1,
          "energy_edges": 2.0 * 1.5 ** np.arange(4) if log_e else 2.0 + 1.5 * np.arange(4), "time_edges": 10.0 + 5.0 * np.arange(3) if time_axis else None})


def test_caustic():
    cm = capi.CausticMap()
    cm.nx, cm.ny = 2, 3
    assert api.caustic_words(cm) == 9 * 6 + 7 == 61
    w = words_of(61)
    want = {k: w[6 * q:6 * q + 6].reshape(2, 3) for q, k in enumerate(("det_j", "sign_j", "order", "hit", "radius", "phi", "x_disc", "y_disc", "redshift"))}
    want.update(disc_count=54, horizon=55, rlim=56, steplim=57, out_of_range=58, other=59, suppressed=60)
    same(api.caustic_from_words(cm, w), want)


@pytest.mark.parametrize("kind,planes,counts", [
    ("sphere", ("det_j", "sign_j", "order", "escaped", "theta_s", "phi_s", "rdot_flips", "equat_cross"), ("escaped_count", "captured", "steplim")),
    ("plane", ("det_j", "sign_j", "order", "hit_plane", "x_s", "y_s", "rdot_flips", "equat_cross"), ("hit_count", "captured", "steplim"))])
def test_source_caustic(kind, planes, counts):
    sm = api.source_map_struct(kind, 2, 3, 0.1, 0.2)
    assert api.source_caustic_words(sm) == 8 * 6 + 3 == 51
    w = words_of(51)
    want = {k: w[6 * q:6 * q + 6].reshape(2, 3) for q, k in enumerate(planes)}
    want.update({k: 48 + q for q, k in enumerate(counts)})
    same(api.source_caustic_from_words(sm, w), want)


def test_volume():
    m = api.volume_map_struct(1.5, 20.0, 3, 2, 4, True)
    assert api.volume_words(m) == 3 * 24 + 4 == 76
    w = words_of(76)
    same(api.volume_from_words(m, w), {"count": w[0:24].reshape(3, 2, 4), "time": w[24:48].reshape(3, 2, 4), "redshift": w[48:72].reshape(3, 2, 4),
                                       "rows": 72, "in_grid": 73, "deposits": 74, "bad_g": 75})


@pytest.mark.parametrize("logbin_en", [False, True])
def test_observe(logbin_en):
    b = api.observe_bins_struct(0.5, 2.0, 3, logbin_en, tmax=10.0, nt=2)
    assert api.observe_words(b) == 3 + 3 + 6 + 6 == 18
    w = words_of(18)
    i = np.arange(4, dtype=np.float64)
    same(api.observe_from_words(b, w),
         {"energy": 0.5 * np.power(b.den, i) if logbin_en else 0.5 + b.den * i, "spectrum": w[0:3], "hits": w[3:6], "response": w[6:12].reshape(3, 2),
          "rows": 12, "in_grid": 13, "lit": 14, "contributions": 15, "bad_g": 16, "degenerate": 17})
    none = api.observe_bins_struct(0.5, 2.0, 3)
    assert api.observe_words(none) == 12 and api.observe_from_words(none, words_of(12))["response"].shape == (3, 0)


def test_healpix_map():
    m = api.healpix_map_struct(12, 1.3, 50.0, 100.0)
    assert api.healpix_map_words(m) == 7 * 12 + 6 == 90          # six tally words, five of them named
    w = words_of(90)
    want = {"class": np.arange(12, dtype=np.int64)}
    want.update({k: w[12 * q:12 * q + 12] for q, k in enumerate(("r", "theta", "phi", "g", "t", "emis"), 1)})
    want.update(live=84, disc=85, escape=86, lost=87, self=88, disc_frac=85.0 / 84.0, escape_frac=86.0 / 84.0, lost_frac=87.0 / 84.0, self_frac=88.0 / 84.0)
    same(api.healpix_map_from_words(m, w), want)
    got = api.healpix_map_from_words(m, np.zeros(90))
    assert all(np.isnan(got[k]) for k in ("disc_frac", "escape_frac", "lost_frac", "self_frac")), "no live ray: 0 / 0"


def emis_bins(nr=3):
    b = capi.EmisBins()
    b.nr = nr
    return b


def test_emissivity():
    """The histogram of kr_reduce_emissivity_dev_f64 / kr_post_emissivity_*: the dict reduce_emissivity returns."""
    assert api.emissivity_words(emis_bins()) == 5 * 3 + 1 == 16
    w = words_of(16) + 0.75                                        # count and disc_count are truncated, as int() and astype do
    same(api.emissivity_from_words(emis_bins(), w), {"count": np.arange(3, dtype=np.int64), "flux": w[3:6], "emis": w[6:9], "sum_redshift": w[9:12],
                                                     "sum_time": w[12:15], "disc_count": 15})


def test_emissivity_mu():
    assert api.emissivity_mu_words(emis_bins(), 2) == (2 * 2 + 1) * 3 + 3 == 18
    assert api.emissivity_mu_words(emis_bins(), 0) == 6
    w = words_of(18)
    same(api.emissivity_mu_from_words(emis_bins(), 2, w), {"count2": np.arange(6, dtype=np.int64).reshape(3, 2), "flux2": w[6:12].reshape(3, 2), "sum_mu": w[12:15],
                                                           "disc_count": 15, "binned": 16, "bad_angle": 17})
