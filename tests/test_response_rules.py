"""CPU: the numpy statement of the reverberation-response rule (tests/response_rules.py) against the text of include/kr_trace.h (kr_response_model), on
synthetic records: where the edges of the time window fall, what a NaN time and a non-finite table_time do, that the rows sum to the spectrum of
tests/spectrum_rules.py, and additivity.  No device, no library call."""
import numpy as np
import pytest

import response_rules as rr
import spectrum_rules as sr
from raytrace_cpu_amd import capi

R_ISCO, R_DISC = 1.5, 30.0


def spec(ne=12, nz=2, table_emis=None, nr=8):
    s_ne = 40
    s_de = (1e4) ** (1.0 / (s_ne - 1))
    e = 0.01 * s_de ** np.arange(s_ne)
    S = np.array([e ** -(1.5 + 0.25 * z) for z in range(nz)])
    extra = dict(table_emis=table_emis) if table_emis is not None else {}
    return capi.spectrum_model("table", 0.5, 1.2, ne, log_e=True, r_isco=R_ISCO, r_disc=R_DISC, q1=3.0, rb1=4.0, q2=2.5, rb2=10.0, q3=3.0, s=S, s_e_min=0.01,
                               s_de=s_de, table_r_min=R_ISCO, table_dr=(R_DISC / R_ISCO) ** (1.0 / nr), **extra)


def test_the_edges_of_the_time_window():
    """t0 = 8, dt = 0.5, nt = 4: ft = (t - 8) / 0.5 is exact for these t.  ft exactly 0 is row 0; just below 0 is outside; just below nt is row nt - 1;
    exactly nt is outside; a NaN t is outside.  All of them are `used`."""
    t = np.array([8.0, np.nextafter(8.0, 0.0), np.nextafter(10.0, 0.0), 10.0, np.nan, 9.25])
    rays = rr.synthetic_records(np.full(6, 5.0), np.full(6, 0.8), t)
    R = capi.response_model(spec(), 8.0, 0.5, 4)
    res = rr.response(R, rays)
    assert list(res["row"]) == [0, -1, 3, -1, -1, 2]
    assert rr.tallies(res) == (6, 6, 0, 3)
    one = rr.response(R, rays[:1])["resp"][0]
    assert one.max() > 0 and np.array_equal(res["resp"][0], one) and np.array_equal(res["resp"][3], one) and np.array_equal(res["resp"][2], one)
    assert not res["resp"][1].any()


def test_a_record_without_ir_or_with_a_non_finite_time_is_not_used():
    """table_time alone (no table_emis) still needs ir: a record outside the table, or in a bin whose time is NaN or inf, passes the filter, is not used
    and does not count in `outside`."""
    nr = 8
    time = np.linspace(3.0, 10.0, nr)
    time[2], time[5] = np.nan, np.inf
    m = spec(nr=nr)
    m.table_r_min, m.table_dr = 3.0, 1.3                           # r in [R_ISCO, 3 / 1.3) has fi <= -1: no ir
    R = capi.response_model(m, 0.0, 1.0, 64, table_time=time)
    assert R.spec.table_nr == nr
    dr = m.table_dr
    r = np.array([1.55, 3.0 * dr ** 0.5, 3.0 * dr ** 2.5, 3.0 * dr ** 5.5, 3.0 * dr ** 7.5])
    assert r[0] * dr < 3.0 and r[-1] < R_DISC
    rays = rr.synthetic_records(r, np.full(5, 0.9), np.full(5, 20.0))
    res = rr.response(R, rays)
    assert list(res["used_index"]) == [1, 4] and rr.tallies(res) == (5, 2, 0, 0)
    assert list(res["row"]) == [int(20.0 + time[0]), int(20.0 + time[7])]
    # the same with table_emis present: a non-finite emissivity drops the record too
    emis = np.ones(nr)
    emis[7] = np.nan
    m2 = spec(nr=nr, table_emis=emis)
    m2.table_r_min, m2.table_dr = 3.0, 1.3
    R2 = capi.response_model(m2, 0.0, 1.0, 64, table_time=time)
    assert list(rr.response(R2, rays)["used_index"]) == [1]
    with pytest.raises(ValueError):
        capi.response_model(m2, 0.0, 1.0, 64, table_time=time[:-1])


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("tables", [False, True])
def test_the_rows_sum_to_the_spectrum(dtype, tables):
    rng = np.random.default_rng(5)
    n, nr = 700, 8
    r, g, t = rng.uniform(1.0, 35.0, n), rng.uniform(0.3, 1.3, n), rng.uniform(100.0, 140.0, n)
    m = spec(nz=3, nr=nr, table_emis=np.linspace(2.0, 0.2, nr) if tables else None)
    R = capi.response_model(m, 90.0, 0.37, 200, table_time=np.linspace(1.0, 9.0, nr) if tables else None)
    rays = rr.synthetic_records(r, g, t)
    rays["steps"][::17] = 0
    res, flux = rr.response(R, rays, dtype=dtype), sr.spectrum(R.spec, rays, dtype=dtype)
    assert res["outside"] == 0 and res["used"] == flux["used"] > 400 and res["on_disc"] == flux["on_disc"]
    assert np.array_equal(res["used_index"], flux["used_index"])
    assert len(set(res["row"])) > 50
    assert sr.rel_diff(res["resp"].sum(axis=0), flux["flux"]) <= 1e-13
    noise, lo, hi = rr.noise(R, rays)
    assert 0 < noise < 1e-13


def test_additive_over_a_split():
    rng = np.random.default_rng(6)
    n = 300
    rays = rr.synthetic_records(rng.uniform(1.0, 35.0, n), rng.uniform(0.3, 1.3, n), rng.uniform(0.0, 50.0, n))
    R = capi.response_model(spec(), 5.0, 1.5, 20)
    whole, a, b = rr.response(R, rays), rr.response(R, rays[:113]), rr.response(R, rays[113:])
    assert whole["outside"] > 0 and whole["used"] - whole["outside"] > 100
    assert rr.tallies(whole) == tuple(x + y for x, y in zip(rr.tallies(a), rr.tallies(b)))
    assert sr.rel_diff(a["resp"] + b["resp"], whole["resp"]) <= 1e-14
    assert np.array_equal((a["resp"] + b["resp"]) == 0, whole["resp"] == 0)
