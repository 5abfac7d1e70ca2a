"""CPU: the numpy rule of the landing map (tests/return_map_rules.py) against the two rule sets it is made of, both pinned to the oracle by
tests/test_reducer_rules.py: its four scalars are reducer_rules.reduce_return's, and with unit weights (plane_iso = limb = 0) its count / flux / emis
/ time planes are reducer_rules.reduce_emissivity's count / flux / emis / sum_time on the `return`-class records with num_primary_rays = 1 --
exactly, NaN for NaN -- over the chosen records of tests/reducer_cases.py, all eight weight cases, nr on either side of the LDS capacity and both
bin kinds."""
import numpy as np
import pytest

import reducer_cases as rc
import reducer_rules as rr
import return_map_rules as rm
from raytrace_cpu_amd import capi

NRS = (1, 7, 1024, 1025)
CASES = [(case, nr, lb) for case in sorted(rc.return_cases()) for nr in NRS for lb in (0, 1)]


def landing_map(case, nr, logbin):
    eb = rc.emis_bins(nr, logbin)
    return rm.map_struct(rc.return_cases()[case], eb.r_min, eb.dr, nr, logbin, eb.gamma)


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@pytest.mark.parametrize("case,nr,logbin", CASES, ids=[f"{c}-{'log' if lb else 'lin'}-nr{nr}" for c, nr, lb in CASES])
def test_map_rule_is_the_return_rule_and_the_emissivity_rule(case, nr, logbin):
    rays = rc.small().return_rays
    m = landing_map(case, nr, logbin)
    got = rm.reduce_return_map(m, rays)
    assert same(got["scalars"], rr.reduce_return(m.cls, rays))
    assert got["on_disc"] >= got["binned"] == int(got["count"].sum())
    if m.cls.plane_iso or m.cls.limb:
        return
    rec = rays[rays["steps"] > 0]
    ret = rec[rm.return_class(m.cls, rec, rec["phi"])]
    eb = capi.EmisBins()
    eb.r_min, eb.dr, eb.r_isco, eb.gamma, eb.spin, eb.num_primary_rays, eb.nr, eb.logbin = m.r_min, m.dr, m.cls.r_isco, m.gamma, 0.998, 1.0, nr, logbin
    want = rr.reduce_emissivity(eb, ret)
    assert want["disc_count"] == (ret["redshift"] > 0).sum() and got["on_disc"] == len(ret)
    for mine, theirs in (("count", "count"), ("flux", "flux"), ("emis", "emis"), ("time", "sum_time")):
        assert same(got[mine], want[theirs]), (mine, case, nr, logbin)
        if mine != "count":
            assert same(got["abs"][mine], want["abs"][theirs])
    assert same(got["weight"], got["count"]) and same(got["abs"]["weight"], got["count"])


def test_the_record_set_exercises_the_rule():
    """Every class, the self-zone, g <= 0 and NaN among the returning records, and non-finite sums."""
    rec = rc.small()
    rays = rec.return_rays
    m = landing_map("iso1-limb1-norm1", 7, 1)
    plain = rm.reduce_return_map(m, rays)
    assert plain["on_disc"] > plain["binned"] > rc.N_CONTENTION
    assert np.isnan(plain["scalars"][1:]).all() and np.isnan(plain["weight"]).any() and not np.isnan(plain["weight"]).all()
    assert not np.isfinite(plain["time"][np.isfinite(plain["weight"])]).all()           # a poison record without a NaN weight
    live = rays[rays["steps"] > 0]
    ret = live[rm.return_class(m.cls, live, live["phi"])]
    with np.errstate(invalid="ignore"):
        assert (ret["redshift"] <= 0).any() and np.isnan(ret["redshift"]).any()
    fin = rm.reduce_return_map(m, rays[~rec.nan_weight & ~rec.poison])
    assert all(np.isfinite(fin[k]).all() for k in rm.MAP_SUMS) and np.isfinite(fin["scalars"]).all() and (fin["scalars"] > 0).all()
