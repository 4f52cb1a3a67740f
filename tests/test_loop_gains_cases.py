"""What tests/test_gpu_loop_gains.py takes for granted, checked without a GPU: its cases reach every producer and sweep class of
the solve loop in both modes, the Python mirror of the loop's route selection (tests/loop_gains_cases.py) reads the launchers'
tables, and every `last` case meets -- on the oracle alone, with its committed seed -- the conditions that keep the GPU test from
passing on nothing."""
import numpy as np
import pytest

from tests import linesearch_cases as lc
from tests import loop_gains_cases as lg

CASES = lg.all_cases()
LAST = [c for c in CASES if c.mode == "last"]


def test_constants_are_read_from_the_sources():
    assert lg.WAVE_SIZES == lg.TEAM_SIZES == {(4, 2), (8, 4), (12, 6), (16, 8), (20, 10)}
    assert (6, 4, 2) in lg.WG_SIZES and (10, 6, 3) in lg.WG_SIZES and (5, 12, 4) in lg.WG_RECORD_SIZES and not lg.WG_SIZES & lg.WG_RECORD_SIZES
    assert lg.TILES_WAVE_TABLE == {(0, k) for k in range(1, 7)}
    assert (lg.BIG_ABOVE, lg.TIER12_ABOVE, lg.TIER8_ABOVE, lg.TEAM_MAX) == (60, 2048, 1024, lc.TEAM_MAX)
    assert lg.STATIC_MODELS == (0, 1, 6)
    assert {"DPILQR_NO_FUSED", "DPILQR_TILES_NO_STATIC", "DPILQR_TILES_GENERIC", "DPILQR_MFMA_WAVES", "DPILQR_NO_TEAM",
            "DPILQR_FORCE_BIG", "DPILQR_INPROD_RECORDS"} <= set(lg.ROUTE_SWITCHES)
    assert lg.MU_SCHEDULE == [1.0, 0.5, 0.125, 2.0 ** -6, 2.0 ** -10, 2.0 ** -15, 0.0]


def test_every_class_appears_in_both_modes():
    for mode in ("first", "last"):
        routes = [lg.loop_route(c) for c in CASES if c.mode == mode]
        assert {p for p, _ in routes} == set(lg.PRODUCERS) - {"static+sparse"}, mode
        assert {s for _, s in routes} == set(lg.SWEEPS), mode
    assert all(p in lg.PRODUCERS and s in lg.SWEEPS for p, s in map(lg.loop_route, CASES))
    assert len({c.id for c in CASES}) == len(CASES)


def test_static_part_with_the_generic_producer_serves_no_shape():
    """k_make_tiles<NS, NC, true> with dyn_only = 1 (`static+sparse`): the static part needs one of the linear models for the
    whole batch, and every cluster of those that keeps records -- six DoubleIntDynamics4D -- has a k_make_tiles_wave
    instantiation; the six-state linear models never keep records (in-sweep production up to four agents, the fused workgroup
    sweep up to ten, the large-cluster path beyond).  No case can reach the class without a route switch."""
    for m in lc.MODEL_DIMS:
        for k in range(1, 26):
            for per_agent in (False, True):
                assert lg.loop_route(lg.Case([m] * k, 8, 8, "first", 1, per_agent=per_agent))[0] != "static+sparse", (m, k)


def test_launch_widths_cover_the_team_and_every_tier():
    first = [c for c in CASES if c.mode == "first"]
    for models in ([0] * 5, [0] * 6):
        assert sorted(c.window for c in first if c.models == models and c.B > 260) == [700, 1100, 2100]
    assert {lg.sweep_tier(c) for c in first if c.models == [0] * 5} == {4, 8, 12}
    assert {(lg.loop_route(c)[1], lg.sweep_tier(c)) for c in first if c.models == [0] * 6} == {("record-fed wavefront", 4), ("record-fed wavefront", 8)}
    assert all(c.window == c.B for c in first)
    assert sorted(c.models for c in LAST if c.window == 7) == [[0] * 6, [7] * 2]
    assert all(len(c.checked()) <= 46 and c.checked()[-1] == c.B - 1 for c in CASES)


def test_big_agrees_with_the_line_search_cases():
    """lc.expected_route calls `big` what leaves the LDS-staged k_forward; of those, the clusters with n_x > 60 -- and only they
    -- take the large-cluster sweep."""
    for c in CASES:
        n_x = c.k * lc.MODEL_DIMS[c.models[0]][0]
        big = lg.loop_route(c) == ("big", "big")
        assert big == (c.expected_route() == "big" and n_x > lg.BIG_ABOVE), c.id
        assert big or "big" not in lg.loop_route(c), c.id
    assert any(c.expected_route() == "big" and lg.loop_route(c)[1] == "record-fed workgroup" for c in CASES)      # five Quadcopter12D


def test_bounds():
    assert lg.GainsRef.bound_of(0.0) == lg.TOL_PASS and lg.GainsRef.bound_of(1e-10) == 1e-8
    assert lg.GainsRef.bound_of(2e-7) is None and lg.GainsRef.bound_of(np.inf) is None and lg.GainsRef.bound_of(np.nan) is None
    c = CASES[0]
    b = lg.make_batch(c, B=2)
    p = lg.item_problem(b, 1)
    X, _ = p.rollout(b["x0"][1], b["U0"][1])
    ref = lg.GainsRef(p, X, b["U0"][1], 1.0)
    assert ref.K.shape == (b["T"], 12, 24) and 0.0 < ref.spread_K < 1e-9 and ref.bound_K == ref.bound_d == lg.TOL_PASS


@pytest.mark.parametrize("case", LAST, ids=[c.id for c in LAST])
def test_last_cases_meet_their_conditions_on_the_oracle(case):
    b = lg.make_batch(case)
    st = lg.LastStats()
    for i in case.checked():
        p = lg.item_problem(b, i)
        r = lg.oracle_last(p, b["x0"][i], b["U0"][i])
        if r["status"] == 2:
            assert r["mu"] in lg.MU_SCHEDULE
            st.add(2, r["mu"], lg.GainsRef(p, r["X"], r["U"], r["mu"]))
        else:
            st.add(r["status"])
    st.check()
