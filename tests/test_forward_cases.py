"""What tests/test_gpu_forward.py takes for granted, checked without a GPU: its cases reach every rollout instantiation the
launcher's source names and every route either mode can take, and -- from the reference alone -- every case is one the check
means something on: few items without a bound, pairs inside the radius, costs that depend on alpha."""
import pytest

from tests import forward_cases as fc
from tests import linesearch_cases as lc

ALL = fc.ROLLOUT_CASES + fc.CANDIDATES_CASES


def test_rollout_table_and_routes():
    assert len(fc.RO_TABLE) == 75
    assert len({c.id for c in ALL}) == len(ALL)
    assert all(c.expected_route() == c.route for c in ALL), [c.id for c in ALL if c.expected_route() != c.route]
    waved = {(c.models[0], c.k) for c in fc.ROLLOUT_CASES if c.route == "wave"}
    assert not [key for key in fc.RO_TABLE if key not in waved]
    full = {(c.models[0], c.k) for c in fc.ROLLOUT_CASES if c.route == "wave" and c.B == 4 * (64 // c.k) + 1 and c.weights == "shared"}
    assert full == fc.RO_TABLE                      # one full workgroup plus one item, for every instantiation
    # every route a mode can take (a rollout has no gains and never takes the matrix pipe; the wave kernels are rollouts)
    assert {c.route for c in fc.ROLLOUT_CASES} == fc.REACHABLE["rollout"]
    assert {c.route for c in fc.CANDIDATES_CASES} == fc.REACHABLE["candidates"]
    assert fc.REACHABLE["rollout"] | fc.REACHABLE["candidates"] == set(fc.ROUTES)
    assert {fc.staged_threads(c.models, len(c.alpha_values())) for c in fc.CANDIDATES_CASES if c.route == "staged"} == {128, 192, 256}
    # the alpha sets: one, three and ten of the table, two values off it, and the longest prefix that fits where ten do not
    assert {c.alphas for c in fc.CANDIDATES_CASES} == {"P1", "P3", "P10", "OFF", "P8"}
    for c in fc.CANDIDATES_CASES:
        if c.alphas == "P8":
            assert c.k * 8 <= 256 < c.k * 9
    for route in fc.REACHABLE["candidates"]:
        of = [c for c in fc.CANDIDATES_CASES if c.route == route]
        assert {c.uniform for c in of} == {True, False} and len({c.weights for c in of}) >= 2, route
        if route == "staged-packed":
            assert any(c.B % 4 == 1 and c.B > 4 for c in of)
        assert any(c.B > 1 for c in of)
    assert any(c.B % 4 == 1 and c.weights == "per_item" for c in fc.ROLLOUT_CASES if c.route == "staged-packed")


def test_samples_cover_every_route():
    for mode in ("rollout", "candidates"):
        assert {fc.by_id(s).route for s in fc.ROUTE_SAMPLES if fc.by_id(s).mode == mode} == fc.REACHABLE[mode]
    assert all(fc.by_id(s).B > 1 for s in fc.ROUTE_SAMPLES)
    assert {(fc.by_id(s).mode, fc.by_id(s).route) for s in fc.POISON_SAMPLES} == {("rollout", "wave"), ("rollout", "staged-packed"),
                                                                                  ("candidates", "staged-packed")}
    for pub in map(fc.by_id, fc.PUBLIC_PATH_CASES):
        assert pub.route == "big-nopipe" and pub.mode == "candidates" and len(pub.alpha_values()) == 1
    assert any(c.k * c.nc > 64 for c in map(fc.by_id, fc.PUBLIC_PATH_CASES))      # more controls than one alpha's launch has threads


def test_pipe_predicate_agrees_with_the_line_search_mirror():
    """At the solve loop's ten candidates the predicate with the thread count as an argument is linesearch_cases's, which
    tests/test_linesearch_cases.py holds to forward.hpp itself."""
    for (ns, nc) in sorted(set(lc.MODEL_DIMS.values())):
        for k in range(1, 26):
            n, m = k * ns, k * nc
            assert fc.forward_on_pipe(n, m, k, fc.forward_threads(k, 10), 10) == lc.forward_on_pipe(n, m, k), (ns, k)


def test_big_nopipe_in_candidates_mode_is_what_one_alpha_launches():
    """k_forward<double, NS, NC, true, false> WITH gains: with one alpha a launch has 64 threads and forward_on_pipe allows two
    row tiles of sixteen controls, so every large cluster with n_u > 32 is off the pipe -- config 5's n_u = 80 included."""
    assert fc.expected_route("candidates", [7] * 14 + [8] * 6, 1) == "big-nopipe"
    assert fc.expected_route("candidates", [7] * 14 + [8] * 6, 10) == "big-pipe"
    for m0, (ns, nc) in lc.MODEL_DIMS.items():
        for k in range(1, 41):
            if k * ns > 60 and k * ns <= 240:
                assert (fc.expected_route("candidates", [m0] * k, 1) == "big-nopipe") == (k * nc > 32), (m0, k)


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_case_conditions(case):
    r = fc.case_ref(case)
    idx = r.idx
    assert idx[0] == 0 and idx[-1] == case.B - 1 and max(case.B - 2, 0) in idx
    print(f"FWD_CPU {case.id} checked={len(idx)} unchecked={r.unchecked_fraction():.3f} near={r.near_fraction():.2f} max_spread={r.max_spread():.2e}")
    assert r.unchecked_fraction() <= fc.MAX_UNCHECKED
    if case.k >= 2:
        assert r.near_fraction() >= fc.MIN_NEAR
    if case.mode == "candidates":
        assert all(r.costs_differ(i) for i in idx)
