"""What the CPU alone says about the capped-neighbourhood cases (tests/nearest_cases.py), without a GPU: the cases' margins (a
condition on the cases, so that rounding or a fused multiply-add in dx*dx + dy*dy cannot move a mask), the uncapped sizes the
module docstring quotes, dpilqr_amd.distributed.nearest_neighbourhoods against the brute-force reference, the hand-made scenarios'
points, and that the oracle's capped distributed solves are well conditioned -- so that tests/test_gpu_nearest.py can hold them
to TOL_SOLVE."""
import numpy as np
import pytest

from tests import nearest_cases as nc

SIZES = {6: (6, 6), 64: (61, 64), 65: (58, 65), 130: (70, 130), 256: (70, 229)}      # uncapped, scenario 0, all 11 rows


def _forms(case):
    """(label, X) of every scenario in both forms: the first row alone, and all ROWS rows"""
    x0, _, X = nc.scenario(case.k)
    for s in range(nc.S):
        yield f"s{s}-row0", x0[s][None]
        yield f"s{s}-rows", X[s]


@pytest.mark.parametrize("case", nc.CASES, ids=nc.IDS)
def test_margins_and_sizes(case):
    worst_gap, worst_thr, bites = np.inf, np.inf, 0
    for label, X in _forms(case):
        graph, dropped, sizes, gap, thr_margin = nc.reference(X, case.k, nc.NS, nc.GRAPH_RADIUS, case.m)
        worst_gap, worst_thr, bites = min(worst_gap, gap), min(worst_thr, thr_margin), bites + int((dropped > 0).sum())
        assert max(len(v) for v in graph.values()) <= case.m and (dropped == sizes - [len(graph[i]) for i in range(case.k)]).all()
        if label == "s0-rows":
            assert (int(sizes.min()), int(sizes.max())) == SIZES[case.k], (sizes.min(), sizes.max())
        P = np.atleast_2d(X).reshape(-1, case.k, nc.NS)[:, :, :2]
        sep = min(float(np.sqrt(((P[r][:, None] - P[r][None]) ** 2).sum(-1) + 1e9 * np.eye(case.k)).min()) for r in range(P.shape[0]))
        assert sep > nc.COST_RADIUS + 0.05, (label, sep)      # the proximity cost stays out of play
    print(f"\n[nearest margins {case.id}] smallest key gap at the cut {worst_gap:.3g}, smallest |key - thr| {worst_thr:.3g} (both >= {nc.MARGIN:g} "
          f"asked); agents the cap bites {bites}")
    assert worst_thr >= nc.MARGIN and worst_gap >= nc.MARGIN
    assert bites > 0


def _as_index_graph(g, ids):
    return {ids.index(id_): [ids.index(int(j)) for j in v] for id_, v in g.items()}


@pytest.mark.parametrize("case", nc.CASES, ids=nc.IDS)
def test_nearest_neighbourhoods_equals_the_brute_force_reference(case):
    from dpilqr_amd.distributed import define_inter_graph_threshold, nearest_neighbourhoods
    ids = [100 + 3 * i for i in range(case.k)]
    for label, X in _forms(case):
        want = nc.reference(X, case.k, nc.NS, nc.GRAPH_RADIUS, case.m)[0]
        got = nearest_neighbourhoods(X, nc.GRAPH_RADIUS, [nc.NS] * case.k, ids, case.m)
        assert list(got) == ids and _as_index_graph(got, ids) == want, label
    # m >= every neighbourhood: today's graph, ids as it returns them (the agent's own a Python int, neighbours NumPy integers)
    if case.k <= 64:
        x0 = nc.scenario(case.k)[0]
        a, b = nearest_neighbourhoods(x0[0][None], nc.GRAPH_RADIUS, [nc.NS] * case.k, ids, 64), define_inter_graph_threshold(
            x0[0][None], nc.GRAPH_RADIUS, [nc.NS] * case.k, ids)
        assert a == b and all([type(j) for j in a[i]] == [type(j) for j in b[i]] for i in ids)


@pytest.mark.parametrize("hand", nc.HAND, ids=nc.HAND_IDS)
def test_hand_made_scenarios(hand):
    from dpilqr_amd.distributed import nearest_neighbourhoods
    k, m = hand["k"], hand["m"]
    graph, dropped, sizes, gap, thr_margin = nc.reference(hand["X"], k, nc.NS, hand["radius"], m)
    got = nearest_neighbourhoods(hand["X"], hand["radius"], [nc.NS] * k, list(range(k)), m)
    assert {i: [int(j) for j in v] for i, v in got.items()} == graph
    assert thr_margin >= nc.MARGIN
    name = hand["name"]
    if name.startswith("ties"):
        key = nc.keys_of(hand["X"], k, nc.NS)
        c, tied = {"ties-k6": (0, [1, 2, 3, 4]), "ties-k70": (0, [63, 64, 65, 66]), "ties-k70-rev": (69, [63, 64, 65, 66])}[name]
        assert all(key[c, j] == 0.5 for j in tied) and gap == 0.0      # exact ties, at the cut
        assert graph[c] == sorted([c] + tied[:2]) and dropped[c] == 2      # the two lowest indices win
    elif name == "later-row":
        assert gap >= nc.MARGIN
        row0 = nc.reference(hand["X"][:1], k, nc.NS, hand["radius"], m)[0]
        assert graph[0] == [0, 2] and row0[0] == [0, 1]      # min over the rows, not row 0
    else:
        assert gap >= nc.MARGIN
        uncapped = nc.reference(hand["X"], k, nc.NS, hand["radius"], 64)[0]
        bitten = [i for i in range(k) if dropped[i] > 0]
        spared = [i for i in range(k) if dropped[i] == 0 and sizes[i] > 1]
        assert len(bitten) == 5 and len(spared) == 2 and all(graph[i] == uncapped[i] for i in range(k) if i not in bitten)


def test_reference_properties():
    """m = 1: every agent alone; m >= every neighbourhood: the uncapped graph (the oracle's own define_inter_graph_threshold)."""
    for k in (6, 65):
        x0, _, X = nc.scenario(k)
        alone, dropped, sizes, _, _ = nc.reference(X[0], k, nc.NS, nc.GRAPH_RADIUS, 1)
        assert alone == {i: [i] for i in range(k)} and (dropped == sizes - 1).all()
        full = nc.reference(X[0], k, nc.NS, nc.GRAPH_RADIUS, k)
        assert full[0] == nc.orc.define_inter_graph_threshold(X[0], nc.GRAPH_RADIUS, k, nc.NS) and not full[1].any()


@pytest.mark.parametrize("case", nc.SOLVE_CASES + [c for c in nc.POLICY_CASES if not c.S_solve], ids=lambda c: c.id)
def test_capped_solves_are_insensitive_to_rounding(case):
    """U0 moved by 1e-12: the oracle's capped X_dec, U_dec and J_full move by less than 1e-9 (relative to the largest entry) --
    the rule of tests/test_swarm_cases.py."""
    ci = nc.CASES.index(case)
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))
    worst = 0.0
    for s in range(case.S_solve or 1):
        X, U, J, g, _ = nc.oracle_solve(ci, s)
        Xp, Up, Jp, _, _ = nc.oracle_solve(ci, s, 1e-12)
        worst = max(worst, rel(Xp, X), rel(Up, U), rel(Jp, J))
        assert max(len(v) for v in g.values()) == case.m
    print(f"\n[nearest conditioning {case.id}] the oracle's capped solve moves by {worst:.3g} under a 1e-12 change of U0 (< 1e-9 asked)")
    assert worst < 1e-9
