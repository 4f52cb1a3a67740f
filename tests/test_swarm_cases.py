"""What the oracle alone says about the wide-team cases (tests/swarm_cases.py), without a GPU: the cluster-size tables, that
neighbourhoods do span the words of a multi-word mask and that quirk Q11 has identical ones to merge, and that the distributed
solves are well conditioned -- so that tests/test_gpu_swarm.py can hold every agent of every scenario to TOL_SOLVE."""
import numpy as np
import pytest

from tests import swarm_cases as sw

# cluster size -> agents, members whose neighbourhood spans bit 64, distinct neighbourhoods (scenario 0, offset 0.6)
TABLE = {65: ({1: 63, 2: 2}, 2, 64), 70: ({1: 57, 2: 12, 3: 1}, 12, 65), 130: ({1: 115, 2: 14, 3: 1}, 14, 124)}


@pytest.mark.parametrize("case", sw.SOLVE_CASES, ids=lambda c: c.id)
def test_cluster_tables(case):
    graph = sw.oracle_solve(sw.CASES.index(case), 0)[3]
    sizes, spanning, distinct = sw.cluster_table(graph)
    assert (sizes, spanning, distinct) == TABLE[case.k]
    assert spanning >= 2 and distinct < case.k      # words are crossed; Q11 has identical neighbourhoods to merge
    if case.k > 66:      # the asymmetric triple: agent 10's neighbourhood is shared by neither of its members
        assert graph[10] == [10, 63, case.k - 1] and graph[63] == [10, 63] and graph[case.k - 1] == [10, case.k - 1]


@pytest.mark.parametrize("case", sw.CASES, ids=lambda c: c.id)
def test_every_scenario_crosses_words_and_stays_small(case):
    """All S scenarios (the jittered ones too): at least two neighbourhoods span two words, no cluster comes near 64 agents."""
    x0s, _, _ = sw.scenario(case, sw.OFFSET_SOLVE)
    for s in range(sw.S):
        graph = sw.orc.define_inter_graph_threshold(x0s[s][None], sw.RADIUS, case.k, case.ns)
        sizes, spanning, _ = sw.cluster_table(graph)
        assert spanning >= 2 and max(sizes) <= 6, (s, sizes)
        masks = [sw.mask_of(graph[i]) for i in range(case.k)]
        w = np.array([[(m >> (64 * q)) & (2 ** 64 - 1) for q in range(case.n_words)] for m in masks], dtype=np.uint64)
        assert list(sw.words_to_masks(w.view(np.int64))) == masks      # the word layout the tests read the device's masks with


@pytest.mark.parametrize("case", sw.SOLVE_CASES, ids=lambda c: c.id)
def test_solves_are_insensitive_to_rounding(case):
    """U0 moved by 1e-12: the oracle's X_dec, U_dec and J_full move by less than 1e-9 (relative to the largest entry)."""
    ci = sw.CASES.index(case)
    X, U, J, g = sw.oracle_solve(ci, 0)
    Xp, Up, Jp, gp = sw.oracle_solve(ci, 0, 1e-12)
    assert g == gp
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))
    assert max(rel(Xp, X), rel(Up, U), rel(Jp, J)) < 1e-9, (rel(Xp, X), rel(Up, U), rel(Jp, J))


def test_rollout_offset_puts_pairs_inside_the_radius():
    """At the rollout tests' offset the partners start inside the proximity cost's radius: the pairs across a word boundary pay."""
    for case in sw.CASES:
        x0s, xf, _ = sw.scenario(case, sw.OFFSET_ROLLOUT)
        assert sw.oracle_problem(case, xf).prox_cost(x0s[0]) > 0.0
