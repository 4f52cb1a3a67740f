"""What tests/test_gpu_linesearch.py takes for granted, checked without a GPU: its cases cover every line-search instantiation the
launchers' sources name, and the Python statements of the launchers' size rules (tests/linesearch_cases.py) agree with the C++
ones, which a small host program compiled from forward.hpp and riccati_big.hpp prints (tests/linesearch_sizes.cpp)."""
import os
import subprocess

import pytest

from tests import linesearch_cases as lc

ROOT = lc.CSRC.parent.parent
FAMILIES = [(3, 2), (4, 2), (5, 2), (6, 3), (12, 4)]


@pytest.fixture(scope="module")
def sizes(tmp_path_factory):
    """{(ns, nc, k): (on_pipe, staged forward LDS, large-cluster forward LDS, large-cluster sweep LDS, kMaxStage, kMaxLds)} at ten
    candidates, from the headers themselves."""
    exe = tmp_path_factory.mktemp("ls") / "sizes"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O0", "-Iinclude", "-Idpilqr_amd/csrc", "-o", str(exe),
                    "tests/linesearch_sizes.cpp"], cwd=ROOT, check=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        v = [int(t) for t in line.split()]
        out[tuple(v[:3])] = tuple(v[3:])
    return out


def test_size_rules_agree_with_the_headers(sizes):
    assert sorted({(ns, nc) for ns, nc, _ in sizes}) == FAMILIES == sorted(set(lc.MODEL_DIMS.values()))
    for (ns, nc, k), (pipe, staged, fwd, big, max_stage, max_lds) in sizes.items():
        n, m = k * ns, k * nc
        assert (max_stage, max_lds) == (lc.K_MAX_STAGE, lc.K_MAX_LDS)
        assert lc.forward_on_pipe(n, m, k) == bool(pipe), (ns, k)
        assert lc.forward_lds_bytes(n, m, k, 10, False) == staged and lc.forward_lds_bytes(n, m, k, 10, True) == fwd, (ns, k)
        assert lc.big_sweep_lds_bytes(k, ns, nc) == big, (ns, k)


def test_no_served_cluster_leaves_the_matrix_pipe(sizes):
    """k_forward<..., KDIRECT, PIPE = false> cannot be launched in line-search mode: at the solve loop's ten candidates every
    cluster of at most 25 agents (256 threads) that takes the large-cluster k_forward and whose line search and sweep fit kMaxLds
    satisfies forward_on_pipe.  The one size that fails the predicate, twenty-four twelve-state agents, is refused by the
    library (its sweep needs 179 360 B of LDS).  The other form serves rollouts only."""
    off = [(ns, k) for (ns, nc, k), v in sizes.items() if not v[0] and k * ns > 60]
    assert off == [(12, 24)]
    assert max(sizes[(12, 4, 24)][2:4]) > lc.K_MAX_LDS


def test_every_instantiation_has_a_case():
    """The tables are read from tu_forward.hip / tu_lsteam.hip; a case counts for an instantiation only where launch_forward's
    every branch, in its order, sends the case's launch to it."""
    cases = lc.all_cases()
    assert all(c.expected_route() == c.route for c in cases)
    launched = {(c.route, c.models[0], c.k) for c in cases if c.uniform}
    assert len(lc.WAVE_TABLE) == 74 and len(lc.TEAM_TABLE) == 30
    assert not [key for key in lc.WAVE_TABLE if ("wave",) + key not in launched]
    assert not [key for key in lc.TEAM_TABLE if ("team",) + key not in launched]
    # no dead entries: an instantiation a launch can never reach (as k_linesearch_wave<kQuadcopter12D, 5> was: K[t] is beyond
    # kMaxStage elements per thread, the large-cluster k_forward takes the launch first) must not be in the table
    for m, k in lc.WAVE_TABLE | lc.TEAM_TABLE:
        assert not lc.Case("wave", [m] * k, 2000, 1).leaves_staged_forward(), (m, k)
    routes = {c.route for c in cases}
    assert routes == {"wave", "team", "generic", "big"}
    assert any(c.route == "big" and not c.k * lc.MODEL_DIMS[c.models[0]][0] > 60 for c in cases)      # the kMaxStage clause
