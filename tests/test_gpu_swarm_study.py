"""The Monte-Carlo study for swarms of 65-256 agents on the device: the input generator (dpilqr_trial_inputs) against the fixture
written from the real reference (G11, tests/golden/g11_trial_inputs_wide.npz: bit for bit), against the 64-agent generator and
under guard rows; solve_rhc_scenarios(wide=True) and multi_agent_run(branches=(False,), wide=True, device_inputs=True) against
per-trial solve_rhc on the same inputs, under the rules of tests/test_gpu_analysis.py::_same_rows."""
import logging
from pathlib import Path

import numpy as np
import pytest

from tests import swarm_study_cases as cases
from tests.test_gpu_analysis import _Rows, _same_rows
from tests.test_host_logic import _parse_row

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "g11_trial_inputs_wide.npz"


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib, analysis  # noqa: F401  (dp.analysis)
    _lib.require_gpu()
    return dpilqr_amd


@pytest.fixture(scope="module")
def g11():
    return np.load(GOLD)


def _digest(a):
    v = np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)
    w = np.arange(v.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over="ignore"):
        return np.array([v.sum(dtype=np.uint64), (v * w).sum(dtype=np.uint64)], dtype=np.uint64)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float64).view(np.uint64)


# ---- 1. the generator against G11
@pytest.mark.parametrize("ei", [0, 1])
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_generator_equals_the_reference_stream_bit_for_bit(dp, g11, ci, ei):
    """Seeds 0 .. 4 in one call (three workgroups, the last half empty), two warm starts of N = 3 steps: the setup draws cross a
    twist boundary at k = 256 (1536 doubles), the warm starts everywhere; with the energy, the pairwise sum takes its split path."""
    k, n_s, n_d = (int(v) for v in g11["cases"][ci])
    N, energy, seeds = int(g11["N"]), float(g11["energies"][ci, ei]), [int(s) for s in g11["seeds"]]
    assert float(g11["warm_scale"]) == 0.01 and (energy == 10.0 * k / 5 if ei == 0 else energy == 0.0)
    n_u = k * (3 if n_s == 6 else 2)
    out = [a.cpu().numpy() for a in dp.analysis.trial_inputs_batch(k, n_s, n_u, N, energy or None, n_d, seeds)]
    assert out[0].shape == out[1].shape == (5, k * n_s) and out[2].shape == out[3].shape == (5, N, n_u)
    for si in range(len(seeds)):
        for ai in range(4):
            assert np.array_equal(_digest(out[ai][si]), g11["digest"][ci, ei, si, ai]), (k, energy, seeds[si], ai)
    si = seeds.index(int(g11["full_seed"]))
    for ai, name in enumerate(("x0", "xf")):
        got = out[ai][si].reshape(k, n_s)
        assert np.array_equal(_bits(got[:, :n_d]), _bits(g11[f"full_{name}_{k}_{ei}"])), (name, k)
        assert np.array_equal(_bits(got[:, n_d:]), np.zeros((k, n_s - n_d), dtype=np.uint64))


# ---- 2. ... against the 64-agent generator and the host stream
@pytest.mark.parametrize("k,n_s,n_d", [(1, 4, 2), (5, 4, 2), (5, 6, 3), (64, 4, 2), (64, 6, 3)])
def test_generator_equals_the_one_thread_generator_where_both_serve(dp, k, n_s, n_d):
    import torch
    for energy in (None, 10.0 * k / 5):
        old = dp.util.random_setup_batch(range(3, 10), k, n_s, k / 2, n_d=n_d, energy=energy)
        new = dp.util.random_setup_batch(range(3, 10), k, n_s, k / 2, n_d=n_d, energy=energy, wide=True)
        # (bit patterns: one agent normalised to an energy is 0 / 0 in both, and a NaN equals nothing)
        assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(old, new)), (k, energy)


def test_generator_takes_the_largest_seed_and_a_seed_array(dp, g11):
    k, n_s, n_d = (int(v) for v in g11["small_case"])
    seeds, energy, N = [int(s) for s in g11["small_seeds"]], float(g11["small_energy"]), int(g11["N"])
    assert max(seeds) == 2 ** 32 - 1 and any(b != a + 1 for a, b in zip(seeds, seeds[1:]))
    want = [g11["small_x0"], g11["small_xf"], g11["small_Ua"], g11["small_Ub"]]
    got = dp.analysis.trial_inputs_batch(k, n_s, 2 * k, N, energy, n_d, seeds)                    # a device array of seeds
    for a, w in zip(got, want):
        assert np.array_equal(_bits(a), _bits(w))
    top = seeds.index(2 ** 32 - 1)
    alone = dp.analysis.trial_inputs_batch(k, n_s, 2 * k, N, energy, n_d, [2 ** 32 - 1])         # ... and as seed0
    for a, w in zip(alone, want):
        assert np.array_equal(_bits(a)[0], _bits(w)[top])
    # the stream is the host's own: analysis.trial_inputs on the installed NumPy draws the fixture's values
    host = dp.analysis.trial_inputs(k, n_s, 2 * k, N, energy, n_d, seeds[1])
    for a, w in zip(host, want):
        assert np.array_equal(_bits(np.asarray(a).reshape(w[1].shape)), _bits(w[1]))


# ---- 3. guards
@pytest.mark.parametrize("S", [1, 7])
def test_generator_writes_its_rows_only(dp, S):
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle
    k, n_s, n_d, N = 65, 4, 2, 3
    n_u, poison = 2 * k, -7.25
    bufs = [torch.full((S + 2, w), poison, dtype=torch.float64, device="cuda") for w in (k * n_s, k * n_s, N * n_u, N * n_u)]
    row1 = [b[1:] for b in bufs]      # a view from the second row on: contiguous
    _lib.check(_lib.load().dpilqr_trial_inputs(S, 11, None, k, n_s, n_d, k / 2, 13.0 * k, 2, N, n_u, 0.01, *(ptr(r) for r in row1),
                                               stream_handle()))
    torch.cuda.synchronize()
    want = dp.analysis.trial_inputs_batch(k, n_s, n_u, N, 13.0 * k, n_d, range(11, 11 + S))
    for b, w in zip(bufs, want):
        assert bool((b[0] == poison).all()) and bool((b[-1] == poison).all())
        assert torch.equal(b[1:S + 1], w.reshape(S, -1))
    # one warm start: the second buffer is not required and not touched
    bufs = [torch.full((S + 2, w), poison, dtype=torch.float64, device="cuda") for w in (k * n_s, k * n_s, N * n_u, N * n_u)]
    _lib.check(_lib.load().dpilqr_trial_inputs(S, 11, None, k, n_s, n_d, k / 2, 13.0 * k, 1, N, n_u, 0.01, ptr(bufs[0][1:]), ptr(bufs[1][1:]),
                                               ptr(bufs[2][1:]), None, stream_handle()))
    torch.cuda.synchronize()
    assert bool((bufs[3] == poison).all())
    for b, w in zip(bufs[:3], want[:3]):
        assert bool((b[0] == poison).all()) and bool((b[-1] == poison).all()) and torch.equal(b[1:S + 1], w.reshape(S, -1))


# ---- 4 - 6. the loop and the study against per-trial solve_rhc
def _per_trial(dp, k, N, energy, trials, t_diverge, max_cluster=None):
    """solve_rhc(centralized=False) trial by trial on the study's stream: after random_setup the centralized branch's warm start is
    drawn and dropped, solve_rhc draws its own -- the second.  Returns the logged rows and [(X, U, J)]."""
    from dpilqr_amd import analysis
    model = cases.model()
    log = logging.getLogger(); old = log.level; log.setLevel(logging.INFO)
    h = _Rows(); log.addHandler(h)
    out = []
    extra = {} if max_cluster is None else {"max_cluster": max_cluster}
    try:
        for i in trials:
            np.random.seed(analysis.seed_of(model, k, i))
            x0, xf = dp.random_setup(k, 4, is_rotation=False, rel_dist=k, var=k / 2, n_d=2, random=True, energy=energy)
            np.random.rand(N, 2 * k)
            prob = analysis.build_problem(model, k, cases.DT, cases.RADIUS, xf, 2)
            out.append(dp.solve_rhc(prob, x0, N, cases.RADIUS, centralized=False, n_d=2, step_size=cases.STEP_SIZE, i_trial=i,
                                    dist_converge=0.1, t_diverge=t_diverge, **extra))
    finally:
        log.removeHandler(h); log.setLevel(old)
    return h.rows, out


def _same_trajectories(mine, ref):
    for (X, U, J, _), (Xr, Ur, Jr) in zip(mine, ref):
        assert X.shape == Xr.shape and np.max(np.abs(X - Xr)) <= 1e-5 * np.max(np.abs(Xr))
        assert U.shape == Ur.shape and np.max(np.abs(U - Ur)) <= 1e-5 * np.max(np.abs(Ur))
        assert abs(J - Jr) <= 1e-6 * abs(Jr)


@pytest.mark.parametrize("dense", [False, True])
def test_wide_loop_on_a_swarm_equals_per_trial_solve_rhc(dp, dense):
    from dpilqr_amd import analysis
    L = cases.LOOP
    k, N, trials = L["k"], L["N"], list(L["trials"])
    energy, cap = (L["energy_dense"], L["max_cluster"]) if dense else (L["energy_sparse"], None)
    x0, xf, _, U_d = cases.inputs(k, N, energy, trials)
    prob = analysis.build_problem(cases.model(), k, cases.DT, cases.RADIUS, xf[0], 2)
    rows = []
    res = dp.distributed.solve_rhc_scenarios(prob, np.stack(x0), N, cases.RADIUS, xf=np.stack(xf), U0=np.stack(U_d), centralized=False,
                                             n_d=2, step_size=cases.STEP_SIZE, dist_converge=0.1, t_diverge=cases.T_DIVERGE_FOUR_ROUNDS,
                                             i_trial=trials, rows=rows, wide=True, max_cluster=cap)
    ref_rows, ref = _per_trial(dp, k, N, energy, trials, cases.T_DIVERGE_FOUR_ROUNDS, cap)
    got = [r for per in rows for r in per]
    assert all(2 <= len(per) <= 5 for per in rows)      # at most four rounds and the closing row
    _same_rows(got, ref_rows)
    _same_trajectories(res, ref)
    sizes = [len(g) for r in got for g in _parse_row(r)["subgraphs"]]
    first = [len(g) for per in rows for g in _parse_row(per[0])["subgraphs"]]      # the first round's graph: x0 alone
    if dense:
        assert max(sizes) == cap      # the cap bites, and no entry exceeds it in any round
    else:
        assert 1 <= min(first) and max(first) <= 8 and max(first) >= 2 and max(sizes) <= 64


def test_wide_route_equals_the_default_route_on_a_small_team(dp):
    """k = 5, two trials: the arrays bit for bit, the rows string-equal but for `times`; the distributed-only study emits exactly
    the two-branch study's distributed rows; inputs drawn on the device give the rows of inputs drawn on the host."""
    from dpilqr_amd import analysis
    model, k, N, trials, t_div = cases.model(), 5, 10, [0, 1], cases.T_DIVERGE_FOUR_ROUNDS
    drawn = [analysis.trial_inputs(k, 4, 2 * k, N, 10.0, 2, analysis.seed_of(model, k, i)) for i in trials]
    x0, xf, U_d = np.stack([d[0].ravel() for d in drawn]), np.stack([d[1].ravel() for d in drawn]), np.stack([d[3] for d in drawn])
    prob = analysis.build_problem(model, k, cases.DT, cases.RADIUS, xf[0], 2)
    kw = dict(xf=xf, U0=U_d, centralized=False, n_d=2, step_size=cases.STEP_SIZE, dist_converge=0.1, t_diverge=t_div, i_trial=trials)
    rows_a, rows_b = [], []
    a = dp.distributed.solve_rhc_scenarios(prob, x0, N, cases.RADIUS, rows=rows_a, **kw)
    b = dp.distributed.solve_rhc_scenarios(prob, x0, N, cases.RADIUS, rows=rows_b, wide=True, **kw)
    for (Xa, Ua, Ja, ca), (Xb, Ub, Jb, cb) in zip(a, b):
        assert np.array_equal(_bits(Xa), _bits(Xb)) and np.array_equal(_bits(Ua), _bits(Ub)) and Ja == Jb and ca == cb

    def no_times(row):
        f = _parse_row(row)
        assert len(f["times"]) == k
        return {key: repr(v) for key, v in f.items() if key != "times"}

    flat_a, flat_b = [r for per in rows_a for r in per], [r for per in rows_b for r in per]
    assert len(flat_a) == len(flat_b) and [no_times(r) for r in flat_a] == [no_times(r) for r in flat_b]

    run = lambda **extra: (lambda got: (got, analysis.multi_agent_run(model, [4] * k, cases.DT, N, cases.RADIUS, trials=trials, emit=got.append,
                                                                      dist_converge=0.1, t_diverge=t_div, **extra)))([])
    both, res_both = run()
    only, res_only = run(branches=(False,))
    dev, _ = run(branches=(False,), device_inputs=True)
    wide_dev, _ = run(branches=(False,), device_inputs=True, wide=True)
    dist_rows = [r for r in both if not _parse_row(r)["centralized"]]
    assert 0 < len(dist_rows) < len(both)
    for other in (only, dev, wide_dev):
        assert len(other) == len(dist_rows) and [no_times(r) for r in other] == [no_times(r) for r in dist_rows]
    for i in trials:
        assert len(res_only[i]) == 1 and np.array_equal(_bits(res_only[i][0][0]), _bits(res_both[i][1][0]))


def test_study_of_a_two_word_swarm_equals_per_trial_solve_rhc(dp):
    from dpilqr_amd import analysis
    S = cases.STUDY
    k, N, trials = S["k"], S["N"], list(S["trials"])
    got = []
    res = analysis.multi_agent_run(cases.model(), [4] * k, cases.DT, N, cases.RADIUS, energy=S["energy"], trials=trials, emit=got.append,
                                   branches=(False,), wide=True, device_inputs=True, max_cluster=S["max_cluster"], dist_converge=0.1,
                                   t_diverge=cases.T_DIVERGE_TWO_ROUNDS)
    ref_rows, ref = _per_trial(dp, k, N, S["energy"], trials, cases.T_DIVERGE_TWO_ROUNDS, S["max_cluster"])
    assert len(got) == 3 * len(trials)      # two rounds and the closing row per trial
    _same_rows(got, ref_rows)
    _same_trajectories([res[i][0] for i in trials], ref)
    sizes = [len(g) for r in got for g in _parse_row(r)["subgraphs"]]
    assert max(sizes) == S["max_cluster"]
    assert any(m >= 164 for r in got for g in _parse_row(r)["subgraphs"] for m in g)      # members of the second mask word
