"""Separated random scenarios on the device (dpilqr_setup_separate, include/dpilqr_separated_setup.h) against the fixture written from
the real reference (G12, tests/golden/g12_separated_setup.npz: bit for bit, round counts included), against util.separate_locs,
under guard rows and poisoned columns, under the cap, and end to end through the study and the swarm loop."""
from pathlib import Path

import numpy as np
import pytest

from tests import swarm_study_cases as cases

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "g12_separated_setup.npz"
N_WARM = 3      # steps of the warm starts drawn beside a fixture case
# the cap: seven agents in [-3.5, 3.5]^2 held to a separation at which some sets are apart as drawn and some are not
CAP = dict(k=7, n_s=4, n_d=2, var=3.5, rel_dist=1.0, energy=35.0, seeds=range(0, 12))


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib, analysis  # noqa: F401  (dp.analysis)
    _lib.require_gpu()
    return dpilqr_amd


@pytest.fixture(scope="module")
def g12():
    return np.load(GOLD)


def _digest(a):
    v = np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)
    w = np.arange(v.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over="ignore"):
        return np.array([v.sum(dtype=np.uint64), (v * w).sum(dtype=np.uint64)], dtype=np.uint64)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float64).view(np.uint64)


def _groups(g):
    """The fixture's records grouped into launches: consecutive records that differ in the seed only."""
    key = lambda r: tuple(float(g[name][r]) for name in ("k", "n_s", "n_d", "rel_dist", "var", "energy"))
    out = []
    for r in range(len(g["k"])):
        if out and key(out[-1][0]) == key(r) and int(g["seed"][r]) == int(g["seed"][out[-1][-1]]) + 1:
            out[-1].append(r)
        else:
            out.append([r])
    return out


def _host(k, n_s, n_d, var, rel_dist, energy, seed, max_iter=None):
    """One scenario from util.separate_locs chained as random_setup chains it: (x0 row, xf row, [rounds]).  A set the cap stops is
    left as it stands, not normalised."""
    from dpilqr_amd.util import normalize_energy, separate_locs
    np.random.seed(seed)
    rows, rounds = [], []
    for _ in range(2):
        x, r = separate_locs(var * np.random.uniform(-1, 1, (k, n_d)), rel_dist, max_iter)
        row = np.c_[x, np.zeros((k, n_s - n_d))].reshape(-1, 1)
        if energy and r > 0:
            row = normalize_energy(row, [n_s] * k, energy, n_d)
        rows.append(row.ravel()); rounds.append(r)
    return rows[0], rows[1], rounds


# ---- 1. every fixture case, both routes
@pytest.mark.parametrize("gi", range(26))
def test_fixture_cases_bit_for_bit_on_both_routes(dp, g12, gi):
    recs = _groups(g12)[gi]
    r0 = recs[0]
    k, n_s, n_d = (int(g12[name][r0]) for name in ("k", "n_s", "n_d"))
    rel_dist, var, energy = (float(g12[name][r0]) for name in ("rel_dist", "var", "energy"))
    seeds = [int(g12["seed"][r]) for r in recs]
    assert len(seeds) >= 3 and var == k / 2
    x0, xf, rounds = dp.util.random_setup_batch(range(seeds[0], seeds[0] + len(seeds)), k, n_s, var, n_d=n_d, energy=energy or None,
                                                separated=True, rel_dist=rel_dist, return_rounds=True)
    n_u = k * (3 if n_s == 6 else 2)
    t = dp.analysis.trial_inputs_batch(k, n_s, n_u, N_WARM, energy or None, n_d, seeds, separated=True, rel_dist=rel_dist)
    plain = dp.analysis.trial_inputs_batch(k, n_s, n_u, N_WARM, energy or None, n_d, seeds)
    assert rounds.shape == (len(seeds), 2) and np.array_equal(rounds, g12["rounds"][recs])
    for si, r in enumerate(recs):
        for ai, (a, b) in enumerate(((x0, t[0]), (xf, t[1]))):
            assert np.array_equal(_digest(a[si].cpu().numpy()), g12["digest"][r, ai]), (r, ai)
            assert np.array_equal(_bits(a[si]), _bits(b[si])), (r, ai)
            if k <= 8:
                assert np.array_equal(_bits(a[si]), g12[f"{('x0', 'xf')[ai]}_{r}"].view(np.uint64)), (r, ai)
            cols = a[si].cpu().numpy().reshape(k, n_s)[:, n_d:]
            assert np.array_equal(cols.view(np.uint64), np.zeros(cols.shape, dtype=np.uint64))
    # the push draws nothing: the warm starts are those of random=True, and the positions are not
    assert np.array_equal(_bits(t[2]), _bits(plain[2])) and np.array_equal(_bits(t[3]), _bits(plain[3]))
    assert not np.array_equal(_bits(t[0]), _bits(plain[0]))


def test_fixture_groups_are_the_26_launches_above(g12):
    groups = _groups(g12)
    assert len(groups) == 26 and sorted(r for grp in groups for r in grp) == list(range(len(g12["k"])))
    assert {int(g12["k"][grp[0]]) for grp in groups} == {2, 3, 5, 7, 24, 64, 65, 129, 130, 256}


# ---- 2. batch sizes, seeds, rows alone
@pytest.mark.parametrize("S", [1, 2, 3, 37])
def test_batch_sizes_equal_separate_locs_and_the_seed_drawn_alone(dp, S):
    k, n_s, n_d, var, rel_dist, energy, seed0 = 5, 4, 2, 2.5, 5.0, 25.0, 90
    x0, xf, rounds = dp.util.random_setup_batch((seed0, S), k, n_s, var, n_d=n_d, energy=energy, separated=True, rel_dist=rel_dist,
                                                return_rounds=True)
    assert x0.shape == xf.shape == (S, k * n_s) and rounds.shape == (S, 2)
    for s in range(S):
        h0, hf, hr = _host(k, n_s, n_d, var, rel_dist, energy, seed0 + s)
        assert np.array_equal(_bits(x0[s]), h0.view(np.uint64)) and np.array_equal(_bits(xf[s]), hf.view(np.uint64)), s
        assert rounds[s].tolist() == hr, s
    assert rounds.min() >= 1 and rounds.max() >= 3
    for s in sorted({0, S // 2, S - 1}):
        a0, af, ar = dp.util.random_setup_batch(range(seed0 + s, seed0 + s + 1), k, n_s, var, n_d=n_d, energy=energy, separated=True,
                                                rel_dist=rel_dist, return_rounds=True)
        assert np.array_equal(_bits(a0[0]), _bits(x0[s])) and np.array_equal(_bits(af[0]), _bits(xf[s])) and np.array_equal(ar[0], rounds[s])


def test_a_seed_array_and_the_host_study_inputs(dp):
    """Non-consecutive seeds go in as a device array; every array equals analysis.trial_inputs(separated=True) of that seed."""
    k, n_s, n_d, N, energy, seeds = 6, 4, 2, 4, 12.0, [7, 3, 4294967295, 100]
    got = dp.analysis.trial_inputs_batch(k, n_s, 2 * k, N, energy, n_d, seeds, separated=True)
    for si, seed in enumerate(seeds):
        want = dp.analysis.trial_inputs(k, n_s, 2 * k, N, energy, n_d, seed, separated=True)
        for a, w in zip(got, want):
            assert np.array_equal(_bits(a[si]).ravel(), np.ascontiguousarray(w).ravel().view(np.uint64)), seed


# ---- 3. guards
@pytest.mark.parametrize("k,n_s,n_d,S", [(5, 4, 2, 3), (130, 6, 3, 2), (256, 4, 1, 1)])
def test_entry_writes_the_position_columns_of_its_rows_only(dp, k, n_s, n_d, S):
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle
    var, rel_dist, energy, seed0, poison = k / 2, float(min(k, 24)), 5.0 * k, 17, -7.25
    raw = dp.util.random_setup_batch((seed0, S), k, n_s, var, n_d=n_d, energy=None, wide=True)
    bufs = [torch.full((S + 2, k, n_s), poison, dtype=torch.float64, device="cuda") for _ in range(2)]
    for b, r in zip(bufs, raw):
        b[1:S + 1, :, :n_d] = r.reshape(S, k, n_s)[:, :, :n_d]
    counts = torch.full((S + 2, 2), -99, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().dpilqr_setup_separate(S, k, n_s, n_d, rel_dist, energy, 256, ptr(bufs[0][1:]), ptr(bufs[1][1:]), ptr(counts[1:]),
                                                 stream_handle()))
    torch.cuda.synchronize()
    assert bool((counts[0] == -99).all()) and bool((counts[-1] == -99).all())
    for ai, b in enumerate(bufs):
        assert bool((b[0] == poison).all()) and bool((b[-1] == poison).all()) and bool((b[1:S + 1, :, n_d:] == poison).all())
    for s in range(S):
        h0, hf, hr = _host(k, n_s, n_d, var, rel_dist, energy, seed0 + s)
        assert counts[1 + s].tolist() == hr
        for b, h in zip(bufs, (h0, hf)):
            assert np.array_equal(_bits(b[1 + s, :, :n_d]), np.ascontiguousarray(h.reshape(k, n_s)[:, :n_d]).view(np.uint64))


@pytest.mark.parametrize("k,n_s,n_d,energy", [(5, 4, 2, None), (5, 4, 2, 10.0), (65, 6, 3, 130.0), (256, 4, 2, 512.0)])
def test_a_distance_nothing_can_meet_leaves_the_generators_output(dp, k, n_s, n_d, energy):
    """rel_dist < 0: no distance is <= it, every set takes its one round and is normalised as dpilqr_trial_inputs normalises."""
    x0, xf, rounds = dp.util.random_setup_batch((4, 5), k, n_s, k / 2, n_d=n_d, energy=energy, separated=True, rel_dist=-1.0,
                                                return_rounds=True)
    w0, wf = dp.util.random_setup_batch((4, 5), k, n_s, k / 2, n_d=n_d, energy=energy, wide=True)
    assert np.array_equal(_bits(x0), _bits(w0)) and np.array_equal(_bits(xf), _bits(wf)) and (rounds == 1).all()


# ---- 4. the cap
def _cap_reference():
    c = CAP
    free = [_host(c["k"], c["n_s"], c["n_d"], c["var"], c["rel_dist"], c["energy"], s) for s in c["seeds"]]
    capped = [_host(c["k"], c["n_s"], c["n_d"], c["var"], c["rel_dist"], c["energy"], s, max_iter=1) for s in c["seeds"]]
    return free, capped


def test_cap_inputs_mix_sets_of_one_round_with_sets_of_more():
    free, capped = _cap_reference()
    rounds = np.array([f[2] for f in free])
    assert (rounds == 1).any() and (rounds > 1).any() and (rounds[:, 0] != rounds[:, 1]).any()
    assert np.array_equal(np.array([c[2] for c in capped]) == -1, rounds > 1)


def test_cap_stops_the_sets_that_need_more_and_only_those(dp):
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle
    c = CAP
    k, n_s, n_d, seeds = c["k"], c["n_s"], c["n_d"], c["seeds"]
    S = len(seeds)
    free, capped = _cap_reference()
    x0, xf = dp.util.random_setup_batch(seeds, k, n_s, c["var"], n_d=n_d, energy=None, wide=True)
    counts = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().dpilqr_setup_separate(S, k, n_s, n_d, c["rel_dist"], c["energy"], 1, ptr(x0), ptr(xf), ptr(counts), stream_handle()))
    u0, uf, u_rounds = dp.util.random_setup_batch(seeds, k, n_s, c["var"], n_d=n_d, energy=c["energy"], separated=True, rel_dist=c["rel_dist"],
                                                  return_rounds=True)
    counts = counts.cpu().numpy()
    assert np.array_equal(counts, np.array([cp[2] for cp in capped])) and np.array_equal(u_rounds, np.array([f[2] for f in free]))
    for s in range(S):
        for ai, (got, whole) in enumerate(((x0, u0), (xf, uf))):
            # a stopped set: one NumPy round, not normalised; any other: the uncapped launch
            assert np.array_equal(_bits(got[s]), capped[s][ai].view(np.uint64)), (s, ai)
            if counts[s, ai] == 1:
                assert np.array_equal(_bits(got[s]), _bits(whole[s])), (s, ai)
    with pytest.raises(ValueError) as e:
        dp.util.random_setup_batch(seeds, k, n_s, c["var"], n_d=n_d, energy=c["energy"], separated=True, rel_dist=c["rel_dist"], max_iter=1)
    named = {(int(seeds[s]), ("starts", "goals")[w]) for s, w in np.argwhere(counts < 0)}
    for seed in seeds:
        for which in ("starts", "goals"):
            assert (f"seed {seed} ({which})" in str(e.value)) == ((seed, which) in named)


# ---- 5. end to end
def _without_times(row):
    """A CSV row with its wall-clock `times` field (the twelfth) cut out: every other byte must match."""
    import csv
    f = next(csv.reader([row]))
    assert len(f) == 14
    return f[:11] + f[12:]


def test_study_rows_with_device_inputs_equal_the_rows_with_host_inputs(dp):
    """monte_carlo_analysis(separated=True) on three double integrators, one trial: the rows with device_inputs=True are the rows
    with device_inputs=False, field by field as strings -- every field but `times`, which is wall-clock seconds and differs between
    any two runs (tests/test_gpu_analysis.py::_same_rows)."""
    from dpilqr_amd import analysis
    kw = dict(n_trials=1, n_agents_iter=(3,), models=(analysis.DoubleIntDynamics4D,), N=10, separated=True)
    dev, host = [], []
    analysis.monte_carlo_analysis(emit=dev.append, device_inputs=True, **kw)
    analysis.monte_carlo_analysis(emit=host.append, device_inputs=False, **kw)
    assert len(dev) == len(host) >= 4
    assert [_without_times(r) for r in dev] == [_without_times(r) for r in host]


def test_separated_swarm_goes_through_the_wide_loop(dp):
    """65 double integrators, two trials, rel_dist = 65 before normalisation to an energy of 20 per agent (a mean distance of 20
    from the centre, forty interaction radii): the first round's neighbourhoods, the graph of x0 alone, are small, and so are those of
    the planned trajectories.  (At the 300 of tests/swarm_study_cases.LOOP the evenly filled disc of a separated swarm plans into
    a neighbourhood of 26 agents, one more than the uncapped solve serves.)  t_diverge is one round's time, step_size * dt: the loop
    stops after its second round at the latest.  N = 8."""
    import torch
    from dpilqr_amd import analysis
    from dpilqr_amd.distributed import define_inter_graph_threshold
    k, N, energy = 65, 8, 20.0 * 65
    x0, xf, rounds = dp.util.random_setup_batch(range(2), k, 4, k / 2, separated=True, rel_dist=float(k), energy=energy, return_rounds=True)
    assert (rounds >= 2).all()
    ids = [100 + i for i in range(k)]
    for row in x0.cpu().numpy():
        g = define_inter_graph_threshold(row.reshape(1, -1), cases.RADIUS, [4] * k, ids)
        assert max(len(g[i]) for i in ids) <= 16
    prob = analysis.build_problem(cases.model(), k, cases.DT, cases.RADIUS, xf[0].cpu().numpy(), 2)
    rows = []
    res = dp.distributed.solve_rhc_scenarios(prob, x0, N, cases.RADIUS, xf=xf, U0=torch.zeros((2, N, 2 * k), dtype=torch.float64, device="cuda"),
                                             centralized=False, n_d=2, step_size=cases.STEP_SIZE, dist_converge=0.1,
                                             t_diverge=cases.STEP_SIZE * cases.DT, i_trial=[0, 1], rows=rows, wide=True)
    assert len(res) == 2 and all(2 <= len(per) <= 3 for per in rows)      # one or two rounds and the closing row
    for X, U, J, _ in res:
        assert X.shape[1] == 4 * k and U.shape[1] == 2 * k and np.isfinite(X).all() and np.isfinite(U).all() and np.isfinite(J)
