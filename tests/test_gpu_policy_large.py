"""The large-cluster closed-loop rollout (dpilqr_policy_rollout_large, csrc/policy_large.hpp) against the CPU reference, per sample.

Cases: tests/policy_large_cases.py; reference, bound and the cap on unchecked samples: tests/policy_cases.py, as
tests/test_gpu_policy.py uses them for dpilqr_policy_rollout.  Every case runs plain, with a disturbance W, with control limits
u_lim, and with Xs / Us not stored; every sample's Xs, Us, J, min_sep, goal_dist must agree with the reference loop within
max(TOL_PASS, SPREAD_FACTOR x the reference's own change under PERTURB-sized perturbations of x0s, K, X, U).  Without a reference:
dpilqr_rollout fed the returned controls reproduces Xs and J to 1e-11; a sample started on the nominal stays on it; a sample's
results do not depend on which other samples share its tiles (alone, and in reversed order: bit-identical); nothing is written past
the outputs; ilqrSolver.closed_loop takes this path for a problem of more than 60 states.

The conditions that keep the cases honest are asserted without a GPU (tests/test_policy_large_host.py: test_case_conditions)."""
import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_large_cases as plc
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

B, T = pc.B, pc.T
IDS = [c.id for c in plc.CASES]
KEYS = ("X", "U", "J", "min_sep", "goal_dist")


def _pb(case, b, repeat=1):
    import dpilqr_amd as dp
    rep = lambda a: np.repeat(a, repeat, axis=0)
    if case.weights == "per_item":
        Q, R, Qf = rep(b["Q"]), rep(b["R"]), rep(b["Qf"])
    else:
        Q, R, Qf = b["Q"], b["R"], b["Qf"]
    return dp.ProblemBatch(b["models"], b["n_dims"], rep(b["xf"]), Q, R, Qf, b["radius"], b["dt"], T)


_RUNS = {}


def gpu_runs(case):
    """The case's launches, once: the three variants with trajectories and without, the nominal start, the first sample alone,
    the samples in reversed order."""
    if case.id not in _RUNS:
        ref = plc.case_ref(case)
        b = ref.batch
        pb = _pb(case, b)
        assert pb.is_large
        host = lambda r: {k_: t.cpu().numpy() for k_, t in r.items()}
        out = {}
        for v in ("plain", "W", "u_lim"):
            W, lim = ref.args(v)
            out[v] = host(pb.policy_rollout_large(ref.X, ref.U, ref.K, b["x0s"], W=W, u_lim=lim, trajectories=True))
            out[v + "-nostore"] = host(pb.policy_rollout_large(ref.X, ref.U, ref.K, b["x0s"], W=W, u_lim=lim))
        out["nominal"] = host(pb.policy_rollout_large(ref.X, ref.U, ref.K, ref.X[:, :1], trajectories=True))
        out["first"] = host(pb.policy_rollout_large(ref.X, ref.U, ref.K, b["x0s"][:, :1], trajectories=True))
        out["reversed"] = host(pb.policy_rollout_large(ref.X, ref.U, ref.K, b["x0s"][:, ::-1], trajectories=True))
        _RUNS[case.id] = out
    return _RUNS[case.id]


@pytest.mark.parametrize("variant", ["plain", "W", "u_lim"])
@pytest.mark.parametrize("case", plc.CASES, ids=IDS)
def test_against_reference(case, variant):
    ref = plc.case_ref(case)
    got = gpu_runs(case)[variant]
    worst, unchecked, failures = 0.0, 0, []
    for i in range(B):
        for s in range(case.S):
            bound = pc.bound_of(ref.spread[variant][i, s])
            if bound is None:
                unchecked += 1
                continue
            g = dict(X=got["X"][i, s], U=got["U"][i, s], J=float(got["J"][i, s]), min_sep=float(got["min_sep"][i, s]),
                     goal_dist=got["goal_dist"][i, s])
            d = pc.difference(g, ref.ref[variant][i][s])
            worst = max(worst, d / bound)
            if not d <= bound:
                failures.append((i, s, d, bound))
    print(f"{case.id} {variant}: worst error / bound {worst:.3g}, unchecked {unchecked} of {B * case.S}")
    assert unchecked <= pc.MAX_UNCHECKED * B * case.S, (unchecked, B * case.S)
    assert not failures, failures[:5]


@pytest.mark.parametrize("variant", ["plain", "W", "u_lim"])
@pytest.mark.parametrize("case", plc.CASES, ids=IDS)
def test_not_storing_trajectories_changes_nothing(case, variant):
    runs = gpu_runs(case)
    a, b_ = runs[variant], runs[variant + "-nostore"]
    assert set(b_) == {"J", "min_sep", "goal_dist"}
    for key in b_:
        assert np.array_equal(a[key], b_[key]), key


@pytest.mark.parametrize("variant", ["plain", "u_lim"])
@pytest.mark.parametrize("case", plc.CASES, ids=IDS)
def test_open_loop_rollout_reproduces_the_samples(case, variant):
    """Self-consistency through a kernel that already exists: the returned controls, applied open loop from the same starts
    by dpilqr_rollout as B * S items, give the same states and the same cost."""
    ref = plc.case_ref(case)
    b, S = ref.batch, case.S
    got = gpu_runs(case)[variant]
    pb2 = _pb(case, b, repeat=S)
    X2, J2 = pb2.rollout(b["x0s"].reshape(B * S, -1), got["U"].reshape(B * S, T, -1))
    X2, J2 = X2.cpu().numpy(), J2.cpu().numpy()
    Xs, J = got["X"].reshape(B * S, T + 1, -1), got["J"].reshape(-1)
    for q in range(B * S):
        assert relerr(X2[q], Xs[q]) <= pc.TOL_ROLLOUT, (q, relerr(X2[q], Xs[q]))
        assert abs(J2[q] - J[q]) <= pc.TOL_ROLLOUT * abs(J[q]), (q, J2[q], J[q])


@pytest.mark.parametrize("case", plc.CASES, ids=IDS)
def test_a_sample_on_the_nominal_stays_on_it(case):
    ref = plc.case_ref(case)
    got = gpu_runs(case)["nominal"]
    for i in range(B):
        assert relerr(got["U"][i, 0], ref.U[i]) <= pc.TOL_ROLLOUT, (i, relerr(got["U"][i, 0], ref.U[i]))
        assert relerr(got["X"][i, 0], ref.X[i]) <= pc.TOL_ROLLOUT, (i, relerr(got["X"][i, 0], ref.X[i]))


@pytest.mark.parametrize("case", plc.CASES, ids=IDS)
def test_a_sample_does_not_depend_on_its_neighbours(case):
    """Alone in its tile, or with every other sample in another column, column tile and workgroup than before: the same bits.
    Catches anything leaking from unused columns, column tiles and sample slots of the matrix-pipe product."""
    runs = gpu_runs(case)
    full, first, rev = runs["plain"], runs["first"], runs["reversed"]
    for key in KEYS:
        assert first[key].shape[1] == 1 and np.array_equal(first[key][:, 0], full[key][:, 0]), key
        assert np.array_equal(rev[key][:, ::-1], full[key]), key


@pytest.mark.parametrize("case", plc.CASES, ids=IDS)
def test_nothing_is_written_past_the_outputs(case):
    """Through the raw entry point, every output a view into a buffer with a stretch of a sentinel before and after it."""
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle, to_dev
    ref = plc.case_ref(case)
    b, S = ref.batch, case.S
    pb = _pb(case, b)
    n, m, k = pb.n_x, pb.n_u, pb.k
    G, SENT = 4096, -7.25
    sizes = dict(X=B * S * (T + 1) * n, U=B * S * T * m, J=B * S, min_sep=B * S, goal_dist=B * S * k)
    bufs = {key: torch.full((G + size + G,), SENT, dtype=torch.float64, device="cuda") for key, size in sizes.items()}
    view = {key: bufs[key][G:G + sizes[key]] for key in sizes}
    Xd, Ud, Kd, x0d = to_dev(ref.X), to_dev(ref.U), to_dev(ref.K), to_dev(b["x0s"])
    _lib.check(_lib.load().dpilqr_policy_rollout_large(pb._d, ptr(Xd), ptr(Ud), ptr(Kd), S, ptr(x0d), None, None, ptr(view["X"]),
                                                       ptr(view["U"]), ptr(view["J"]), ptr(view["min_sep"]), ptr(view["goal_dist"]),
                                                       stream_handle()))
    torch.cuda.synchronize()
    full = gpu_runs(case)["plain"]
    for key, size in sizes.items():
        h = bufs[key].cpu().numpy()
        assert (h[:G] == SENT).all() and (h[G + size:] == SENT).all(), key
        assert np.array_equal(h[G:G + size], full[key].reshape(-1)), key      # ... and the outputs themselves are the wrapper's


def test_solver_closed_loop_on_a_large_problem():
    """ilqrSolver.closed_loop for a problem of more than 60 states: the large-cluster backward pass, then policy_rollout_large."""
    import dpilqr_amd as dp
    from dpilqr_amd.util import perturbed_starts
    k, N = 16, 15
    dp._reset_ids()
    ang = 2.0 * np.pi * np.arange(k) / k
    x0 = np.zeros((k, 4)); xf = np.zeros((k, 4))
    x0[:, 0], x0[:, 1] = 4.0 * np.cos(ang), 4.0 * np.sin(ang)
    xf[:, 0], xf[:, 1] = 3.0 * np.cos(ang + 0.4), 3.0 * np.sin(ang + 0.4)
    x0, xf = x0.reshape(-1), xf.reshape(-1)
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(xf[4 * i:4 * i + 4], np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    prob = dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k)))
    sol = dp.ilqrSolver(prob, N)
    assert sol.n_x == 64 and sol._pb(N).is_large
    X, U, J = sol.solve(x0, verbose=False)
    starts = np.vstack([x0[None], perturbed_starts(x0, [4] * k, 7, var=0.3, seed=5)])
    r = sol.closed_loop(X, U, starts, trajectories=True)
    assert r["J"].shape == (8,) and r["min_sep"].shape == (8,) and r["goal_dist"].shape == (8, k)
    Xr, Jr = sol._rollout(x0, U)
    assert relerr(r["X"][0], Xr) <= 1e-9 and abs(r["J"][0] - Jr) <= 1e-9 * abs(Jr)      # the unperturbed start: the plan itself
    assert np.isfinite(r["J"]).all() and len(set(r["J"].tolist())) == 8      # the perturbed starts: finite and distinct
