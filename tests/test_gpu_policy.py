"""The closed-loop ensemble rollout (dpilqr_policy_rollout, csrc/policy.hpp) against the CPU reference, per sample.

Cases, reference and bound: tests/policy_cases.py.  Every case runs four ways -- plain, with a disturbance W, with control
limits u_lim, and with Xs / Us not stored -- and every sample's Xs, Us, J, min_sep, goal_dist must agree with the reference
loop (oracle.Problem.step / .cost; the NumPy RK4 of tests/linesearch_cases.py for BikeDynamics5D) within
max(TOL_PASS, SPREAD_FACTOR x the reference's own change under PERTURB-sized perturbations of x0s, K, X, U); a sample whose
own sensitivity exceeds SPREAD_CAP is unchecked, and at most 5 % of a case's samples may be.  Two checks need no reference:
dpilqr_rollout fed the returned controls reproduces Xs and J to 1e-11, and a sample started on the nominal stays on it.

The conditions that keep the cases honest are asserted from the reference alone (test_case_conditions): 10-90 % of the
control entries clamped in the u_lim runs, at least 10 % of the samples of every k >= 2 case inside the radius, the perturbed
starts moving J by at least 1 % on at least half the samples.  Figures: profiles/policy_rollout_sensitivity.txt.

Mutants of csrc/policy.hpp tried by hand, each restored afterwards, and the cases they turned red: see that file's tail."""
import numpy as np
import pytest

from tests import policy_cases as pc
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

B, T = pc.B, pc.T
IDS = [c.id for c in pc.CASES]


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
    """The case's launches, once: the three variants with trajectories, the plain one again without, the nominal start."""
    if case.id not in _RUNS:
        ref = pc.case_ref(case)
        b = ref.batch
        pb = _pb(case, b)
        strides = (pb.desc.Q_bstride, pb.desc.R_bstride, pb.desc.Qf_bstride)
        assert all(s > 0 for s in strides) if case.weights == "per_item" else all(s == 0 for s in strides), strides
        out = {}
        for v in ("plain", "W", "u_lim"):
            W, lim = ref.args(v)
            out[v] = {k_: t.cpu().numpy() for k_, t in pb.policy_rollout(ref.X, ref.U, ref.K, b["x0s"], W=W, u_lim=lim, trajectories=True).items()}
            out[v + "-nostore"] = {k_: t.cpu().numpy() for k_, t in pb.policy_rollout(ref.X, ref.U, ref.K, b["x0s"], W=W, u_lim=lim).items()}
        out["nominal"] = {k_: t.cpu().numpy() for k_, t in pb.policy_rollout(ref.X, ref.U, ref.K, ref.X[:, :1], trajectories=True).items()}
        _RUNS[case.id] = out
    return _RUNS[case.id]


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_case_conditions(case):
    """From the reference alone: the case exercises what it is meant to, and stays inside the unchecked cap."""
    ref = pc.case_ref(case)
    f = ref.figures()
    print(case.id, f)
    assert 0.10 <= f["clamped"] <= 0.90, f
    if case.k >= 2:
        assert f["near"] >= 0.10, f
    assert f["moved"] >= 0.5, f
    assert all(u <= pc.MAX_UNCHECKED for u in f["unchecked"].values()), f


@pytest.mark.parametrize("variant", ["plain", "W", "u_lim"])
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_against_reference(case, variant):
    ref = pc.case_ref(case)
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
    if case.k == 1:
        assert np.isposinf(got["min_sep"]).all()


@pytest.mark.parametrize("variant", ["plain", "W", "u_lim"])
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_not_storing_trajectories_changes_nothing(case, variant):
    runs = gpu_runs(case)
    a, b_ = runs[variant], runs[variant + "-nostore"]
    assert set(b_) == {"J", "min_sep", "goal_dist"}
    for key in b_:
        assert np.array_equal(a[key], b_[key]), key


@pytest.mark.parametrize("variant", ["plain", "u_lim"])
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_open_loop_rollout_reproduces_the_samples(case, variant):
    """Self-consistency through a kernel that already exists: the returned controls, applied open loop from the same starts
    by dpilqr_rollout as B * S items, give the same states and the same cost."""
    ref = pc.case_ref(case)
    b, S = ref.batch, case.S
    got = gpu_runs(case)[variant]
    pb2 = _pb(case, b, repeat=S)
    X2, J2 = pb2.rollout(b["x0s"].reshape(B * S, -1), got["U"].reshape(B * S, T, -1))
    X2, J2 = X2.cpu().numpy(), J2.cpu().numpy()
    Xs, J = got["X"].reshape(B * S, T + 1, -1), got["J"].reshape(-1)
    for q in range(B * S):
        assert relerr(X2[q], Xs[q]) <= pc.TOL_ROLLOUT, (q, relerr(X2[q], Xs[q]))
        assert abs(J2[q] - J[q]) <= pc.TOL_ROLLOUT * abs(J[q]), (q, J2[q], J[q])


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_a_sample_on_the_nominal_stays_on_it(case):
    ref = pc.case_ref(case)
    got = gpu_runs(case)["nominal"]
    for i in range(B):
        assert relerr(got["U"][i, 0], ref.U[i]) <= pc.TOL_ROLLOUT, (i, relerr(got["U"][i, 0], ref.U[i]))
        assert relerr(got["X"][i, 0], ref.X[i]) <= pc.TOL_ROLLOUT, (i, relerr(got["X"][i, 0], ref.X[i]))


def test_solver_closed_loop():
    """ilqrSolver.closed_loop: the public path -- one backward pass at (X, U), then the policy from perturbed starts."""
    import dpilqr_amd as dp
    from dpilqr_amd.util import perturbed_starts
    k, N = 3, 15
    dp._reset_ids()
    x0 = np.array([0.0, 0, 0, 0, 2, 2, 0, 0, -2, 1, 0, 0.0]); xf = np.array([3.0, 3, 0, 0, -1, -1, 0, 0, 1, -2, 0, 0.0])
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(xf[4 * i:4 * i + 4], np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    prob = dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k)))
    sol = dp.ilqrSolver(prob, N)
    X, U, J = sol.solve(x0, verbose=False)
    starts = np.vstack([x0[None], perturbed_starts(x0, [4] * k, 7, var=0.3, seed=5)])
    r = sol.closed_loop(X, U, starts, trajectories=True)
    assert r["J"].shape == (8,) and r["min_sep"].shape == (8,) and r["goal_dist"].shape == (8, k)
    Xr, Jr = sol._rollout(x0, U)
    assert relerr(r["X"][0], Xr) <= 1e-9 and abs(r["J"][0] - Jr) <= 1e-9 * abs(Jr)      # the unperturbed start: the plan itself
    assert np.isfinite(r["J"]).all() and (r["J"][1:] != r["J"][0]).all()
