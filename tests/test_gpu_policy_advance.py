"""The receding-horizon advance (dpilqr_policy_advance / _dec, csrc/policy_advance.hpp) and the loop built on it
(solve_rhc_closed_loop).

Cases: tests/policy_cases.py and tests/policy_dec_cases.py, every (item, sample) one scenario with the item's plan repeated
(tests/policy_advance_cases.py).  The executed prefix is held bit for bit to the rollout kernel it restates
(ProblemBatch.policy_rollout / policy_rollout_dec with trajectories), the executed cost, the separation and the distance left
to the CPU reference's prefix within policy_cases.bound_of of the sample's own sensitivity, the shift to its NumPy definition;
two calls equal one, the capacity holds, and solve_rhc_closed_loop equals a loop written here from the public pieces that
existed before it."""
import numpy as np
import pytest

from tests import policy_advance_cases as ac
from tests import policy_cases as pc
from tests import policy_dec_cases as dc
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

B, T = pc.B, pc.T
IDS = [c.id for c in pc.CASES]
VARIANTS = ("plain", "W", "u_lim")


def _host(d):
    return {k_: t.cpu().numpy() for k_, t in d.items()}


def _nan_state(pb, n_state, L, scen, x0):
    """A state whose every buffer is NaN (n_done zero) but for the named scenarios' plant states and their executed cost so
    far, zero: what an advance does not write stays NaN."""
    st = pb.advance_state(np.zeros((n_state, pb.n_x)), L)
    for f, t in st.items():
        if f != "n_done":
            t.fill_(float("nan"))
    x_cur, J = np.full((n_state, pb.n_x), np.nan), np.full(n_state, np.nan)
    x_cur[scen], J[scen] = x0, 0.0
    st["x_cur"].copy_(st["x_cur"].new_tensor(x_cur)); st["J_exec"].copy_(st["J_exec"].new_tensor(J))
    return st


def _state_W(W, scen, n_state, L):
    """W (items, T, n_x) of the cases as the state's (scenarios, L, n_x), NaN where no item reads."""
    out = np.full((n_state, L, W.shape[2]), np.nan)
    out[scen] = W[:, :L]
    return out


_SETUP, _ROLL, _ADV = {}, {}, {}


def setup(case):
    if case.id not in _SETUP:
        ref = pc.case_ref(case)
        rp = ac.repeated(case, ref)
        _SETUP[case.id] = (ref, rp, ac.problem_batch(case, ref.batch, repeat=case.S), ac.scen_of(case, rp["n"]))
    return _SETUP[case.id]


def rollout(case, variant):
    """The kernel the advance restates, once per variant: policy_rollout on the case's own batch, every sample's trajectory."""
    if (case.id, variant) not in _ROLL:
        ref = pc.case_ref(case)
        W, lim = ref.args(variant)
        r = _host(ac.problem_batch(case, ref.batch).policy_rollout(ref.X, ref.U, ref.K, ref.batch["x0s"], W=W, u_lim=lim, trajectories=True))
        _ROLL[(case.id, variant)] = {k_: v.reshape((B * case.S,) + v.shape[2:]) for k_, v in r.items()}
    return _ROLL[(case.id, variant)]


def advance(case, variant, h, L=None, gains=True):
    """One advance launch of all B * S scenarios through a non-identity scen into a NaN-filled state with spare scenarios."""
    key = (case.id, variant, h, L, gains)
    if key not in _ADV:
        ref, rp, pb, scen = setup(case)
        L = T if L is None else L
        n_state = rp["n"] + ac.SPARE
        _, lim = ref.args(variant)
        st = _nan_state(pb, n_state, L, scen, rp["x0"])
        W = _state_W(rp["W"], scen, n_state, L) if variant == "W" else None
        pb.policy_advance(rp["X"], rp["U"], rp["K"] if gains else None, h, st, scen=scen, W=W, u_lim=lim, n_d=ac.N_D)
        _ADV[key] = _host(st)
    return _ADV[key]


def _unnamed(scen, n_state):
    return np.setdiff1d(np.arange(n_state), scen)


# ------------------------------------------------------------------------------------ 1. bit-equal to the rollout it restates
@pytest.mark.parametrize("h", ac.HS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_executed_prefix_is_the_rollouts(case, variant, h):
    ref, rp, pb, scen = setup(case)
    roll, st = rollout(case, variant), advance(case, variant, h)
    assert np.array_equal(st["X_exec"][scen, :h + 1], roll["X"][:, :h + 1])
    assert np.array_equal(st["U_exec"][scen, :h], roll["U"][:, :h])
    assert np.array_equal(st["x_cur"][scen], roll["X"][:, h])
    assert (st["n_done"][scen] == h).all()
    assert np.isnan(st["X_exec"][scen, h + 1:]).all() and np.isnan(st["U_exec"][scen, h:]).all()      # nothing past the executed steps
    rest = _unnamed(scen, rp["n"] + ac.SPARE)
    assert len(rest) == ac.SPARE and (st["n_done"][rest] == 0).all()
    for f in ("x_cur", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left", "U_next", "X_next"):
        assert np.isnan(st[f][rest]).all(), f      # scenarios not named keep their NaN


# ------------------------------------------------------------------------------------ 2. against the CPU reference, per scenario
@pytest.mark.parametrize("h", ac.HS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_cost_separation_and_distance_against_the_reference(case, variant, h):
    ref, rp, pb, scen = setup(case)
    st = advance(case, variant, h)
    worst, unchecked, failures = 0.0, 0, []
    for i in range(B):
        for s in range(case.S):
            q = scen[i * case.S + s]
            bound = pc.bound_of(ref.spread[variant][i, s])
            if bound is None:
                unchecked += 1
                continue
            J, sep, left = ac.prefix(case, ref, variant, i, s, h)
            d = max(abs(st["J_exec"][q] - J) / max(abs(J), 1e-300), relerr(st["dist_left"][q], left))
            if np.isinf(sep) or np.isinf(st["min_sep"][q]):
                d = d if st["min_sep"][q] == sep else np.inf
            else:
                d = max(d, abs(st["min_sep"][q] - sep) / max(abs(sep), 1e-300))
            worst = max(worst, d / bound)
            if not d <= bound:
                failures.append((i, s, d, bound))
    print(f"{case.id} {variant} h={h}: worst error / bound {worst:.3g}, unchecked {unchecked} of {B * case.S}")
    assert unchecked <= pc.MAX_UNCHECKED * B * case.S, (unchecked, B * case.S)
    assert not failures, failures[:5]
    if case.k == 1:
        assert np.isposinf(st["min_sep"][scen]).all()
    # ... and J_exec against the cost kernel at the executed points
    c = pb.cost(st["X_exec"][scen, :h], st["U_exec"][scen, :h]).cpu().numpy().sum(axis=1)
    assert np.all(np.abs(st["J_exec"][scen] - c) <= pc.TOL_ROLLOUT * np.abs(c)), np.max(np.abs(st["J_exec"][scen] - c) / np.abs(c))


# ------------------------------------------------------------------------------------ 3. the shift
@pytest.mark.parametrize("h", (1, 3, T))
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_the_shift_is_its_definition(case, h):
    ref, rp, pb, scen = setup(case)
    st = advance(case, "u_lim", h)
    for j in range(rp["n"]):
        Un, Xn = ac.shift(rp["X"][j], rp["U"][j], st["x_cur"][scen[j]], h)
        assert np.array_equal(st["U_next"][scen[j]], Un) and np.array_equal(st["X_next"][scen[j]], Xn), j
    if h == T:
        assert (st["U_next"][scen] == 0.0).all()
        assert np.array_equal(st["X_next"][scen, 0], st["x_cur"][scen])
        assert np.array_equal(st["X_next"][scen, 1:], np.repeat(rp["X"][:, T:T + 1], T, axis=1))


# ------------------------------------------------------------------------------------ 4. two calls equal one
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_two_calls_equal_one(case):
    """h = 1, then h = 2 on the plan sliced from step 1 (padded on the host), W read at the global step, under limits too,
    against one call of h = 3: the offsets n_done gives into W and the executed buffers, one addition per step into J_exec."""
    ref, rp, pb, scen = setup(case)
    n_state, L = rp["n"] + ac.SPARE, 5
    W = _state_W(rp["W"], scen, n_state, L)
    fresh = lambda: _nan_state(pb, n_state, L, scen, rp["x0"])

    one = _host(pb.policy_advance(rp["X"], rp["U"], rp["K"], 3, fresh(), scen=scen, W=W, u_lim=ref.u_lim, n_d=ac.N_D))
    st = fresh()
    pb.policy_advance(rp["X"], rp["U"], rp["K"], 1, st, scen=scen, W=W, u_lim=ref.u_lim, n_d=ac.N_D)
    pad = lambda a, last: np.concatenate([a[:, 1:], last], axis=1)
    X2, U2, K2 = pad(rp["X"], rp["X"][:, -1:]), pad(rp["U"], np.zeros_like(rp["U"][:, :1])), pad(rp["K"], np.zeros_like(rp["K"][:, :1]))
    two = _host(pb.policy_advance(X2, U2, K2, 2, st, scen=scen, W=W, u_lim=ref.u_lim, n_d=ac.N_D))
    for f in ("X_exec", "U_exec", "J_exec", "min_sep", "n_done", "x_cur", "dist_left"):
        assert np.array_equal(one[f][scen], two[f][scen], equal_nan=True), f      # (NaN: the rows past the three executed steps)
    assert (two["n_done"][scen] == 3).all() and np.isfinite(two["J_exec"][scen]).all()


# ------------------------------------------------------------------------------------ 5. the capacity
@pytest.mark.parametrize("case", [pc.CASES[1], pc.CASES[3]], ids=[IDS[1], IDS[3]])
def test_the_capacity_is_never_passed(case):
    import torch
    ref, rp, pb, scen = setup(case)
    n_state, L = rp["n"] + ac.SPARE, 4
    st = _nan_state(pb, n_state, L, scen, rp["x0"])
    st["n_done"].copy_(torch.full((n_state,), L - 1, dtype=torch.int32))
    st["min_sep"].fill_(float("inf"))
    Wn = np.full((n_state, L, pb.n_x), np.nan); Wn[scen, L - 1] = rp["W"][:, 0]
    got = _host(pb.policy_advance(rp["X"], rp["U"], rp["K"], 3, st, scen=scen, W=Wn, n_d=ac.N_D))
    roll = rollout(case, "W")      # one step from the same starts under the same disturbance
    assert (got["n_done"][scen] == L).all() and (got["n_done"][_unnamed(scen, n_state)] == L - 1).all()
    assert np.array_equal(got["X_exec"][scen, L - 1:], roll["X"][:, :2]) and np.array_equal(got["U_exec"][scen, L - 1], roll["U"][:, 0])
    assert np.isnan(got["X_exec"][scen, :L - 1]).all() and np.isnan(got["U_exec"][scen, :L - 1]).all()
    rest = _unnamed(scen, n_state)      # among them the scenarios that follow a named one in memory
    assert np.isnan(got["X_exec"][rest]).all() and np.isnan(got["U_exec"][rest]).all() and np.isnan(got["X_next"][rest]).all()
    for j in (0, rp["n"] - 1):
        Un, Xn = ac.shift(rp["X"][j], rp["U"][j], got["x_cur"][scen[j]], 1)      # the shift follows the executed step
        assert np.array_equal(got["U_next"][scen[j]], Un) and np.array_equal(got["X_next"][scen[j]], Xn)
    # a full scenario executes nothing more
    again = _host(pb.policy_advance(rp["X"], rp["U"], rp["K"], 2, st, scen=scen, W=Wn, n_d=ac.N_D))
    for f in ("X_exec", "U_exec", "J_exec", "min_sep", "n_done", "x_cur"):
        assert np.array_equal(again[f][scen], got[f][scen], equal_nan=True), f


# ------------------------------------------------------------------------------------ 6. K = NULL
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_without_gains_the_plan_is_executed_open_loop(case):
    ref, rp, pb, scen = setup(case)
    lim = ref.u_lim
    st = advance(case, "u_lim", T, gains=False)
    want = np.where(rp["U"] < lim[0], lim[0], np.where(rp["U"] > lim[1], lim[1], rp["U"]))
    assert np.array_equal(st["U_exec"][scen], want)
    free = advance(case, "plain", T, gains=False)
    assert np.array_equal(free["U_exec"][scen], rp["U"])
    Xr, Jr = pb.rollout(rp["x0"], rp["U"])
    Xr = Xr.cpu().numpy()
    for j in range(rp["n"]):
        assert relerr(free["X_exec"][scen[j]], Xr[j]) <= pc.TOL_ROLLOUT, (j, relerr(free["X_exec"][scen[j]], Xr[j]))


# ------------------------------------------------------------------------------------ 7. the dec form
def _advance_dec(pb, rp_X, rp_U, Kc, masks, scen, x0, W, lim, h, n_state):
    st = _nan_state(pb, n_state, T, scen, x0)
    return _host(pb.policy_advance_dec(rp_X, rp_U, Kc, masks, h, st, scen=scen, W=W, u_lim=lim, n_d=ac.N_D))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_dec_with_full_masks_is_the_dense_advance(case, variant):
    ref, rp, pb, scen = setup(case)
    k, n = case.k, rp["n"]
    masks = np.full((n, k), (1 << k) - 1, dtype=np.uint64)
    Kc = rp["K"].reshape(n, T, k, case.nc, k * case.ns)      # agent a's rows, every agent's columns in order: the dense K regrouped
    _, lim = ref.args(variant)
    W = _state_W(rp["W"], scen, n + ac.SPARE, T) if variant == "W" else None
    dec, dense = _advance_dec(pb, rp["X"], rp["U"], Kc, masks, scen, rp["x0"], W, lim, 3, n + ac.SPARE), advance(case, variant, 3)
    for f in dense:
        assert np.array_equal(dec[f], dense[f], equal_nan=True), f


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_dec_prefix_is_the_dec_rollouts(case, variant):
    ref = dc.case_ref(case)
    b, S, ns, nc = ref.batch, case.S, case.ns, case.nc
    W, lim = ref.args(variant)
    kc_max = ref.true_kc_max(range(B))
    Kc = dc.compact_gains(ref.K, ref.masks, ns, nc, kc_max)      # NaN past every neighbourhood
    roll = _host(ac.problem_batch(case, b).policy_rollout_dec(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
    rep = lambda a: np.repeat(a, S, axis=0)
    n = B * S
    scen = ac.scen_of(case, n)
    pb = ac.problem_batch(case, b, repeat=S)
    Ws = _state_W(b["W"].reshape(n, T, -1), scen, n + ac.SPARE, T) if variant == "W" else None
    x0 = b["x0s"].reshape(n, -1)
    for h in ac.HS:
        got = _advance_dec(pb, rep(ref.X), rep(ref.U), rep(Kc), rep(ref.masks), scen, x0, Ws, lim, h, n + ac.SPARE)
        assert np.array_equal(got["X_exec"][scen, :h + 1], roll["X"].reshape(n, T + 1, -1)[:, :h + 1])
        assert np.array_equal(got["U_exec"][scen, :h], roll["U"].reshape(n, T, -1)[:, :h])
        assert (got["n_done"][scen] == h).all() and np.isfinite(got["J_exec"][scen]).all()
    zero = _advance_dec(pb, rep(ref.X), rep(ref.U), rep(dc.compact_gains(ref.K, ref.masks, ns, nc, kc_max, fill=0.0)), rep(ref.masks), scen,
                        x0, Ws, lim, ac.HS[-1], n + ac.SPARE)
    for f in got:
        assert np.array_equal(got[f], zero[f], equal_nan=True), f      # what lies past a neighbourhood's columns is never read
    # no gains: the nominal alone, whatever the masks
    open_ = _advance_dec(pb, rep(ref.X), rep(ref.U), None, None, scen, x0, None, None, 2, n + ac.SPARE)
    assert np.array_equal(open_["U_exec"][scen, :2], rep(ref.U)[:, :2])


# ------------------------------------------------------------------------------------ 8. the loop
def _loop_problem(k=3):
    import dpilqr_amd as dp
    dp._reset_ids()
    xf = np.array([3.0, 3, 0, 0, -1, -1, 0, 0, 1, -2, 0, 0.0])
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(xf[4 * i:4 * i + 4], np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k))), xf


S_LOOP, N_LOOP, H_LOOP, L_LOOP, RADIUS = 6, 10, 2, 6, 1.0


def _loop_inputs():
    rng = np.random.default_rng(5150)
    x0 = np.array([0.0, 0, 0, 0, 2, 2, 0, 0, -2, 1, 0, 0.0])[None] + 0.3 * rng.normal(size=(S_LOOP, 12)) * np.tile([1, 1, 0.1, 0.1], 3)
    U0 = rng.random((S_LOOP, N_LOOP, 6)) * 0.01
    W = pc.W_SCALE * rng.normal(size=(S_LOOP, L_LOOP, 12))      # as tests/policy_cases.py draws it
    return x0, U0, W


def _loop_by_hand(problem, x0, U0, W, u_lim, centralized, feedback=True):
    """The receding-horizon loop from the pieces that existed before the advance: solve; backward_pass or policy=True;
    policy_rollout / DistributedPolicy.rollout with one sample and W padded to the horizon; the NumPy shift."""
    import dpilqr_amd as dp
    from dpilqr_amd.device import to_dev
    from dpilqr_amd.dispatch import device_constants, solve_scenarios_distributed
    from dpilqr_amd.lowering import describe
    d = describe(problem)
    c = device_constants(d)
    S, n, m, N, h = x0.shape[0], 12, 6, N_LOOP, H_LOOP
    xf_d = to_dev(np.broadcast_to(d["xf"], (S, n)).copy())
    x, U, X = x0.copy(), U0.copy(), None
    Xe, Ue = [x0[:, None].copy()], []
    for r in range(L_LOOP // h):
        Wp = np.zeros((S, 1, N, n)); Wp[:, 0, :h] = W[:, r * h:(r + 1) * h]
        if centralized:
            pb = dp.ProblemBatch(c["model"], c["n_dims"], xf_d, c["Q"], c["R"], c["Qf"], d["radius"], d["dt"], N, w_ref=d["w_ref"],
                                 w_prox=d["w_prox"], B=S, hints=(3, 4, 2, c["word"]))
            sol = pb.solve(x, U)
            K = pb.backward_pass(sol["X"], sol["U"], 0.0)[0]
            Xp, Up = sol["X"].cpu().numpy(), sol["U"].cpu().numpy()
            out = _host(pb.policy_rollout(sol["X"], sol["U"], K, x[:, None], W=Wp, u_lim=u_lim, trajectories=True))
        else:
            Xin = x[:, None, :] if X is None else X
            Xd, Ud, _, info = solve_scenarios_distributed(problem, Xin, U, RADIUS, xf=xf_d, device_out=True, desc=d, policy=True, policy_mu=0.0)
            Xp, Up = Xd.cpu().numpy(), Ud.cpu().numpy()
            out = _host(info["policy"].rollout(x[:, None], W=Wp, u_lim=u_lim, trajectories=True))
        Xe.append(out["X"][:, 0, 1:h + 1]); Ue.append(out["U"][:, 0, :h])
        x = out["X"][:, 0, h].copy()
        nxt = [ac.shift(Xp[s], Up[s], x[s], h) for s in range(S)]
        U, X = np.stack([v[0] for v in nxt]), np.stack([v[1] for v in nxt])
    return np.concatenate(Xe, axis=1), np.concatenate(Ue, axis=1)


@pytest.mark.parametrize("centralized", [True, False])
def test_the_loop_is_the_loop_written_by_hand(centralized):
    import dpilqr_amd as dp
    problem, xf = _loop_problem()
    x0, U0, W = _loop_inputs()
    kw = dict(radius=RADIUS, U0=U0, centralized=centralized, step_size=H_LOOP, dist_converge=1e-3, max_steps=L_LOOP)
    free = np.stack(dp.solve_rhc_closed_loop(problem, x0, N_LOOP, W=W, **kw)["U"]).reshape(-1, 6)
    u_lim = np.stack([np.quantile(free, q, axis=0) for q in pc.QUANTILES])      # as tests/policy_cases.py draws the limits
    got = dp.solve_rhc_closed_loop(problem, x0, N_LOOP, W=W, u_lim=u_lim, **kw)
    Xh, Uh = _loop_by_hand(problem, x0, U0, W, u_lim, centralized)
    assert (got["n_rounds"] == L_LOOP // H_LOOP).all() and not got["converged"].any()      # 1e-3 is not reached in six steps
    X, U = np.stack(got["X"]), np.stack(got["U"])
    assert X.shape == (S_LOOP, L_LOOP + 1, 12) and U.shape == (S_LOOP, L_LOOP, 6)
    bound = (U == u_lim[0]) | (U == u_lim[1])
    assert bound.any() and not bound.all()      # the limits bind somewhere, not everywhere
    for r in range(L_LOOP // H_LOOP):
        sl = slice(r * H_LOOP, (r + 1) * H_LOOP)
        print(f"centralized={centralized} round {r}: X {relerr(X[:, sl.stop], Xh[:, sl.stop]):.3g} U {relerr(U[:, sl], Uh[:, sl]):.3g}")
    assert np.array_equal(X, Xh) and np.array_equal(U, Uh)
    # the realised cost: the executed stage costs plus the terminal cost of the final state
    pb = dp.ProblemBatch([0] * 3, [2] * 3, np.tile(xf, (S_LOOP, 1)), np.eye(4), np.eye(2), 100.0 * np.eye(4), 0.5, 0.1, L_LOOP)
    J = pb.cost(X[:, :-1], U).cpu().numpy().sum(axis=1) + pb.cost(X[:, -1:], np.zeros((S_LOOP, 1, 6)), terminal=True).cpu().numpy()[:, 0]
    assert np.all(np.abs(got["J"] - J) <= pc.TOL_ROLLOUT * np.abs(J))
    e = (X[:, -1] - xf).reshape(S_LOOP, 3, 4)[:, :, :2]
    assert relerr(got["goal_dist"], np.sqrt((e * e).sum(axis=2))) <= pc.TOL_ROLLOUT
    # feedback=False under the same disturbance executes the plans open loop: the gains are not silently dropped above
    open_ = dp.solve_rhc_closed_loop(problem, x0, N_LOOP, W=W, u_lim=u_lim, feedback=False, **kw)
    assert not np.array_equal(np.stack(open_["U"]), U)
    assert np.array_equal(np.stack(open_["U"])[:, 0], U[:, 0])      # x = X[0] at the first step: K dx = 0


@pytest.mark.parametrize("centralized,feedback", [(True, True), (True, False), (False, False), (False, True)])
def test_an_ideal_plant_is_solve_rhc_scenarios_first_round(centralized, feedback):
    """W = None, u_lim = None: the plant follows the plan, so the first round's executed states are solve_rhc_scenarios'."""
    import dpilqr_amd as dp
    problem, _ = _loop_problem()
    x0, U0, _ = _loop_inputs()
    got = dp.solve_rhc_closed_loop(problem, x0, N_LOOP, radius=RADIUS, U0=U0, centralized=centralized, feedback=feedback, step_size=H_LOOP,
                                   dist_converge=1e-3, max_steps=H_LOOP)
    assert got["converged"].tolist() == [False] * S_LOOP and (got["n_rounds"] == 1).all()
    want = dp.solve_rhc_scenarios(problem, x0, N_LOOP, RADIUS, U0=U0, centralized=centralized, step_size=H_LOOP, dist_converge=1e-3,
                                  t_diverge=1e-9)      # two rounds: the second one's first state is where the first one ended
    worst = max(max(relerr(got["X"][s], want[s][0][:H_LOOP + 1]), relerr(got["U"][s], want[s][1][:H_LOOP])) for s in range(S_LOOP))
    print(f"centralized={centralized} feedback={feedback}: worst {worst:.3g}")
    for s in range(S_LOOP):
        assert got["X"][s].shape == (H_LOOP + 1, 12) and want[s][0].shape[0] >= H_LOOP + 1
        assert relerr(got["X"][s], want[s][0][:H_LOOP + 1]) <= pc.TOL_ROLLOUT, (s, relerr(got["X"][s], want[s][0][:H_LOOP + 1]))
        assert relerr(got["U"][s], want[s][1][:H_LOOP]) <= pc.TOL_ROLLOUT
