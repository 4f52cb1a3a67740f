"""The receding-horizon advance for large clusters (dpilqr_policy_advance_large, csrc/policy_advance_large.hpp) and the loop
built on it (solve_rhc_closed_loop(large=True)).

Cases: tests/policy_large_cases.py, every (item, sample) one scenario with the item's plan repeated
(tests/policy_advance_large_cases.py).  The executed prefix is held BIT FOR BIT to the rollout kernel whose product it restates
(ProblemBatch.policy_rollout_large with trajectories, the samples of an item side by side in its column tiles where the advance
has one live column); the executed cost, the separation and the distance left to the CPU reference's prefix within
policy_cases.bound_of of the sample's own sensitivity; the shift to its NumPy definition; two calls equal one; the capacity
holds; without gains the plan is executed as it stands; a poisoned item and the words around the outputs stay where they are;
and solve_rhc_closed_loop(large=True) equals a loop written here from the public pieces that existed before it."""
import numpy as np
import pytest

from tests import policy_advance_large_cases as alc
from tests import policy_cases as pc
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

B, T = alc.B, alc.T
VARIANTS = ("plain", "W", "u_lim")
FIELDS = ("x_cur", "n_done", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left", "U_next", "X_next")


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
        ref = alc.case_ref(case)
        rp = alc.repeated(case, ref)
        pb = alc.problem_batch(case, ref.batch, repeat=case.S)
        assert pb.is_large
        _SETUP[case.id] = (ref, rp, pb, alc.scen_of(case, rp["n"]))
    return _SETUP[case.id]


def rollout(case, variant):
    """The kernel the advance restates, once per variant: policy_rollout_large on the case's own batch, every sample's trajectory."""
    if (case.id, variant) not in _ROLL:
        ref = alc.case_ref(case)
        W, lim = ref.args(variant)
        r = _host(alc.problem_batch(case, ref.batch).policy_rollout_large(ref.X, ref.U, ref.K, ref.batch["x0s"], W=W, u_lim=lim,
                                                                          trajectories=True))
        _ROLL[(case.id, variant)] = {k_: v.reshape((B * case.S,) + v.shape[2:]) for k_, v in r.items()}
    return _ROLL[(case.id, variant)]


def advance(case, variant, h, gains=True):
    """One advance launch of all B * S scenarios through a non-identity scen into a NaN-filled state with spare scenarios."""
    key = (case.id, variant, h, gains)
    if key not in _ADV:
        ref, rp, pb, scen = setup(case)
        n_state = rp["n"] + alc.SPARE
        _, lim = ref.args(variant)
        st = _nan_state(pb, n_state, T, scen, rp["x0"])
        W = _state_W(rp["W"], scen, n_state, T) if variant == "W" else None
        pb.policy_advance_large(rp["X"], rp["U"], rp["K"] if gains else None, h, st, scen=scen, W=W, u_lim=lim, n_d=alc.N_D)
        _ADV[key] = _host(st)
    return _ADV[key]


def _unnamed(scen, n_state):
    return np.setdiff1d(np.arange(n_state), scen)


# ------------------------------------------------------------------------------------ 1. bit-equal to the rollout it restates
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case,h", alc.CASE_H, ids=alc.CASE_H_IDS)
def test_executed_prefix_is_the_large_rollouts(case, h, variant):
    ref, rp, pb, scen = setup(case)
    assert not np.array_equal(scen, np.arange(rp["n"]))      # the map is not the identity
    roll, st = rollout(case, variant), advance(case, variant, h)
    assert np.array_equal(st["X_exec"][scen, :h + 1], roll["X"][:, :h + 1])
    assert np.array_equal(st["U_exec"][scen, :h], roll["U"][:, :h])
    assert np.array_equal(st["x_cur"][scen], roll["X"][:, h])
    assert (st["n_done"][scen] == h).all()
    assert np.isnan(st["X_exec"][scen, h + 1:]).all() and np.isnan(st["U_exec"][scen, h:]).all()      # nothing past the executed steps
    rest = _unnamed(scen, rp["n"] + alc.SPARE)
    assert len(rest) == alc.SPARE and (st["n_done"][rest] == 0).all()
    for f in ("x_cur", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left", "U_next", "X_next"):
        assert np.isnan(st[f][rest]).all(), f      # scenarios not named keep their NaN


# ------------------------------------------------------------------------------------ 2. against the CPU reference, per scenario
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case,h", alc.CASE_H, ids=alc.CASE_H_IDS)
def test_cost_separation_and_distance_against_the_reference(case, h, variant):
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
            J, sep, left = alc.prefix(case, ref, variant, i, s, h)
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


# ------------------------------------------------------------------------------------ 3. the shift, the capacity
@pytest.mark.parametrize("case,h", alc.CASE_H, ids=alc.CASE_H_IDS)
def test_the_shift_is_its_definition(case, h):
    ref, rp, pb, scen = setup(case)
    st = advance(case, "u_lim", h)
    for j in range(rp["n"]):
        Un, Xn = alc.shift(rp["X"][j], rp["U"][j], st["x_cur"][scen[j]], h)
        assert np.array_equal(st["U_next"][scen[j]], Un) and np.array_equal(st["X_next"][scen[j]], Xn), j
    if h == T:
        assert (st["U_next"][scen] == 0.0).all()
        assert np.array_equal(st["X_next"][scen, 0], st["x_cur"][scen])
        assert np.array_equal(st["X_next"][scen, 1:], np.repeat(rp["X"][:, T:T + 1], T, axis=1))


@pytest.mark.parametrize("case", alc.CASES, ids=alc.IDS)
def test_the_capacity_is_never_passed(case):
    """n_done = L - 1 and h = 3: one step is executed and the plan is shifted by one; n_done = L: nothing is executed."""
    import torch
    ref, rp, pb, scen = setup(case)
    n_state, L = rp["n"] + alc.SPARE, 4
    st = _nan_state(pb, n_state, L, scen, rp["x0"])
    st["n_done"].copy_(torch.full((n_state,), L - 1, dtype=torch.int32))
    st["min_sep"].fill_(float("inf"))
    Wn = np.full((n_state, L, pb.n_x), np.nan); Wn[scen, L - 1] = rp["W"][:, 0]
    got = _host(pb.policy_advance_large(rp["X"], rp["U"], rp["K"], 3, st, scen=scen, W=Wn, n_d=alc.N_D))
    roll = rollout(case, "W")      # one step from the same starts under the same disturbance
    rest = _unnamed(scen, n_state)      # among them the scenarios that follow a named one in memory
    assert (got["n_done"][scen] == L).all() and (got["n_done"][rest] == L - 1).all()
    assert np.array_equal(got["X_exec"][scen, L - 1:], roll["X"][:, :2]) and np.array_equal(got["U_exec"][scen, L - 1], roll["U"][:, 0])
    assert np.isnan(got["X_exec"][scen, :L - 1]).all() and np.isnan(got["U_exec"][scen, :L - 1]).all()
    assert np.isnan(got["X_exec"][rest]).all() and np.isnan(got["U_exec"][rest]).all() and np.isnan(got["X_next"][rest]).all()
    for j in range(rp["n"]):
        Un, Xn = alc.shift(rp["X"][j], rp["U"][j], got["x_cur"][scen[j]], 1)      # the shift follows the executed step
        assert np.array_equal(got["U_next"][scen[j]], Un) and np.array_equal(got["X_next"][scen[j]], Xn), j
    # a full scenario executes nothing more; its warm start is its plan, unshifted, behind the plant's state
    again = _host(pb.policy_advance_large(rp["X"], rp["U"], rp["K"], 2, st, scen=scen, W=Wn, n_d=alc.N_D))
    for f in ("X_exec", "U_exec", "J_exec", "min_sep", "n_done", "x_cur", "dist_left"):
        assert np.array_equal(again[f][scen], got[f][scen], equal_nan=True), f
    assert np.array_equal(again["U_next"][scen], rp["U"]) and np.array_equal(again["X_next"][scen, 1:], rp["X"][:, 1:])
    assert np.array_equal(again["X_next"][scen, 0], got["x_cur"][scen])


# ------------------------------------------------------------------------------------ 4. two calls equal one
@pytest.mark.parametrize("case", alc.CASES, ids=alc.IDS)
def test_two_calls_equal_one(case):
    """h = 1, then h = 2 on the plan sliced from step 1 (padded on the host, the gains with it), W read at the global step, under
    limits too, against one call of h = 3: the offsets n_done gives into W and the executed buffers, one addition per step into
    J_exec."""
    ref, rp, pb, scen = setup(case)
    n_state, L = rp["n"] + alc.SPARE, 5
    W = _state_W(rp["W"], scen, n_state, L)
    fresh = lambda: _nan_state(pb, n_state, L, scen, rp["x0"])

    one = _host(pb.policy_advance_large(rp["X"], rp["U"], rp["K"], 3, fresh(), scen=scen, W=W, u_lim=ref.u_lim, n_d=alc.N_D))
    st = fresh()
    pb.policy_advance_large(rp["X"], rp["U"], rp["K"], 1, st, scen=scen, W=W, u_lim=ref.u_lim, n_d=alc.N_D)
    pad = lambda a, last: np.concatenate([a[:, 1:], last], axis=1)
    X2, U2, K2 = pad(rp["X"], rp["X"][:, -1:]), pad(rp["U"], np.zeros_like(rp["U"][:, :1])), pad(rp["K"], np.zeros_like(rp["K"][:, :1]))
    two = _host(pb.policy_advance_large(X2, U2, K2, 2, st, scen=scen, W=W, u_lim=ref.u_lim, n_d=alc.N_D))
    for f in ("X_exec", "U_exec", "J_exec", "min_sep", "n_done", "x_cur", "dist_left"):
        assert np.array_equal(one[f][scen], two[f][scen], equal_nan=True), f      # (NaN: the rows past the three executed steps)
    assert (two["n_done"][scen] == 3).all() and np.isfinite(two["J_exec"][scen]).all()
    # the warm start after the two calls is the one call's: the plan shifted by three
    assert np.array_equal(one["U_next"][scen][:, :T - 3], two["U_next"][scen][:, :T - 3])
    assert np.array_equal(one["X_next"][scen], two["X_next"][scen])


# ------------------------------------------------------------------------------------ 5. K = NULL
@pytest.mark.parametrize("case,h", alc.CASE_H, ids=alc.CASE_H_IDS)
def test_without_gains_the_plan_is_executed_open_loop(case, h):
    ref, rp, pb, scen = setup(case)
    free = advance(case, "plain", h, gains=False)
    assert np.array_equal(free["U_exec"][scen, :h], rp["U"][:, :h])
    assert (free["n_done"][scen] == h).all() and np.isnan(free["U_exec"][scen, h:]).all()
    if h == T:
        lim = ref.u_lim
        st = advance(case, "u_lim", T, gains=False)
        want = np.where(rp["U"] < lim[0], lim[0], np.where(rp["U"] > lim[1], lim[1], rp["U"]))
        assert np.array_equal(st["U_exec"][scen], want)
        Xr, _ = pb.rollout(rp["x0"], rp["U"])
        Xr = Xr.cpu().numpy()
        for j in range(rp["n"]):
            assert relerr(free["X_exec"][scen[j]], Xr[j]) <= pc.TOL_ROLLOUT, (j, relerr(free["X_exec"][scen[j]], Xr[j]))


# ------------------------------------------------------------------------------------ 6. guards
@pytest.mark.parametrize("case", alc.CASES, ids=alc.IDS)
def test_a_poisoned_item_stays_alone(case):
    """One item's plan, gains and plant state are NaN: every other scenario's fields are what they are without the poison."""
    ref, rp, pb, scen = setup(case)
    j0 = rp["n"] // 2
    X, U, K, x0 = rp["X"].copy(), rp["U"].copy(), rp["K"].copy(), rp["x0"].copy()
    X[j0], U[j0], K[j0], x0[j0] = np.nan, np.nan, np.nan, np.nan
    n_state = rp["n"] + alc.SPARE
    st = _nan_state(pb, n_state, T, scen, x0)
    W = _state_W(rp["W"], scen, n_state, T)
    got = _host(pb.policy_advance_large(X, U, K, 3, st, scen=scen, W=W, n_d=alc.N_D))
    clean = advance(case, "W", 3)
    others = np.setdiff1d(np.arange(n_state), [scen[j0]])
    for f in FIELDS:
        assert np.array_equal(got[f][others], clean[f][others], equal_nan=True), f
    assert got["n_done"][scen[j0]] == 3 and np.isnan(got["X_exec"][scen[j0]]).all() and np.isnan(got["J_exec"][scen[j0]])


@pytest.mark.parametrize("case", alc.CASES, ids=alc.IDS)
def test_nothing_is_written_around_the_state(case):
    """Every buffer of the state a view into a larger one with a stretch of a sentinel before and after it."""
    import torch
    ref, rp, pb, scen = setup(case)
    n_state, G, SENT = rp["n"] + alc.SPARE, 4096, -7.25
    st = _nan_state(pb, n_state, T, scen, rp["x0"])
    bufs, view = {}, {}
    for f, t in st.items():
        sent = 77 if f == "n_done" else SENT
        bufs[f] = torch.full((G + t.numel() + G,), sent, dtype=t.dtype, device=t.device)
        view[f] = bufs[f][G:G + t.numel()].view(t.shape)
        view[f].copy_(t)
    pb.policy_advance_large(rp["X"], rp["U"], rp["K"], 3, view, scen=scen, u_lim=ref.u_lim, n_d=alc.N_D)
    torch.cuda.synchronize()
    want = advance(case, "u_lim", 3)
    for f, t in st.items():
        h_ = bufs[f].cpu().numpy()
        sent = 77 if f == "n_done" else SENT
        assert (h_[:G] == sent).all() and (h_[G + t.numel():] == sent).all(), f
        assert np.array_equal(h_[G:G + t.numel()].reshape(t.shape), want[f], equal_nan=True), f


# ------------------------------------------------------------------------------------ 7. the loop
K_LOOP, S_LOOP, N_LOOP, H_LOOP, L_LOOP = 16, 3, 10, 2, 4
N_X, N_U = 4 * K_LOOP, 2 * K_LOOP


def _loop_problem():
    import dpilqr_amd as dp
    dp._reset_ids()
    k = K_LOOP
    ang = 2.0 * np.pi * np.arange(k) / k
    x0 = np.zeros((k, 4)); xf = np.zeros((k, 4))
    x0[:, 0], x0[:, 1] = 4.0 * np.cos(ang), 4.0 * np.sin(ang)
    xf[:, 0], xf[:, 1] = 3.0 * np.cos(ang + 0.4), 3.0 * np.sin(ang + 0.4)
    x0, xf = x0.reshape(-1), xf.reshape(-1)
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(xf[4 * i:4 * i + 4], np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k))), x0, xf


def _loop_inputs(x0):
    rng = np.random.default_rng(5150)
    x0s = x0[None] + 0.3 * rng.normal(size=(S_LOOP, N_X)) * np.tile([1, 1, 0.1, 0.1], K_LOOP)
    U0 = rng.random((S_LOOP, N_LOOP, N_U)) * 0.01
    W = pc.W_SCALE * rng.normal(size=(S_LOOP, L_LOOP, N_X))      # as tests/policy_cases.py draws it
    return x0s, U0, W


def _loop_by_hand(problem, x0, U0, W, u_lim):
    """The receding-horizon loop from the pieces that existed before the advance: solve; backward_pass; policy_rollout_large with
    one sample and W padded to the horizon; the NumPy shift.  Returns the executed X, U and every round's planned U[0]."""
    import dpilqr_amd as dp
    from dpilqr_amd.device import to_dev
    from dpilqr_amd.dispatch import device_constants
    from dpilqr_amd.lowering import describe
    d = describe(problem)
    c = device_constants(d)
    S, n, N, h = x0.shape[0], N_X, N_LOOP, H_LOOP
    xf_d = to_dev(np.broadcast_to(d["xf"], (S, n)).copy())
    x, U = x0.copy(), U0.copy()
    Xe, Ue, first = [x0[:, None].copy()], [], []
    for r in range(L_LOOP // h):
        Wp = np.zeros((S, 1, N, n)); Wp[:, 0, :h] = W[:, r * h:(r + 1) * h]
        pb = dp.ProblemBatch(c["model"], c["n_dims"], xf_d, c["Q"], c["R"], c["Qf"], d["radius"], d["dt"], N, w_ref=d["w_ref"],
                             w_prox=d["w_prox"], B=S, hints=(K_LOOP, 4, 2, c["word"]))
        assert pb.is_large
        sol = pb.solve(x, U)
        K = pb.backward_pass(sol["X"], sol["U"], 0.0)[0]
        Xp, Up = sol["X"].cpu().numpy(), sol["U"].cpu().numpy()
        out = _host(pb.policy_rollout_large(sol["X"], sol["U"], K, x[:, None], W=Wp, u_lim=u_lim, trajectories=True))
        Xe.append(out["X"][:, 0, 1:h + 1]); Ue.append(out["U"][:, 0, :h]); first.append(Up[:, 0])
        x = out["X"][:, 0, h].copy()
        U = np.stack([alc.shift(Xp[s], Up[s], x[s], h)[0] for s in range(S)])
    return np.concatenate(Xe, axis=1), np.concatenate(Ue, axis=1), first


def test_the_large_loop_is_the_loop_written_by_hand():
    import dpilqr_amd as dp
    problem, x0, xf = _loop_problem()
    x0s, U0, W = _loop_inputs(x0)
    kw = dict(U0=U0, step_size=H_LOOP, dist_converge=1e-3, max_steps=L_LOOP, large=True)
    free = np.stack(dp.solve_rhc_closed_loop(problem, x0s, N_LOOP, W=W, **kw)["U"]).reshape(-1, N_U)
    u_lim = np.stack([np.quantile(free, q, axis=0) for q in pc.QUANTILES])      # as tests/policy_cases.py draws the limits
    got = dp.solve_rhc_closed_loop(problem, x0s, N_LOOP, W=W, u_lim=u_lim, **kw)
    Xh, Uh, first = _loop_by_hand(problem, x0s, U0, W, u_lim)
    assert (got["n_rounds"] == L_LOOP // H_LOOP).all() and not got["converged"].any()      # 1e-3 is not reached in four steps
    X, U = np.stack(got["X"]), np.stack(got["U"])
    assert X.shape == (S_LOOP, L_LOOP + 1, N_X) and U.shape == (S_LOOP, L_LOOP, N_U)
    bound = (U == u_lim[0]) | (U == u_lim[1])
    assert bound.any() and not bound.all()      # the limits bind somewhere, not everywhere
    for r in range(L_LOOP // H_LOOP):
        sl = slice(r * H_LOOP, (r + 1) * H_LOOP)
        print(f"round {r}: X {relerr(X[:, sl.stop], Xh[:, sl.stop]):.3g} U {relerr(U[:, sl], Uh[:, sl]):.3g}")
    assert np.array_equal(X, Xh) and np.array_equal(U, Uh)
    # the realised cost: the executed stage costs plus the terminal cost of the final state
    pb = dp.ProblemBatch([0] * K_LOOP, [2] * K_LOOP, np.tile(xf, (S_LOOP, 1)), np.eye(4), np.eye(2), 100.0 * np.eye(4), 0.5, 0.1, L_LOOP)
    J = pb.cost(X[:, :-1], U).cpu().numpy().sum(axis=1) + pb.cost(X[:, -1:], np.zeros((S_LOOP, 1, N_U)), terminal=True).cpu().numpy()[:, 0]
    assert np.all(np.abs(got["J"] - J) <= pc.TOL_ROLLOUT * np.abs(J))
    e = (X[:, -1] - xf).reshape(S_LOOP, K_LOOP, 4)[:, :, :2]
    assert relerr(got["goal_dist"], np.sqrt((e * e).sum(axis=2))) <= pc.TOL_ROLLOUT
    # at a round's first step the plant is on the plan, x = X[0]: K dx = 0 and the executed control is the planned one, limited
    clamp = lambda u: np.where(u < u_lim[0], u_lim[0], np.where(u > u_lim[1], u_lim[1], u))
    for r in range(L_LOOP // H_LOOP):
        assert np.array_equal(U[:, r * H_LOOP], clamp(first[r])), r
    # feedback=False under the same disturbance executes the plans open loop: the gains are not silently dropped above
    open_ = np.stack(dp.solve_rhc_closed_loop(problem, x0s, N_LOOP, W=W, u_lim=u_lim, feedback=False, **kw)["U"])
    assert not np.array_equal(open_, U)
    assert np.array_equal(open_[:, 0], U[:, 0])      # the first round's first step: the same plan, K dx = 0
    assert not np.array_equal(open_[:, 1], U[:, 1])      # ... and its second step already differs: the disturbance is fed back
    # a problem of n_x <= 60 takes the existing route whatever `large` says
    assert dp.solve_rhc_closed_loop is dp.distributed.solve_rhc_closed_loop
