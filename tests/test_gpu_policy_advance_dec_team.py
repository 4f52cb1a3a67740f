"""The team receding-horizon advance (dpilqr_policy_advance_dec_team, csrc/policy_advance_dec_team.hpp) on the GPU, and the
distributed loop built on it (solve_rhc_closed_loop(centralized=False, team=True)).

Cases: tests/policy_dec_team_cases.py, every (item, sample) one scenario with the item's plan repeated
(tests/policy_advance_dec_team_cases.py); the kernel gets the compact gains with every unused column NaN.
  prefix      X_exec / U_exec bit for bit against the rollout it restates (ProblemBatch.policy_rollout_dec_team)
  reference   J_exec, min_sep, dist_left against the CPU reference's prefix within the sample's own bound
  shift       against its NumPy definition; two calls equal one; the capacity; entries of scen out of range; open loop; columns
              never read; position independence and guard rows; NaN containment
  cross       against policy_advance_dec where both serve the shape (mixed models; mixed n_dims)
  loop        24 double integrators: solve_rhc_closed_loop(team=True) against the loop written from the pieces that existed
              before it; an ideal plant against solve_rhc_scenarios' first round"""
import numpy as np
import pytest

from tests import policy_advance_cases as ac
from tests import policy_advance_dec_team_cases as atc
from tests import policy_cases as pc
from tests import policy_dec_cases as dc
from tests import policy_dec_team_cases as tc
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

B, T = pc.B, pc.T
FIELDS = ("x_cur", "n_done", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left", "U_next", "X_next")
BITWISE = ("X_exec", "U_exec", "x_cur", "n_done", "dist_left", "U_next", "X_next")


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


def _unnamed(scen, n_state):
    return np.setdiff1d(np.arange(n_state), scen)


_SETUP, _ROLL, _ADV = {}, {}, {}


def setup(case):
    if case.id not in _SETUP:
        ref = tc.case_ref(case)
        rp = atc.repeated(case, ref)
        assert np.isnan(rp["Kc"]).any() or case.k == 1
        _SETUP[case.id] = (ref, rp, ac.problem_batch(case, ref.batch, repeat=case.S), ac.scen_of(case, rp["n"]))
    return _SETUP[case.id]


def rollout(case, variant):
    """The kernel the advance restates, once per variant: policy_rollout_dec_team on the case's own batch, every sample's trajectory."""
    if (case.id, variant) not in _ROLL:
        ref = tc.case_ref(case)
        W, lim = ref.args(variant)
        Kc = dc.compact_gains(ref.K, ref.masks, case.ns, case.nc, case.k)
        r = _host(ac.problem_batch(case, ref.batch).policy_rollout_dec_team(ref.X, ref.U, Kc, ref.masks, ref.batch["x0s"], W=W, u_lim=lim,
                                                                            trajectories=True))
        _ROLL[(case.id, variant)] = {k_: v.reshape((B * case.S,) + v.shape[2:]) for k_, v in r.items()}
    return _ROLL[(case.id, variant)]


def advance(case, variant, h, gains=True):
    """One launch of all B * S scenarios through a non-identity scen into a NaN-filled state with spare scenarios."""
    key = (case.id, variant, h, gains)
    if key not in _ADV:
        ref, rp, pb, scen = setup(case)
        n_state = rp["n"] + atc.SPARE
        _, lim = ref.args(variant)
        st = _nan_state(pb, n_state, T, scen, rp["x0"])
        W = _state_W(rp["W"], scen, n_state, T) if variant == "W" else None
        pb.policy_advance_dec_team(rp["X"], rp["U"], rp["Kc"] if gains else None, rp["masks"] if gains else None, h, st, scen=scen, W=W,
                                   u_lim=lim, n_d=atc.N_D)
        _ADV[key] = _host(st)
    return _ADV[key]


# ------------------------------------------------------------------------------------ 1. bit-equal to the rollout it restates
@pytest.mark.parametrize("h", atc.HS)
@pytest.mark.parametrize("variant", atc.VARIANTS)
@pytest.mark.parametrize("case", atc.CASES, ids=atc.IDS)
def test_executed_prefix_is_the_team_rollouts(case, variant, h):
    ref, rp, pb, scen = setup(case)
    roll, st = rollout(case, variant), advance(case, variant, h)
    assert np.array_equal(st["X_exec"][scen, :h + 1], roll["X"][:, :h + 1])
    assert np.array_equal(st["U_exec"][scen, :h], roll["U"][:, :h])
    assert np.array_equal(st["x_cur"][scen], roll["X"][:, h])
    assert (st["n_done"][scen] == h).all()
    assert np.isnan(st["X_exec"][scen, h + 1:]).all() and np.isnan(st["U_exec"][scen, h:]).all()      # nothing past the executed steps
    rest = _unnamed(scen, rp["n"] + atc.SPARE)
    assert len(rest) == atc.SPARE and (st["n_done"][rest] == 0).all()
    for f in FIELDS:
        if f != "n_done":
            assert np.isnan(st[f][rest]).all(), f      # scenarios not named keep their NaN


# ------------------------------------------------------------------------------------ 2. against the CPU reference, per scenario
def worst_against_reference(case, variant, h, st, scen):
    """(largest error / bound, largest error, its bound, scenarios without a bound, failures)."""
    ref = tc.case_ref(case)
    worst, at, unchecked, failures = 0.0, (0.0, 0.0), 0, []
    for i in range(B):
        for s in range(case.S):
            bound = pc.bound_of(ref.spread[variant][i, s])
            if bound is None:
                unchecked += 1
                continue
            d = atc.scenario_error(st, scen[i * case.S + s], *atc.prefix(case, ref, variant, i, s, h))
            if d / bound >= worst:
                worst, at = d / bound, (d, bound)
            if not d <= bound:
                failures.append((i, s, d, bound))
    return worst, at[0], at[1], unchecked, failures


@pytest.mark.parametrize("h", atc.HS)
@pytest.mark.parametrize("variant", atc.VARIANTS)
@pytest.mark.parametrize("case", atc.CASES, ids=atc.IDS)
def test_cost_separation_and_distance_against_the_reference(case, variant, h):
    ref, rp, pb, scen = setup(case)
    st = advance(case, variant, h)
    worst, d, bound, unchecked, failures = worst_against_reference(case, variant, h, st, scen)
    print(f"{case.id} {variant} h={h}: worst error / bound {worst:.3g} (error {d:.3g}, bound {bound:.3g}), unchecked {unchecked} of {B * case.S}")
    assert unchecked <= pc.MAX_UNCHECKED * B * case.S, (unchecked, B * case.S)
    assert not failures, failures[:5]
    assert np.isfinite(st["J_exec"][scen]).all() and np.isfinite(st["min_sep"][scen]).all()


# ------------------------------------------------------------------------------------ 3. the shift
@pytest.mark.parametrize("h", (1, 3, T))
@pytest.mark.parametrize("case", atc.CASES, ids=atc.IDS)
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
@pytest.mark.parametrize("case", atc.CASES, ids=atc.IDS)
def test_two_calls_equal_one(case):
    """h = 1, then h = 2 on the plan sliced from step 1 (padded on the host), W read at the global step, under limits too,
    against one call of h = 3: the offsets n_done gives into W and the executed buffers, one addition per step into J_exec."""
    ref, rp, pb, scen = setup(case)
    n_state, L = rp["n"] + atc.SPARE, 5
    W = _state_W(rp["W"], scen, n_state, L)
    fresh = lambda: _nan_state(pb, n_state, L, scen, rp["x0"])
    kw = dict(scen=scen, W=W, u_lim=ref.u_lim, n_d=atc.N_D)

    one = _host(pb.policy_advance_dec_team(rp["X"], rp["U"], rp["Kc"], rp["masks"], 3, fresh(), **kw))
    st = fresh()
    pb.policy_advance_dec_team(rp["X"], rp["U"], rp["Kc"], rp["masks"], 1, st, **kw)
    pad = lambda a, last: np.concatenate([a[:, 1:], last], axis=1)
    X2, U2, K2 = pad(rp["X"], rp["X"][:, -1:]), pad(rp["U"], np.zeros_like(rp["U"][:, :1])), pad(rp["Kc"], np.zeros_like(rp["Kc"][:, :1]))
    two = _host(pb.policy_advance_dec_team(X2, U2, K2, rp["masks"], 2, st, **kw))
    for f in ("X_exec", "U_exec", "J_exec", "min_sep", "n_done", "x_cur", "dist_left"):
        assert np.array_equal(one[f][scen], two[f][scen], equal_nan=True), f      # (NaN: the rows past the three executed steps)
    assert (two["n_done"][scen] == 3).all() and np.isfinite(two["J_exec"][scen]).all()
    for j in (0, rp["n"] - 1):      # ... and the plan shifted twice is the plan shifted by three
        Un, Xn = ac.shift(rp["X"][j], rp["U"][j], two["x_cur"][scen[j]], 3)
        assert np.array_equal(two["U_next"][scen[j]], Un) and np.array_equal(one["U_next"][scen[j]], Un)
        assert np.array_equal(one["X_next"][scen[j]], Xn)


# ------------------------------------------------------------------------------------ 5. the capacity, and entries of scen out of range
CAP_CASES = [atc.CASES[0], atc.CASES[5]]      # twelve and four items per workgroup


@pytest.mark.parametrize("case", CAP_CASES, ids=[c.id for c in CAP_CASES])
def test_the_capacity_is_never_passed(case):
    import torch
    ref, rp, pb, scen = setup(case)
    n, n_state, L = rp["n"], rp["n"] + atc.SPARE, 4
    full = scen[1::2]      # every other scenario is at its capacity already: he differs between the items of a workgroup
    st = _nan_state(pb, n_state, L, scen, rp["x0"])
    done = np.full(n_state, L - 1, dtype=np.int32); done[full] = L
    st["n_done"].copy_(torch.from_numpy(done))
    st["min_sep"].fill_(float("inf"))
    before = _host(st)
    Wn = np.full((n_state, L, pb.n_x), np.nan); Wn[scen, L - 1] = rp["W"][:, 0]
    got = _host(pb.policy_advance_dec_team(rp["X"], rp["U"], rp["Kc"], rp["masks"], 3, st, scen=scen, W=Wn, n_d=atc.N_D))
    roll = rollout(case, "W")      # one step from the same starts under the same disturbance
    short = np.arange(n)[0::2]
    assert (got["n_done"][scen] == L).all() and (got["n_done"][_unnamed(scen, n_state)] == L - 1).all()
    assert np.array_equal(got["X_exec"][scen[short], L - 1:], roll["X"][short, :2]) and np.array_equal(got["U_exec"][scen[short], L - 1], roll["U"][short, 0])
    assert np.isnan(got["X_exec"][scen[short], :L - 1]).all() and np.isnan(got["U_exec"][scen[short], :L - 1]).all()
    assert np.isfinite(got["J_exec"][scen[short]]).all()
    rest = _unnamed(scen, n_state)      # among them the scenarios that follow a named one in memory
    assert np.isnan(got["X_exec"][rest]).all() and np.isnan(got["U_exec"][rest]).all() and np.isnan(got["X_next"][rest]).all()
    for j in (0, short[-1]):
        Un, Xn = ac.shift(rp["X"][j], rp["U"][j], got["x_cur"][scen[j]], 1)      # the shift follows the executed step
        assert np.array_equal(got["U_next"][scen[j]], Un) and np.array_equal(got["X_next"][scen[j]], Xn)
    # a scenario at its capacity executes nothing: its plant state, executed cost and buffers are kept, only X_exec[L] is written again
    for f in ("U_exec", "J_exec", "n_done", "x_cur"):
        assert np.array_equal(got[f][full], before[f][full], equal_nan=True), f
    assert np.array_equal(got["X_exec"][full, :L], before["X_exec"][full, :L], equal_nan=True)
    assert np.array_equal(got["X_exec"][full, L], before["x_cur"][full])
    for j in (1, int(np.arange(n)[1::2][-1])):
        Un, Xn = ac.shift(rp["X"][j], rp["U"][j], got["x_cur"][scen[j]], 0)      # the plan is handed on unshifted
        assert np.array_equal(got["U_next"][scen[j]], Un) and np.array_equal(got["X_next"][scen[j]], Xn)
    # ... and a second call executes nothing for anybody
    again = _host(pb.policy_advance_dec_team(rp["X"], rp["U"], rp["Kc"], rp["masks"], 2, st, scen=scen, W=Wn, n_d=atc.N_D))
    for f in ("X_exec", "U_exec", "J_exec", "min_sep", "n_done", "x_cur"):
        assert np.array_equal(again[f][scen], got[f][scen], equal_nan=True), f


@pytest.mark.parametrize("case", CAP_CASES, ids=[c.id for c in CAP_CASES])
def test_a_scen_entry_out_of_range_is_skipped(case):
    """Given as a device tensor, which the host does not check: the entries -1, n_state and 2^31 - 1 name nobody."""
    import torch
    from dpilqr_amd.device import to_dev
    ref, rp, pb, scen = setup(case)
    n, n_state = rp["n"], rp["n"] + atc.SPARE
    base = advance(case, "plain", 3)
    bad = scen.copy()
    skipped = [0, n // 2, n - 1]
    bad[skipped] = [-1, n_state, 2 ** 31 - 1]
    st = _nan_state(pb, n_state, T, scen, rp["x0"])
    before = _host(st)
    got = _host(pb.policy_advance_dec_team(rp["X"], rp["U"], rp["Kc"], rp["masks"], 3, st, scen=to_dev(bad, torch.int32), n_d=atc.N_D))
    kept = np.setdiff1d(np.arange(n), skipped)
    for f in FIELDS:
        assert np.array_equal(got[f][scen[kept]], base[f][scen[kept]], equal_nan=True), f
        assert np.array_equal(got[f][scen[skipped]], before[f][scen[skipped]], equal_nan=True), f      # untouched
        rest = _unnamed(scen, n_state)
        assert np.array_equal(got[f][rest], before[f][rest], equal_nan=True), f


# ------------------------------------------------------------------------------------ 6. Kc = NULL
@pytest.mark.parametrize("case", atc.CASES, ids=atc.IDS)
def test_without_gains_the_plan_is_executed_open_loop(case):
    ref, rp, pb, scen = setup(case)
    lim = ref.u_lim
    st = advance(case, "u_lim", T, gains=False)
    want = np.where(rp["U"] < lim[0], lim[0], np.where(rp["U"] > lim[1], lim[1], rp["U"]))
    assert np.array_equal(st["U_exec"][scen], want)
    free = advance(case, "plain", T, gains=False)
    assert np.array_equal(free["U_exec"][scen], rp["U"])
    # ... whatever the masks: garbage masks beside no gains change nothing (they are not read)
    n_state = rp["n"] + atc.SPARE
    st2 = _nan_state(pb, n_state, T, scen, rp["x0"])
    pb.policy_advance_dec_team(rp["X"], rp["U"], None, np.zeros_like(rp["masks"]), T, st2, scen=scen, n_d=atc.N_D)
    st2 = _host(st2)
    for f in FIELDS:
        assert np.array_equal(st2[f], free[f], equal_nan=True), f
    assert not np.array_equal(free["U_exec"][scen], advance(case, "plain", T)["U_exec"][scen])      # the gains do something


# ------------------------------------------------------------------------------------ 7. columns never read
@pytest.mark.parametrize("case", [atc.CASES[0], atc.CASES[5]], ids=[atc.IDS[0], atc.IDS[5]])
def test_columns_past_a_neighbourhood_are_never_read(case):
    ref, rp, pb, scen = setup(case)
    base = advance(case, "u_lim", 3)      # NaN there
    zero = atc.repeated(case, ref, fill=0.0)
    assert not np.isnan(zero["Kc"]).any()
    st = _nan_state(pb, rp["n"] + atc.SPARE, T, scen, rp["x0"])
    got = _host(pb.policy_advance_dec_team(rp["X"], rp["U"], zero["Kc"], rp["masks"], 3, st, scen=scen, u_lim=ref.u_lim, n_d=atc.N_D))
    for f in FIELDS:
        assert np.array_equal(got[f], base[f], equal_nan=True), f
    assert np.isfinite(base["U_exec"][scen, :3]).all()


# ------------------------------------------------------------------------------------ 8. against policy_advance_dec
@pytest.mark.parametrize("case", atc.CROSS, ids=[c.id for c in atc.CROSS])
def test_against_the_old_kernel(case):
    ref = dc.case_ref(case)
    rp = atc.repeated(case, ref)
    pb, scen = ac.problem_batch(case, ref.batch, repeat=case.S), ac.scen_of(case, rp["n"])
    n_state = rp["n"] + atc.SPARE
    for v in atc.VARIANTS:
        _, lim = ref.args(v)
        W = _state_W(rp["W"], scen, n_state, T) if v == "W" else None
        for h in atc.HS:
            run = lambda f: _host(f(rp["X"], rp["U"], rp["Kc"], rp["masks"], h, _nan_state(pb, n_state, T, scen, rp["x0"]), scen=scen, W=W,
                                    u_lim=lim, n_d=atc.N_D))
            old, new = run(pb.policy_advance_dec), run(pb.policy_advance_dec_team)
            for f in BITWISE:
                assert np.array_equal(old[f], new[f], equal_nan=True), (v, h, f)
            eJ = np.max(np.abs(new["J_exec"][scen] - old["J_exec"][scen]) / np.abs(old["J_exec"][scen]))
            eS = np.max(np.abs(new["min_sep"][scen] - old["min_sep"][scen]) / np.abs(old["min_sep"][scen]))
            print(f"{case.id} {v} h={h}: J_exec {eJ:.2e}, min_sep {eS:.2e} (tol {pc.TOL_ROLLOUT:.0e})")
            assert np.isfinite(old["J_exec"][scen]).all() and eJ <= pc.TOL_ROLLOUT and eS <= pc.TOL_ROLLOUT, (v, h, eJ, eS)
            rest = _unnamed(scen, n_state)
            assert np.isnan(new["J_exec"][rest]).all() and np.isnan(new["min_sep"][rest]).all()


# ------------------------------------------------------------------------------------ 9. position independence and guard rows
POS_CASE = atc.CASES[0]      # 21 mixed agents, per-item weights, 12 items per workgroup


def _sub_batch(case, b, items):
    import dpilqr_amd as dp
    if case.weights == "per_item":
        Q, R, Qf = b["Q"][items], b["R"][items], b["Qf"][items]
    else:
        Q, R, Qf = b["Q"], b["R"], b["Qf"]
    return dp.ProblemBatch(b["models"], b["n_dims"], b["xf"][items], Q, R, Qf, b["radius"], b["dt"], T)


def test_position_independence_and_guards():
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import device, ptr, stream_handle, to_dev
    case = POS_CASE
    ref, rp, pb, scen = setup(case)
    S, k, n_all, h = case.S, case.k, rp["n"], 3
    base = advance(case, "W", h)
    item_of = np.repeat(np.arange(B), S)      # the case's item behind every scenario

    def run(order, scen_of_item):
        """The scenarios `order` (indices into the case's B * S) as one batch, item q at scenario scen_of_item[q]."""
        sub = _sub_batch(case, ref.batch, item_of[order])
        n_state = int(max(scen_of_item)) + 1
        st = _nan_state(sub, n_state, T, scen_of_item, rp["x0"][order])
        W = _state_W(rp["W"][order], scen_of_item, n_state, T)
        return _host(sub.policy_advance_dec_team(rp["X"][order], rp["U"][order], rp["Kc"][order], rp["masks"][order], h, st, scen=scen_of_item,
                                                 W=W, n_d=atc.N_D))

    # alone (B = 1): slot 0 of the only workgroup
    for j in (0, 17, n_all - 1):
        alone = run(np.array([j]), np.array([0], dtype=np.int32))
        for f in FIELDS:
            assert np.array_equal(alone[f][0], base[f][scen[j]], equal_nan=True), (j, f)
    # permuted across slots and workgroups, and a run repeated
    perm = np.random.default_rng(99).permutation(n_all)
    ident = np.arange(n_all, dtype=np.int32)
    shuffled, again = run(perm, ident), run(perm, ident)
    for f in FIELDS:
        assert np.array_equal(shuffled[f], base[f][scen[perm]], equal_nan=True), f
        assert np.array_equal(shuffled[f], again[f], equal_nan=True), f
    # guard rows around every state tensor, through the C entry
    n, m = pb.n_x, pb.n_u
    shapes = dict(x_cur=(n_all, n), n_done=(n_all,), X_exec=(n_all, T + 1, n), U_exec=(n_all, T, m), J_exec=(n_all,), min_sep=(n_all,),
                  dist_left=(n_all, k), U_next=(n_all, T, m), X_next=(n_all, T + 1, n))
    whole = {f: torch.full((sh[0] + 2,) + sh[1:], -7 if f == "n_done" else -7.25, dtype=torch.int32 if f == "n_done" else torch.float64,
                           device=device()) for f, sh in shapes.items()}
    view = {f: w[1:-1] for f, w in whole.items()}
    view["x_cur"].copy_(to_dev(rp["x0"])); view["n_done"].zero_(); view["J_exec"].zero_()
    dev = [to_dev(a) for a in (rp["X"], rp["U"], rp["Kc"], rp["W"])]
    bits = torch.from_numpy(rp["masks"].view(np.int64)).to(device())
    _lib.check(pb._lib.dpilqr_policy_advance_dec_team(pb._d, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), k, ptr(bits), h, None, n_all, T, atc.N_D,
                                                      ptr(dev[3]), None, *[ptr(view[f]) for f in FIELDS], stream_handle()))
    torch.cuda.synchronize()
    for f, w in whole.items():
        hst = w.cpu().numpy()
        g = -7 if f == "n_done" else -7.25
        assert (hst[0] == g).all() and (hst[-1] == g).all(), f
        want = base[f][scen]
        if f in ("X_exec", "U_exec"):      # (the rows past the executed steps keep the guard value here, NaN there)
            stop = h + 1 if f == "X_exec" else h
            assert np.array_equal(hst[1:-1][:, :stop], want[:, :stop]) and (hst[1:-1][:, stop:] == g).all(), f
        else:
            assert np.array_equal(hst[1:-1], want), f


# ------------------------------------------------------------------------------------ 10. NaN containment
def test_nan_poisons_only_its_scenario():
    case = POS_CASE
    ref, rp, pb, scen = setup(case)
    base = advance(case, "u_lim", 3)
    n_state = rp["n"] + atc.SPARE
    X, U, x0 = rp["X"].copy(), rp["U"].copy(), rp["x0"].copy()
    poisoned = [5, 12]      # slot 5 of the first workgroup, slot 0 of the second
    for j in poisoned:
        X[j] = np.nan; U[j] = np.nan; x0[j] = np.nan
    st = _nan_state(pb, n_state, T, scen, x0)
    got = _host(pb.policy_advance_dec_team(X, U, rp["Kc"], rp["masks"], 3, st, scen=scen, u_lim=ref.u_lim, n_d=atc.N_D))
    clean = np.setdiff1d(np.arange(rp["n"]), poisoned)
    for f in FIELDS:
        assert np.array_equal(got[f][scen[clean]], base[f][scen[clean]], equal_nan=True), f
    assert np.isfinite(base["J_exec"][scen]).all()
    assert np.isnan(got["J_exec"][scen[poisoned]]).all() and np.isnan(got["X_exec"][scen[poisoned], :4]).all()
    assert (got["n_done"][scen[poisoned]] == 3).all()


# ------------------------------------------------------------------------------------ 11. the loop
def _loop_by_hand(problem, x0, xf, U0, W, u_lim):
    """The receding-horizon loop from the pieces that existed before the team advance: solve_scenarios_distributed(policy=True),
    DistributedPolicy.rollout with one sample and W padded to the horizon, the NumPy shift."""
    from dpilqr_amd.device import to_dev
    from dpilqr_amd.dispatch import solve_scenarios_distributed
    from dpilqr_amd.lowering import describe
    d = describe(problem)
    S, n, N, h = x0.shape[0], x0.shape[1], atc.N_LOOP, atc.H_LOOP
    xf_d = to_dev(xf)
    x, U, X = x0.copy(), U0.copy(), None
    Xe, Ue = [x0[:, None].copy()], []
    for r in range(atc.L_LOOP // h):
        Wp = np.zeros((S, 1, N, n)); Wp[:, 0, :h] = W[:, r * h:(r + 1) * h]
        Xin = x[:, None, :] if X is None else X
        Xd, Ud, _, info = solve_scenarios_distributed(problem, Xin, U, atc.RADIUS, xf=xf_d, device_out=True, desc=d, policy=True, policy_mu=0.0)
        Xp, Up = Xd.cpu().numpy(), Ud.cpu().numpy()
        out = _host(info["policy"].rollout(x[:, None], W=Wp, u_lim=u_lim, trajectories=True))
        Xe.append(out["X"][:, 0, 1:h + 1]); Ue.append(out["U"][:, 0, :h])
        x = out["X"][:, 0, h].copy()
        nxt = [ac.shift(Xp[s], Up[s], x[s], h) for s in range(S)]
        U, X = np.stack([v[0] for v in nxt]), np.stack([v[1] for v in nxt])
    return np.concatenate(Xe, axis=1), np.concatenate(Ue, axis=1)


def test_the_loop_is_the_loop_written_by_hand(monkeypatch):
    import dpilqr_amd as dp
    from dpilqr_amd.batch import ProblemBatch
    x0, xf, U0, W = atc.loop_inputs()
    problem = atc.loop_problem(xf[0])
    S, L, h, n, m = atc.S_LOOP, atc.L_LOOP, atc.H_LOOP, atc.K_AG * atc.NS, atc.K_AG * atc.NC
    entries = []
    for name in ("policy_advance_dec", "policy_advance_dec_team"):
        real = getattr(ProblemBatch, name)
        monkeypatch.setattr(ProblemBatch, name, (lambda real, name: lambda self, *a, **kw: (entries.append((name, a[2] is not None)), real(self, *a, **kw))[1])(real, name))
    kw = dict(radius=atc.RADIUS, xf=xf, U0=U0, centralized=False, team=True, step_size=h, dist_converge=1e-3, max_steps=L)
    free = np.stack(dp.solve_rhc_closed_loop(problem, x0, atc.N_LOOP, W=W, **kw)["U"]).reshape(-1, m)
    u_lim = np.stack([np.quantile(free, q, axis=0) for q in pc.QUANTILES])      # as tests/policy_cases.py draws the limits
    entries.clear()
    got = dp.solve_rhc_closed_loop(problem, x0, atc.N_LOOP, W=W, u_lim=u_lim, **kw)
    assert entries == [("policy_advance_dec_team", True)] * (L // h)      # the team advance was the entry called, once per round, with gains
    Xh, Uh = _loop_by_hand(problem, x0, xf, U0, W, u_lim)
    assert (got["n_rounds"] == L // h).all() and not got["converged"].any()      # 1e-3 is not reached in four steps
    X, U = np.stack(got["X"]), np.stack(got["U"])
    assert X.shape == (S, L + 1, n) and U.shape == (S, L, m)
    bound = (U == u_lim[0]) | (U == u_lim[1])
    assert bound.any() and not bound.all()      # the limits bind somewhere, not everywhere
    for r in range(L // h):
        sl = slice(r * h, (r + 1) * h)
        print(f"round {r}: X {relerr(X[:, sl.stop], Xh[:, sl.stop]):.3g} U {relerr(U[:, sl], Uh[:, sl]):.3g}")
    assert np.array_equal(X, Xh) and np.array_equal(U, Uh)
    # the realised cost: the executed stage costs plus the terminal cost of the final state
    pb = dp.ProblemBatch([0] * atc.K_AG, [2] * atc.K_AG, xf, atc.Q, atc.R, atc.QF, atc.PROX_RADIUS, atc.DT, L)
    J = pb.cost(X[:, :-1], U).cpu().numpy().sum(axis=1) + pb.cost(X[:, -1:], np.zeros((S, 1, m)), terminal=True).cpu().numpy()[:, 0]
    assert np.all(np.abs(got["J"] - J) <= pc.TOL_ROLLOUT * np.abs(J)), np.max(np.abs(got["J"] - J) / np.abs(J))
    e = (X[:, -1] - xf).reshape(S, atc.K_AG, atc.NS)[:, :, :2]
    assert relerr(got["goal_dist"], np.sqrt((e * e).sum(axis=2))) <= pc.TOL_ROLLOUT
    sep = np.array([min(tc.separation(X[s, t], atc.K_AG, atc.NS, [2] * atc.K_AG) for t in range(L + 1)) for s in range(S)])
    assert relerr(got["min_sep"], sep) <= pc.TOL_ROLLOUT
    # feedback=False under the same disturbance executes the plans open loop: the gains are not silently dropped above
    entries.clear()
    open_ = dp.solve_rhc_closed_loop(problem, x0, atc.N_LOOP, W=W, u_lim=u_lim, feedback=False, **kw)
    assert entries == [("policy_advance_dec_team", False)] * (L // h)
    assert not np.array_equal(np.stack(open_["U"]), U)
    assert np.array_equal(np.stack(open_["U"])[:, 0], U[:, 0])      # x = X[0] at the first step: K dx = 0


# ------------------------------------------------------------------------------------ 12. an ideal plant
@pytest.mark.parametrize("feedback", [True, False])
def test_an_ideal_plant_is_solve_rhc_scenarios_first_round(feedback):
    """W = None, u_lim = None: the plant follows the plan, so the first round's executed states are solve_rhc_scenarios'."""
    import dpilqr_amd as dp
    x0, xf, U0, _ = atc.loop_inputs()
    S, h, n = atc.S_LOOP, atc.H_LOOP, atc.K_AG * atc.NS
    problem = atc.loop_problem(xf[0])
    got = dp.solve_rhc_closed_loop(problem, x0, atc.N_LOOP, radius=atc.RADIUS, xf=xf, U0=U0, centralized=False, team=True, feedback=feedback,
                                   step_size=h, dist_converge=1e-3, max_steps=h)
    assert got["converged"].tolist() == [False] * S and (got["n_rounds"] == 1).all()
    want = dp.solve_rhc_scenarios(problem, x0, atc.N_LOOP, atc.RADIUS, xf=xf, U0=U0, centralized=False, step_size=h, dist_converge=1e-3,
                                  t_diverge=1e-9)      # two rounds: the second one's first state is where the first one ended
    worst = max(max(relerr(got["X"][s], want[s][0][:h + 1]), relerr(got["U"][s], want[s][1][:h])) for s in range(S))
    print(f"feedback={feedback}: worst {worst:.3g}, largest executed control {max(np.abs(got['U'][s]).max() for s in range(S)):.3g}")
    for s in range(S):
        assert np.abs(got["U"][s]).max() > 10 * np.abs(U0[s]).max()      # the round's solve moved the plan: not the warm start executed
        assert got["X"][s].shape == (h + 1, n) and want[s][0].shape[0] >= h + 1
        assert relerr(got["X"][s], want[s][0][:h + 1]) <= pc.TOL_ROLLOUT, (s, relerr(got["X"][s], want[s][0][:h + 1]))
        assert relerr(got["U"][s], want[s][1][:h]) <= pc.TOL_ROLLOUT, (s, relerr(got["U"][s], want[s][1][:h]))
