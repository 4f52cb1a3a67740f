"""The receding-horizon advance of a team of up to 256 agents (dpilqr_policy_advance_dec_wide, csrc/policy_advance_dec_team.hpp at four mask words)
on the GPU, the cost of a point of such a team (dpilqr_cost_eval_wide), and the distributed loop built on them
(solve_rhc_closed_loop(centralized=False, wide=True)).

Cases: tests/policy_dec_wide_cases.py, every (item, sample) one scenario with the item's plan repeated
(tests/policy_advance_dec_wide_cases.py); the kernel gets the compact gains with every unused column NaN.
  prefix      X_exec / U_exec bit for bit against the rollout it restates (ProblemBatch.policy_rollout_dec_wide); scenarios not
              named keep every bit
  reference   J_exec, min_sep, dist_left against the CPU reference's prefix within the sample's own bound
  shift       against its NumPy definition; two calls equal one; the capacity; entries of scen out of range; open loop; columns
              never read; NaN containment
  one word    on the cases of tests/policy_dec_team_cases.py and its cross cases, masks reshaped to (B, k, 1): all nine fields
              equal policy_advance_dec_team's bit for bit
  cost_wide   equals cost bit for bit at k <= 64; against the oracle's Problem.cost at k = 65 and 256
  loop        65 double integrators: solve_rhc_closed_loop(wide=True) against the loop written from the pieces that existed
              before it; on the 24-agent loop of the team advance, wide=True against team=True bit for bit"""
import numpy as np
import pytest

from tests import policy_advance_cases as ac
from tests import policy_advance_dec_team_cases as atc
from tests import policy_advance_dec_wide_cases as awc
from tests import policy_cases as pc
from tests import policy_dec_cases as dc
from tests import policy_dec_team_cases as tc
from tests import policy_dec_wide_cases as wc
from tests import swarm_cases as sw
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

B, T = pc.B, pc.T
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


def _unnamed(scen, n_state):
    return np.setdiff1d(np.arange(n_state), scen)


_SETUP, _ROLL, _ADV = {}, {}, {}


def setup(case):
    if case.id not in _SETUP:
        ref = wc.case_ref(case)
        rp = awc.repeated(case, ref)
        assert np.isnan(rp["Kc"]).any()
        _SETUP[case.id] = (ref, rp, awc.problem_batch(case, ref.batch, rp["item"]), ac.scen_of(case, rp["n"]))
    return _SETUP[case.id]


def rollout(case, variant):
    """The kernel the advance's arithmetic is: policy_rollout_dec_wide on the case's own batch, every kept sample's trajectory."""
    if (case.id, variant) not in _ROLL:
        ref = wc.case_ref(case)
        W, lim = ref.args(variant)
        r = _host(awc.problem_batch(case, ref.batch, np.arange(B)).policy_rollout_dec_wide(ref.X, ref.U, ref.Kc, ref.words, ref.batch["x0s"], W=W,
                                                                                           u_lim=lim, trajectories=True))
        _ROLL[(case.id, variant)] = {k_: v.reshape((B * case.S,) + v.shape[2:])[awc.kept(case)] for k_, v in r.items()}
    return _ROLL[(case.id, variant)]


def advance(case, variant, h, gains=True):
    """One launch of all the case's scenarios through a non-identity scen into a NaN-filled state with spare scenarios."""
    key = (case.id, variant, h, gains)
    if key not in _ADV:
        ref, rp, pb, scen = setup(case)
        n_state = rp["n"] + awc.SPARE
        _, lim = ref.args(variant)
        st = _nan_state(pb, n_state, T, scen, rp["x0"])
        W = _state_W(rp["W"], scen, n_state, T) if variant == "W" else None
        pb.policy_advance_dec_wide(rp["X"], rp["U"], rp["Kc"] if gains else None, rp["words"] if gains else None, h, st, scen=scen, W=W,
                                   u_lim=lim, n_d=awc.N_D)
        _ADV[key] = _host(st)
    return _ADV[key]


# ------------------------------------------------------------------------------------ 1. bit-equal to the rollout it restates
@pytest.mark.parametrize("h", awc.HS)
@pytest.mark.parametrize("variant", awc.VARIANTS)
@pytest.mark.parametrize("case", awc.CASES, ids=awc.IDS)
def test_executed_prefix_is_the_wide_rollouts(case, variant, h):
    ref, rp, pb, scen = setup(case)
    roll, st = rollout(case, variant), advance(case, variant, h)
    assert np.isfinite(roll["X"]).all() and np.isfinite(roll["U"]).all()
    assert np.array_equal(st["X_exec"][scen, :h + 1], roll["X"][:, :h + 1])
    assert np.array_equal(st["U_exec"][scen, :h], roll["U"][:, :h])
    assert np.array_equal(st["x_cur"][scen], roll["X"][:, h])
    assert (st["n_done"][scen] == h).all()
    assert np.isnan(st["X_exec"][scen, h + 1:]).all() and np.isnan(st["U_exec"][scen, h:]).all()      # nothing past the executed steps
    rest = _unnamed(scen, rp["n"] + awc.SPARE)
    assert len(rest) == awc.SPARE and (st["n_done"][rest] == 0).all()
    for f in FIELDS:
        if f != "n_done":
            assert np.isnan(st[f][rest]).all(), f      # scenarios not named keep their NaN


# ------------------------------------------------------------------------------------ 2. against the CPU reference, per scenario
def worst_against_reference(case, variant, h, st, scen, rp):
    """(largest error / bound, largest error, its bound, scenarios without a bound, failures)."""
    ref = wc.case_ref(case)
    worst, at, unchecked, failures = 0.0, (0.0, 0.0), 0, []
    for q in range(rp["n"]):
        i, s = int(rp["item"][q]), int(rp["sample"][q])
        bound = pc.bound_of(ref.spread[variant][i, s])
        if bound is None:
            unchecked += 1
            continue
        d = awc.scenario_error(st, scen[q], *awc.prefix(case, ref, variant, i, s, h))
        if d / bound >= worst:
            worst, at = d / bound, (d, bound)
        if not d <= bound:
            failures.append((i, s, d, bound))
    return worst, at[0], at[1], unchecked, failures


@pytest.mark.parametrize("h", awc.HS)
@pytest.mark.parametrize("variant", awc.VARIANTS)
@pytest.mark.parametrize("case", awc.CASES, ids=awc.IDS)
def test_cost_separation_and_distance_against_the_reference(case, variant, h):
    ref, rp, pb, scen = setup(case)
    st = advance(case, variant, h)
    worst, d, bound, unchecked, failures = worst_against_reference(case, variant, h, st, scen, rp)
    print(f"{case.id} {variant} h={h}: worst error / bound {worst:.3g} (error {d:.3g}, bound {bound:.3g}), unchecked {unchecked} of {rp['n']}")
    assert unchecked <= pc.MAX_UNCHECKED * rp["n"], (unchecked, rp["n"])
    assert not failures, failures[:5]
    assert np.isfinite(st["J_exec"][scen]).all() and np.isfinite(st["min_sep"][scen]).all()


# ------------------------------------------------------------------------------------ 3. the shift
@pytest.mark.parametrize("h", (1, 3, T))
@pytest.mark.parametrize("case", awc.CASES, ids=awc.IDS)
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
@pytest.mark.parametrize("case", awc.CASES, ids=awc.IDS)
def test_two_calls_equal_one(case):
    """h = 1, then h = 2 on the plan sliced from step 1 (padded on the host), W read at the global step, under limits too,
    against one call of h = 3: the offsets n_done gives into W and the executed buffers, one addition per step into J_exec."""
    ref, rp, pb, scen = setup(case)
    n_state, L = rp["n"] + awc.SPARE, 5
    W = _state_W(rp["W"], scen, n_state, L)
    fresh = lambda: _nan_state(pb, n_state, L, scen, rp["x0"])
    kw = dict(scen=scen, W=W, u_lim=ref.u_lim, n_d=awc.N_D)

    one = _host(pb.policy_advance_dec_wide(rp["X"], rp["U"], rp["Kc"], rp["words"], 3, fresh(), **kw))
    st = fresh()
    pb.policy_advance_dec_wide(rp["X"], rp["U"], rp["Kc"], rp["words"], 1, st, **kw)
    pad = lambda a, last: np.concatenate([a[:, 1:], last], axis=1)
    X2, U2, K2 = pad(rp["X"], rp["X"][:, -1:]), pad(rp["U"], np.zeros_like(rp["U"][:, :1])), pad(rp["Kc"], np.zeros_like(rp["Kc"][:, :1]))
    two = _host(pb.policy_advance_dec_wide(X2, U2, K2, rp["words"], 2, st, **kw))
    for f in ("X_exec", "U_exec", "J_exec", "min_sep", "n_done", "x_cur", "dist_left"):
        assert np.array_equal(one[f][scen], two[f][scen], equal_nan=True), f      # (NaN: the rows past the three executed steps)
    assert (two["n_done"][scen] == 3).all() and np.isfinite(two["J_exec"][scen]).all()
    for j in range(rp["n"]):      # ... and the plan shifted twice is the plan shifted by three: all nine fields
        Un, Xn = ac.shift(rp["X"][j], rp["U"][j], two["x_cur"][scen[j]], 3)
        assert np.array_equal(two["U_next"][scen[j]], Un) and np.array_equal(one["U_next"][scen[j]], Un)
        assert np.array_equal(one["X_next"][scen[j]], Xn) and np.array_equal(two["X_next"][scen[j]], Xn)


# ------------------------------------------------------------------------------------ 5. the capacity, and entries of scen out of range
CAP_CASES = [awc.CASES[0], awc.CASES[1], awc.CASES[4]]      # three, two and one items per workgroup
CAP_IDS = [c.id for c in CAP_CASES]


@pytest.mark.parametrize("case", CAP_CASES, ids=CAP_IDS)
def test_the_capacity_is_never_passed(case):
    import torch
    ref, rp, pb, scen = setup(case)
    n, n_state, L = rp["n"], rp["n"] + awc.SPARE, 4
    full = scen[1::2]      # every other scenario is at its capacity already: he differs between the items of a workgroup
    st = _nan_state(pb, n_state, L, scen, rp["x0"])
    done = np.full(n_state, L - 1, dtype=np.int32); done[full] = L
    st["n_done"].copy_(torch.from_numpy(done))
    st["min_sep"].fill_(float("inf"))
    before = _host(st)
    Wn = np.full((n_state, L, pb.n_x), np.nan); Wn[scen, L - 1] = rp["W"][:, 0]
    got = _host(pb.policy_advance_dec_wide(rp["X"], rp["U"], rp["Kc"], rp["words"], 3, st, scen=scen, W=Wn, n_d=awc.N_D))
    roll = rollout(case, "W")      # one step from the same starts under the same disturbance
    short = np.arange(n)[0::2]
    assert (got["n_done"][scen] == L).all() and (got["n_done"][_unnamed(scen, n_state)] == L - 1).all()
    assert np.array_equal(got["X_exec"][scen[short], L - 1:], roll["X"][short, :2]) and np.array_equal(got["U_exec"][scen[short], L - 1], roll["U"][short, 0])
    assert np.isnan(got["X_exec"][scen[short], :L - 1]).all() and np.isnan(got["U_exec"][scen[short], :L - 1]).all()
    assert np.isfinite(got["J_exec"][scen[short]]).all()
    rest = _unnamed(scen, n_state)      # among them the scenarios that follow a named one in memory
    assert np.isnan(got["X_exec"][rest]).all() and np.isnan(got["U_exec"][rest]).all() and np.isnan(got["X_next"][rest]).all()
    for j in (0, short[-1]):
        Un, Xn = ac.shift(rp["X"][j], rp["U"][j], got["x_cur"][scen[j]], 1)      # the shift follows the executed step (he, not h)
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
    again = _host(pb.policy_advance_dec_wide(rp["X"], rp["U"], rp["Kc"], rp["words"], 2, st, scen=scen, W=Wn, n_d=awc.N_D))
    for f in ("X_exec", "U_exec", "J_exec", "min_sep", "n_done", "x_cur"):
        assert np.array_equal(again[f][scen], got[f][scen], equal_nan=True), f


def test_guard_rows_past_the_capacity_keep_their_values():
    """Through the C entry, every state tensor between two guard rows: nothing before, nothing after, and the rows past the
    executed steps keep the guard value."""
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import device, ptr, stream_handle, to_dev
    case = awc.CASES[0]
    ref, rp, pb, scen = setup(case)
    k, n_all, h, n, m = case.k, rp["n"], 3, pb.n_x, pb.n_u
    base = advance(case, "W", h)
    shapes = dict(x_cur=(n_all, n), n_done=(n_all,), X_exec=(n_all, T + 1, n), U_exec=(n_all, T, m), J_exec=(n_all,), min_sep=(n_all,),
                  dist_left=(n_all, k), U_next=(n_all, T, m), X_next=(n_all, T + 1, n))
    whole = {f: torch.full((sh[0] + 2,) + sh[1:], -7 if f == "n_done" else -7.25, dtype=torch.int32 if f == "n_done" else torch.float64,
                           device=device()) for f, sh in shapes.items()}
    view = {f: w[1:-1] for f, w in whole.items()}
    view["x_cur"].copy_(to_dev(rp["x0"])); view["n_done"].zero_(); view["J_exec"].zero_()
    dev = [to_dev(a) for a in (rp["X"], rp["U"], rp["Kc"], rp["W"])]
    bits = torch.from_numpy(np.ascontiguousarray(rp["words"]).view(np.int64)).to(device())
    _lib.check(pb._lib.dpilqr_policy_advance_dec_wide(pb._d, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), case.kc_max, ptr(bits), h, None, n_all, T, awc.N_D,
                                                      ptr(dev[3]), None, *[ptr(view[f]) for f in FIELDS], case.n_words, stream_handle()))
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


@pytest.mark.parametrize("case", CAP_CASES, ids=CAP_IDS)
def test_a_scen_entry_out_of_range_is_skipped(case):
    """Given as a device tensor, which the host does not check: the entries -1, n_state and 2^31 - 1 name nobody (the kernel
    documents this as a skip: such an item's lanes take part in the barriers and in nothing else)."""
    import torch
    from dpilqr_amd.device import to_dev
    ref, rp, pb, scen = setup(case)
    n, n_state = rp["n"], rp["n"] + awc.SPARE
    base = advance(case, "plain", 3)
    bad = scen.copy()
    skipped = [0, n // 2, n - 1]
    bad[skipped] = [-1, n_state, 2 ** 31 - 1]
    st = _nan_state(pb, n_state, T, scen, rp["x0"])
    before = _host(st)
    got = _host(pb.policy_advance_dec_wide(rp["X"], rp["U"], rp["Kc"], rp["words"], 3, st, scen=to_dev(bad, torch.int32), n_d=awc.N_D))
    keep = np.setdiff1d(np.arange(n), skipped)
    rest = _unnamed(scen, n_state)
    for f in FIELDS:
        assert np.array_equal(got[f][scen[keep]], base[f][scen[keep]], equal_nan=True), f
        assert np.array_equal(got[f][scen[skipped]], before[f][scen[skipped]], equal_nan=True), f      # untouched
        assert np.array_equal(got[f][rest], before[f][rest], equal_nan=True), f


# ------------------------------------------------------------------------------------ 6. Kc = NULL
@pytest.mark.parametrize("case", awc.CASES, ids=awc.IDS)
def test_without_gains_the_plan_is_executed_open_loop(case):
    ref, rp, pb, scen = setup(case)
    lim = ref.u_lim
    st = advance(case, "u_lim", T, gains=False)
    want = np.where(rp["U"] < lim[0], lim[0], np.where(rp["U"] > lim[1], lim[1], rp["U"]))
    assert np.array_equal(st["U_exec"][scen], want)
    free = advance(case, "plain", T, gains=False)
    assert np.array_equal(free["U_exec"][scen], rp["U"])
    # ... whatever the masks: garbage masks beside no gains change nothing (they are not read)
    n_state = rp["n"] + awc.SPARE
    st2 = _nan_state(pb, n_state, T, scen, rp["x0"])
    pb.policy_advance_dec_wide(rp["X"], rp["U"], None, np.zeros_like(rp["words"]), T, st2, scen=scen, n_d=awc.N_D)
    st2 = _host(st2)
    for f in FIELDS:
        assert np.array_equal(st2[f], free[f], equal_nan=True), f
    assert not np.array_equal(free["U_exec"][scen], advance(case, "plain", T)["U_exec"][scen])      # the gains do something


# ------------------------------------------------------------------------------------ 7. columns never read
@pytest.mark.parametrize("case", [awc.CASES[0], awc.CASES[5]], ids=[awc.IDS[0], awc.IDS[5]])
def test_columns_past_a_neighbourhood_are_never_read(case):
    ref, rp, pb, scen = setup(case)
    base = advance(case, "u_lim", 3)      # NaN there
    zero = awc.repeated(case, ref, fill=0.0)
    assert not np.isnan(zero["Kc"]).any() and np.isnan(rp["Kc"]).any()
    st = _nan_state(pb, rp["n"] + awc.SPARE, T, scen, rp["x0"])
    got = _host(pb.policy_advance_dec_wide(rp["X"], rp["U"], zero["Kc"], rp["words"], 3, st, scen=scen, u_lim=ref.u_lim, n_d=awc.N_D))
    for f in FIELDS:
        assert np.array_equal(got[f], base[f], equal_nan=True), f
    for f in FIELDS:      # every result of the named scenarios is finite (the rows past the executed steps aside)
        v = base[f][scen]
        v = v[:, :4] if f == "X_exec" else v[:, :3] if f == "U_exec" else v
        assert np.isfinite(v).all(), f


# ------------------------------------------------------------------------------------ 8. NaN containment
def test_nan_poisons_only_its_scenario():
    case = awc.CASES[0]      # three items per workgroup
    ref, rp, pb, scen = setup(case)
    base = advance(case, "u_lim", 3)
    n_state = rp["n"] + awc.SPARE
    x0 = rp["x0"].copy()
    poisoned = [1, 3]      # slot 1 of the first workgroup, slot 0 of the second
    x0[poisoned] = np.nan
    st = _nan_state(pb, n_state, T, scen, x0)
    got = _host(pb.policy_advance_dec_wide(rp["X"], rp["U"], rp["Kc"], rp["words"], 3, st, scen=scen, u_lim=ref.u_lim, n_d=awc.N_D))
    clean = np.setdiff1d(np.arange(rp["n"]), poisoned)
    for f in FIELDS:
        assert np.array_equal(got[f][scen[clean]], base[f][scen[clean]], equal_nan=True), f
    assert np.isfinite(base["J_exec"][scen]).all()
    assert np.isnan(got["J_exec"][scen[poisoned]]).all() and np.isnan(got["X_exec"][scen[poisoned], :4]).all()
    assert (got["n_done"][scen[poisoned]] == 3).all()


# ------------------------------------------------------------------------------------ 9. n_words = 1: the team advance, bit for bit
ONE_WORD = [(c, tc.case_ref) for c in tc.CASES] + [(c, dc.case_ref) for c in tc.CROSS]


def one_word_differences(case, case_ref):
    """{(variant, h): the fields on which the wide entry with n_words = 1 differs from policy_advance_dec_team} (all empty: equal)."""
    ref = case_ref(case)
    rp = atc.repeated(case, ref)
    pb, scen = ac.problem_batch(case, ref.batch, repeat=case.S), ac.scen_of(case, rp["n"])
    n_state = rp["n"] + atc.SPARE
    words = rp["masks"].reshape(rp["n"], case.k, 1)
    out = {}
    for v in atc.VARIANTS:
        _, lim = ref.args(v)
        W = _state_W(rp["W"], scen, n_state, T) if v == "W" else None
        for h in atc.HS:
            fresh = lambda: _nan_state(pb, n_state, T, scen, rp["x0"])
            kw = dict(scen=scen, W=W, u_lim=lim, n_d=atc.N_D)
            team = _host(pb.policy_advance_dec_team(rp["X"], rp["U"], rp["Kc"], rp["masks"], h, fresh(), **kw))
            wide = _host(pb.policy_advance_dec_wide(rp["X"], rp["U"], rp["Kc"], words, h, fresh(), **kw))
            assert np.isfinite(team["J_exec"][scen]).all() and (team["n_done"][scen] == h).all()
            out[v, h] = [f for f in FIELDS if not np.array_equal(team[f], wide[f], equal_nan=True)]
    return out


@pytest.mark.parametrize("case,case_ref", ONE_WORD, ids=[c.id for c, _ in ONE_WORD])
def test_one_word_equals_the_team_advance(case, case_ref):
    assert case.k <= 64
    differ = one_word_differences(case, case_ref)
    assert all(not fields for fields in differ.values()), differ


# ------------------------------------------------------------------------------------ 10. cost_wide
@pytest.mark.parametrize("case", [tc.CASES[0], tc.CASES[-1]], ids=[tc.IDS[0], tc.IDS[-1]])
def test_cost_wide_equals_cost_up_to_64_agents(case):
    ref = tc.case_ref(case)
    pb = ac.problem_batch(case, ref.batch)
    for terminal in (False, True):
        a = pb.cost(ref.X[:, :T], ref.U, terminal=terminal).cpu().numpy()
        w = pb.cost_wide(ref.X[:, :T], ref.U, terminal=terminal).cpu().numpy()
        assert a.shape == (B, T) and np.isfinite(a).all() and np.array_equal(a, w), terminal


@pytest.mark.parametrize("case", [awc.CASES[0], awc.CASES[5]], ids=[awc.IDS[0], awc.IDS[5]])
def test_cost_wide_against_the_oracle(case):
    """k = 65 and 256, at the W variant's reference states (agents inside the radius) with the reference's controls."""
    ref = wc.case_ref(case)
    pb = awc.problem_batch(case, ref.batch, np.arange(B))
    pts = (0, 1, T - 1)
    X = np.stack([[ref.ref["W"][i][0]["X"][t] for t in pts] for i in range(B)])
    U = np.stack([[ref.ref["W"][i][0]["U"][t] for t in pts] for i in range(B)])
    with pytest.raises(Exception, match="k=%d" % case.k):      # the one-word entry keeps its refusal
        pb.cost(X, U)
    for terminal in (False, True):
        got = pb.cost_wide(X, U, terminal=terminal).cpu().numpy()
        want = np.array([[float(ref.problems[i].cost(X[i, q], U[i, q], terminal=terminal)) for q in range(len(pts))] for i in range(B)])
        err = np.max(np.abs(got - want) / np.abs(want))
        print(f"{case.id} terminal={terminal}: cost_wide against the oracle {err:.3g} (tol {pc.TOL_ROLLOUT:.0e})")
        assert np.isfinite(want).all() and err <= pc.TOL_ROLLOUT, (terminal, err)
    assert not np.array_equal(pb.cost_wide(X, U).cpu().numpy(), pb.cost_wide(X, U, terminal=True).cpu().numpy())


# ------------------------------------------------------------------------------------ 11. the loop on a swarm
def _loop_by_hand(problem, x0, xf, U0, W, u_lim, feedback=True):
    """The receding-horizon loop from the pieces that existed before the wide advance: solve_scenarios_distributed(policy="wide"),
    a one-sample policy_rollout_dec_wide over the whole horizon with W padded to it, the NumPy shift and append.  Open loop
    (feedback=False): the stitched plan through the same rollout with zero gains over every agent's own state (u = U + 0)."""
    import dpilqr_amd as dp
    from dpilqr_amd.device import to_dev
    from dpilqr_amd.dispatch import solve_scenarios_distributed
    from dpilqr_amd.lowering import describe
    case = awc.LOOP_CASE
    d = describe(problem)
    S, n, N, h, k = x0.shape[0], x0.shape[1], awc.N_LOOP, awc.H_LOOP, case.k
    xf_d = to_dev(np.tile(xf[None], (S, 1)))
    x, U, X = x0.copy(), U0.copy(), None
    Xe, Ue = [x0[:, None].copy()], []
    Q, R, Qf = sw.weights(case)
    pb = dp.ProblemBatch([case.model] * k, [case.n_d] * k, np.tile(xf[None], (S, 1)), Q, R, Qf, sw.RADIUS, sw.DT, N)
    for r in range(awc.L_LOOP // h):
        Wp = np.zeros((S, 1, N, n)); Wp[:, 0, :h] = W[:, r * h:(r + 1) * h]
        Xin = x[:, None, :] if X is None else X
        Xd, Ud, _, info = solve_scenarios_distributed(problem, Xin, U, sw.RADIUS, xf=xf_d, device_out=True, desc=d,
                                                      policy="wide" if feedback else False, policy_mu=0.0)
        Xp, Up = Xd.cpu().numpy(), Ud.cpu().numpy()
        if feedback:
            out = _host(info["policy"].rollout(x[:, None], W=Wp, u_lim=u_lim, trajectories=True))
        else:
            own = wc.words_of([[[a] for a in range(k)]] * S, k)
            out = _host(pb.policy_rollout_dec_wide(Xp, Up, np.zeros((S, N, k, case.nc, case.ns)), own, x[:, None], W=Wp, u_lim=u_lim, trajectories=True))
        Xe.append(out["X"][:, 0, 1:h + 1]); Ue.append(out["U"][:, 0, :h])
        x = out["X"][:, 0, h].copy()
        nxt = [ac.shift(Xp[s], Up[s], x[s], h) for s in range(S)]
        U, X = np.stack([v[0] for v in nxt]), np.stack([v[1] for v in nxt])
    return np.concatenate(Xe, axis=1), np.concatenate(Ue, axis=1), pb


def test_the_loop_on_a_swarm_is_the_loop_written_by_hand(monkeypatch):
    import dpilqr_amd as dp
    from dpilqr_amd.batch import ProblemBatch
    case = awc.LOOP_CASE
    x0, xf, U0, W = awc.loop_inputs()
    problem = awc.loop_problem(xf)
    S, L, h, k, n, m = awc.S_LOOP, awc.L_LOOP, awc.H_LOOP, case.k, case.k * case.ns, case.k * case.nc
    entries = []
    for name in ("policy_advance_dec", "policy_advance_dec_team", "policy_advance_dec_wide", "cost", "cost_wide"):
        real = getattr(ProblemBatch, name)
        flag = (lambda a, kw: kw.get("terminal", False)) if name.startswith("cost") else (lambda a, kw: a[2] is not None)
        monkeypatch.setattr(ProblemBatch, name, (lambda real, name, flag: lambda self, *a, **kw: (entries.append((name, flag(a, kw))), real(self, *a, **kw))[1])(real, name, flag))
    kw = dict(radius=sw.RADIUS, U0=U0, centralized=False, wide=True, step_size=h, dist_converge=1e-3, max_steps=L)
    with pytest.raises(ValueError, match=r"^solve_rhc_closed_loop is not built for teams of more than 64 agents \(this one has 65\)$"):
        dp.solve_rhc_closed_loop(problem, x0, awc.N_LOOP, W=W, **dict(kw, wide=False, team=True))
    free = np.stack(dp.solve_rhc_closed_loop(problem, x0, awc.N_LOOP, W=W, **kw)["U"]).reshape(-1, m)
    u_lim = np.stack([np.quantile(free, q, axis=0) for q in pc.QUANTILES])      # as tests/policy_cases.py draws the limits
    entries.clear()
    got = dp.solve_rhc_closed_loop(problem, x0, awc.N_LOOP, W=W, u_lim=u_lim, **kw)
    assert entries == [("policy_advance_dec_wide", True)] * (L // h) + [("cost_wide", True)]      # one launch per round, with gains
    Xh, Uh, pb = _loop_by_hand(problem, x0, xf, U0, W, u_lim)
    assert (got["n_rounds"] == L // h).all() and not got["converged"].any()      # 1e-3 is not reached in four steps
    X, U = np.stack(got["X"]), np.stack(got["U"])
    assert X.shape == (S, L + 1, n) and U.shape == (S, L, m)
    bound = (U == u_lim[0]) | (U == u_lim[1])
    assert bound.any() and not bound.all()      # the limits bind somewhere, not everywhere
    for r in range(L // h):
        sl = slice(r * h, (r + 1) * h)
        print(f"round {r}: X {relerr(X[:, sl.stop], Xh[:, sl.stop]):.3g} U {relerr(U[:, sl], Uh[:, sl]):.3g}")
    assert np.array_equal(X, Xh) and np.array_equal(U, Uh)
    # the realised cost: the executed stage costs plus the terminal cost of the final state, on the CPU
    p = sw.oracle_problem(case, xf)
    J = np.array([sum(float(p.cost(X[s, t], U[s, t])) for t in range(L)) + float(p.cost(X[s, L], np.zeros(m), terminal=True)) for s in range(S)])
    eJ = np.max(np.abs(got["J"] - J) / np.abs(J))
    e = (X[:, -1] - xf[None]).reshape(S, k, case.ns)[:, :, :2]
    sep = np.array([min(tc.separation(X[s, t], k, case.ns, [2] * k) for t in range(L + 1)) for s in range(S)])
    eG, eS = relerr(got["goal_dist"], np.sqrt((e * e).sum(axis=2))), relerr(got["min_sep"], sep)
    print(f"J {eJ:.3g}, goal_dist {eG:.3g}, min_sep {eS:.3g} (tol {pc.TOL_ROLLOUT:.0e}, the team loop's own; 1e-9 is asked)")
    assert eJ <= pc.TOL_ROLLOUT <= 1e-9 and eG <= pc.TOL_ROLLOUT and eS <= pc.TOL_ROLLOUT
    # feedback=False under the same disturbance executes the stitched plans open loop
    entries.clear()
    open_ = dp.solve_rhc_closed_loop(problem, x0, awc.N_LOOP, W=W, u_lim=u_lim, feedback=False, **kw)
    assert entries == [("policy_advance_dec_wide", False)] * (L // h) + [("cost_wide", True)]
    Xo, Uo, _ = _loop_by_hand(problem, x0, xf, U0, W, u_lim, feedback=False)
    assert np.array_equal(np.stack(open_["X"]), Xo) and np.array_equal(np.stack(open_["U"]), Uo)
    assert not np.array_equal(np.stack(open_["U"]), U)      # the gains are not silently dropped above
    assert np.array_equal(np.stack(open_["U"])[:, 0], U[:, 0])      # x = X[0] at the first step: K dx = 0


# ------------------------------------------------------------------------------------ 12. one word: the team loop
@pytest.mark.parametrize("feedback", [True, False])
def test_the_loop_with_one_word_is_the_team_loop(feedback):
    """24 double integrators (tests/policy_advance_dec_team_cases.py): every stage -- front end, stitch, advance, terminal cost --
    is bit-identical at one word, so every returned array is."""
    import dpilqr_amd as dp
    x0, xf, U0, W = atc.loop_inputs()
    problem = atc.loop_problem(xf[0])
    kw = dict(radius=atc.RADIUS, xf=xf, U0=U0, centralized=False, step_size=atc.H_LOOP, dist_converge=1e-3, max_steps=atc.L_LOOP, W=W,
              feedback=feedback)
    free = np.stack(dp.solve_rhc_closed_loop(problem, x0, atc.N_LOOP, team=True, **kw)["U"]).reshape(-1, atc.K_AG * atc.NC)
    u_lim = np.stack([np.quantile(free, q, axis=0) for q in pc.QUANTILES])
    team = dp.solve_rhc_closed_loop(problem, x0, atc.N_LOOP, team=True, u_lim=u_lim, **kw)
    wide = dp.solve_rhc_closed_loop(problem, x0, atc.N_LOOP, wide=True, u_lim=u_lim, **kw)
    assert set(team) == set(wide) == {"X", "U", "J", "min_sep", "goal_dist", "converged", "n_rounds"}
    assert (team["n_rounds"] == atc.L_LOOP // atc.H_LOOP).all() and np.isfinite(team["J"]).all()
    for key in team:
        a, b_ = (np.stack(team[key]), np.stack(wide[key])) if key in ("X", "U") else (team[key], wide[key])
        assert np.array_equal(a, b_), key
