"""The closed-loop rollout of a distributed solution for teams of up to 256 agents (dpilqr_policy_rollout_dec_wide,
csrc/policy_dec_team.hpp at four mask words) and the stitch of its gains (dpilqr_dispatch_stitch_policy_wide) on the GPU.

  reference   per case of tests/policy_dec_wide_cases.py and variant (plain, W, u_lim), every sample against the CPU reference
              within its own bound bound_of(spread); the kernel gets the compact gains with every unused column NaN; with /
              without stored trajectories
  one word    on the cases of tests/policy_dec_team_cases.py (k = 21, 33, 64) and its cross cases (mixed models, mixed n_dims)
              the wide entry with n_words = 1 equals policy_rollout_dec_team on all five results, bit for bit
  stitch      with n_words = 1 stitch_policy_wide equals stitch_policy bit for bit on a solved team of 24; at k > 64 it equals a
              NumPy loop of the definition (the same ascending multiply-then-add) bit for bit
  position    an item gives the same bits at another place in the batch and with another number of samples, a run repeated
              gives the same bits, guard rows around every output are untouched, an item of NaN poisons only itself, NaN in the
              never-read columns changes nothing
  end to end  the solvable swarms of tests/swarm_cases.py (k = 65, 70, 130): solve_scenarios_distributed(policy="wide") ->
              policy.rollout against the definition unfolded on the CPU from the solve's own sub-problem solutions and gains; from
              the stitched start the rollout reproduces X_dec wherever every neighbour of an agent follows the plan that agent's
              own sub-problem holds for it; closed_loop_distributed(wide=True) returns scenario 0"""
import numpy as np
import pytest

from tests import linesearch_cases as lc
from tests import policy_cases as pc
from tests import policy_dec_cases as dc
from tests import policy_dec_team_cases as tc
from tests import policy_dec_wide_cases as wc
from tests import swarm_cases as sw

pytestmark = pytest.mark.gpu

B, T = pc.B, pc.T
VARIANTS = ["plain", "W", "u_lim"]
KEYS = ("X", "U", "J", "min_sep", "goal_dist")


def _pb(case, b, items=None):
    import dpilqr_amd as dp
    sel = (lambda a: a) if items is None else (lambda a: a[items])
    if case.weights == "per_item":
        Q, R, Qf = sel(b["Q"]), sel(b["R"]), sel(b["Qf"])
    else:
        Q, R, Qf = b["Q"], b["R"], b["Qf"]
    return dp.ProblemBatch(b["models"], b["n_dims"], sel(b["xf"]), Q, R, Qf, b["radius"], b["dt"], T)


def _host(r):
    return {k_: t.cpu().numpy() for k_, t in r.items()}


_RUNS = {}


def gpu_runs(case):
    """The case's launches, once."""
    if case.id not in _RUNS:
        ref = wc.case_ref(case)
        b = ref.batch
        pb = _pb(case, b)
        assert np.isnan(ref.Kc).any()
        out = {}
        for v in VARIANTS:
            W, lim = ref.args(v)
            out[v] = _host(pb.policy_rollout_dec_wide(ref.X, ref.U, ref.Kc, ref.words, b["x0s"], W=W, u_lim=lim, trajectories=True))
            out[v + "-nostore"] = _host(pb.policy_rollout_dec_wide(ref.X, ref.U, ref.Kc, ref.words, b["x0s"], W=W, u_lim=lim))
        _RUNS[case.id] = out
    return _RUNS[case.id]


def worst_against_reference(case, variant, got):
    """(largest error / bound, largest error, its bound, unchecked samples, failures) over the case's samples."""
    ref = wc.case_ref(case)
    worst, at, unchecked, failures = 0.0, (0.0, 0.0), 0, []
    for i in range(B):
        for s in range(case.S):
            bound = pc.bound_of(ref.spread[variant][i, s])
            if bound is None:
                unchecked += 1
                continue
            g = dict(X=got["X"][i, s], U=got["U"][i, s], J=float(got["J"][i, s]), min_sep=float(got["min_sep"][i, s]),
                     goal_dist=got["goal_dist"][i, s])
            d = pc.difference(g, ref.ref[variant][i][s])
            if d / bound >= worst:
                worst, at = d / bound, (d, bound)
            if not d <= bound:
                failures.append((i, s, d, bound))
    return worst, at[0], at[1], unchecked, failures


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_against_reference(case, variant):
    got = gpu_runs(case)[variant]
    worst, d, bound, unchecked, failures = worst_against_reference(case, variant, got)
    print(f"{case.id} {variant}: worst error / bound {worst:.3g} (error {d:.3g}, bound {bound:.3g}), unchecked {unchecked} of {B * case.S}")
    assert unchecked <= pc.MAX_UNCHECKED * B * case.S, (unchecked, B * case.S)
    assert not failures, failures[:5]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_not_storing_trajectories_changes_nothing(case, variant):
    runs = gpu_runs(case)
    a, b_ = runs[variant], runs[variant + "-nostore"]
    assert set(a) == set(KEYS) and set(b_) == {"J", "min_sep", "goal_dist"}
    for key in b_:
        assert np.array_equal(a[key], b_[key]), key


# ---- n_words = 1: the team kernel's results, bit for bit
ONE_WORD = [(c, tc.case_ref) for c in tc.CASES] + [(c, dc.case_ref) for c in tc.CROSS]


def one_word_equal(case, case_ref):
    """{variant: the keys on which the wide entry with n_words = 1 differs from policy_rollout_dec_team} (all empty: equal)."""
    ref = case_ref(case)
    b, k = ref.batch, case.k
    pb = _pb(case, b)
    Kc = dc.compact_gains(ref.K, ref.masks, case.ns, case.nc, k)
    words = ref.masks.reshape(B, k, 1)
    out = {}
    for v in VARIANTS:
        W, lim = ref.args(v)
        team = _host(pb.policy_rollout_dec_team(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
        wide = _host(pb.policy_rollout_dec_wide(ref.X, ref.U, Kc, words, b["x0s"], W=W, u_lim=lim, trajectories=True))
        assert set(team) == set(wide) == set(KEYS) and np.isfinite(team["J"]).all()
        out[v] = [key for key in KEYS if not np.array_equal(team[key], wide[key])]
    return out


@pytest.mark.parametrize("case,case_ref", ONE_WORD, ids=[c.id for c, _ in ONE_WORD])
def test_one_word_equals_the_team_kernel(case, case_ref):
    assert case.k <= 64
    differ = one_word_equal(case, case_ref)
    assert all(not keys for keys in differ.values()), differ


# ---- the stitch
def _team24():
    from tests import test_gpu_policy_dec_team as tt
    return tt


_NARROW = {}


def narrow_pair():
    """The 24-agent scenarios of tests/test_gpu_policy_dec_team.py solved twice: policy=True and policy='wide'."""
    if not _NARROW:
        import dpilqr_amd as dp
        tt = _team24()
        for pol in (True, "wide"):
            X_dec, U_dec, J, info = dp.solve_scenarios_distributed(tt._problem(), tt.X0[:, None, :], np.zeros((tt.S_E2E, T, tt.K_AG * tt.NC)),
                                                                   tt.RADIUS, xf=tt.XF, policy=pol, policy_mu=tt.MU, n_lqr_iter=20)
            _NARROW[pol] = dict(X_dec=X_dec, U_dec=U_dec, J=J, info=info, pol=info["policy"])
    return _NARROW[True], _NARROW["wide"]


def test_stitch_with_one_word_equals_the_narrow_stitch():
    tt = _team24()
    a, w = narrow_pair()
    assert np.array_equal(a["X_dec"], w["X_dec"]) and np.array_equal(a["U_dec"], w["U_dec"]) and np.array_equal(a["J"], w["J"])
    assert w["info"]["cluster_bits"].shape == (tt.S_E2E, tt.K_AG, 1) and a["info"]["cluster_bits"].shape == (tt.S_E2E, tt.K_AG)
    assert np.array_equal(a["info"]["cluster_bits"], w["info"]["cluster_bits"][:, :, 0])
    pa, pw = a["pol"], w["pol"]
    assert pw.wide and not pa.wide and pa.kc_max == pw.kc_max == 6 and tuple(pw.bits.shape) == (tt.S_E2E, tt.K_AG, 1)
    assert np.array_equal(pa.Kc.cpu().numpy(), pw.Kc.cpu().numpy()) and np.array_equal(pa.U_ff.cpu().numpy(), pw.U_ff.cpu().numpy())
    # ... and so does the rollout: the team kernel against the wide one
    x0s = tt._starts()
    rng = np.random.default_rng(5)
    W = pc.W_SCALE * rng.normal(size=(tt.S_E2E, tt.N_STARTS, T, tt.K_AG * tt.NS))
    ra, rw = _host(pa.rollout(x0s, W=W, trajectories=True)), _host(pw.rollout(x0s, W=W, trajectories=True))
    for key in KEYS:
        assert np.array_equal(ra[key], rw[key]), key
    with pytest.raises(ValueError, match="the wide advance is not built"):
        pw.advance(1, {})


_SWARM = {}


def swarm(case):
    """solve_scenarios_distributed(policy='wide', audit=True) of a solvable swarm, once."""
    if case.id not in _SWARM:
        import dpilqr_amd as dp
        from tests.test_gpu_swarm import dp_problem
        x0s, xf, U0 = sw.scenario(case, sw.OFFSET_SOLVE)
        prob = dp_problem(dp, case, xf)
        U0s = np.tile(U0[None], (sw.S, 1, 1))
        X_dec, U_dec, J, info = dp.solve_scenarios_distributed(prob, x0s[:, None, :], U0s, sw.RADIUS, audit=True, policy="wide", policy_mu=pc.MU,
                                                               n_lqr_iter=sw.N_LQR_ITER)
        masks = sw.words_to_masks(info["cluster_bits"])
        _SWARM[case.id] = dict(X_dec=X_dec, U_dec=U_dec, J=J, info=info, pol=info["policy"], masks=masks, x0s=x0s, xf=xf, U0=U0, prob=prob)
    return _SWARM[case.id]


def _members(mask, k):
    return [j for j in range(k) if (int(mask) >> j) & 1]


def owners(masks, k):
    """(bucket size, slot, members, pos) of every (s, i): representatives in (s, i) order inside their size's bucket."""
    count, slot_of, out = {}, {}, {}
    for s in range(masks.shape[0]):
        for i in range(k):
            key = (s, int(masks[s, i]))
            if key not in slot_of:
                kc = len(_members(masks[s, i], k))
                slot_of[key] = count.get(kc, 0)
                count[kc] = slot_of[key] + 1
    for s in range(masks.shape[0]):
        for i in range(k):
            mem = _members(masks[s, i], k)
            out[s, i] = (len(mem), slot_of[s, int(masks[s, i])], mem, mem.index(i))
    return out


def stitch_definition(r, case):
    """Kc and U_ff of include/dpilqr_policy.h's definition in NumPy: the columns ascending, one multiply and one add per term."""
    k, ns, nc, Tn = case.k, case.ns, case.nc, case.T
    aud, own, kc_max = r["info"]["audit"], owners(r["masks"], k), r["pol"].kc_max
    Kc = np.zeros((sw.S, Tn, k, nc, kc_max * ns)); U_ff = np.zeros((sw.S, Tn, k * nc))
    for s in range(sw.S):
        for i in range(k):
            kc, slot, mem, pos = own[s, i]
            Xi, Ui, Ki = aud[kc]["X"][slot], aud[kc]["U"][slot], aud[kc]["K"][slot]
            rows = Ki[:, pos * nc:(pos + 1) * nc, :]                       # (T, n_c, kc n_s)
            Kc[s, :, i, :, :kc * ns] = rows
            cols = np.concatenate([np.arange(j * ns, (j + 1) * ns) for j in mem])
            diff = r["X_dec"][s][:Tn][:, cols] - Xi[:Tn]                   # (T, kc n_s)
            acc = np.zeros((Tn, nc))
            for col in range(kc * ns):
                acc = acc + rows[:, :, col] * diff[:, col][:, None]
            U_ff[s, :, i * nc:(i + 1) * nc] = Ui[:, pos * nc:(pos + 1) * nc] + acc
    return Kc, U_ff


@pytest.mark.parametrize("case", sw.SOLVE_CASES[:2], ids=lambda c: c.id)
def test_stitch_of_a_wide_team_equals_the_definition(case):
    r = swarm(case)
    pol, k = r["pol"], case.k
    assert pol.wide and tuple(pol.bits.shape) == (sw.S, k, case.n_words) and r["info"]["cluster_bits"].shape == (sw.S, k, case.n_words)
    sizes = {len(_members(m, k)) for m in r["masks"].reshape(-1)}
    assert pol.kc_max == max(sizes) >= 2 and any(min(_members(m, k)) < 64 <= max(_members(m, k)) for m in r["masks"].reshape(-1))
    Kc, U_ff = stitch_definition(r, case)
    assert np.array_equal(pol.Kc.cpu().numpy(), Kc)
    assert np.array_equal(pol.U_ff.cpu().numpy(), U_ff)


# ---- position independence
POS_CASE = wc.CASES[0]      # 65 agents, two words, 3 samples per workgroup


def _guarded(S, k, n, m, Bn):
    """Outputs with a guard row of NaN before and after, handed to the C entry directly: (views, whole buffers)."""
    import torch
    from dpilqr_amd.device import device
    shapes = dict(X=(Bn * S, T + 1, n), U=(Bn * S, T, m), J=(Bn * S,), min_sep=(Bn * S,), goal_dist=(Bn * S, k))
    whole = {key: torch.full((sh[0] + 2,) + sh[1:], float("nan"), dtype=torch.float64, device=device()) for key, sh in shapes.items()}
    return {key: w[1:-1] for key, w in whole.items()}, whole


def test_position_independence_and_guards():
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle, to_dev
    case = POS_CASE
    ref = wc.case_ref(case)
    b, k, ns, nc, S = ref.batch, case.k, case.ns, case.nc, case.S
    n, m = k * ns, k * nc
    full = gpu_runs(case)["W"]
    assert all(np.isfinite(full[key]).all() for key in full)
    # a run repeated: the same bits
    again = _host(_pb(case, b).policy_rollout_dec_wide(ref.X, ref.U, ref.Kc, ref.words, b["x0s"], W=b["W"], trajectories=True))
    for key in full:
        assert np.array_equal(full[key], again[key]), key
    # item 2 at place 0 of a batch of two, two of its samples in another order: another chunk, another workgroup, another S;
    # one item alone; an item at the end of the batch
    for items, smp in (([2, 0], [3, 0]), ([1], [0, 1, 2, 3]), ([0, 1, 2], [2])):
        r = _host(_pb(case, b, items).policy_rollout_dec_wide(ref.X[items], ref.U[items], ref.Kc[items], ref.words[items], b["x0s"][items][:, smp],
                                                              W=b["W"][items][:, smp], trajectories=True))
        for key in full:
            assert np.array_equal(r[key], full[key][items][:, smp]), (items, key)
    # guard rows around every output, through the C entry
    pb = _pb(case, b)
    view, whole = _guarded(S, k, n, m, B)
    dev = [to_dev(a) for a in (ref.X, ref.U, ref.Kc, b["x0s"], b["W"])]
    bits = torch.from_numpy(ref.words.view(np.int64)).to(dev[0].device)
    _lib.check(pb._lib.dpilqr_policy_rollout_dec_wide(pb._d, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), case.kc_max, ptr(bits), S, ptr(dev[3]),
                                                      ptr(dev[4]), None, ptr(view["X"]), ptr(view["U"]), ptr(view["J"]), ptr(view["min_sep"]),
                                                      ptr(view["goal_dist"]), case.n_words, stream_handle()))
    torch.cuda.synchronize()
    for key, w in whole.items():
        h = w.cpu().numpy()
        assert np.isnan(h[0]).all() and np.isnan(h[-1]).all(), key
        assert np.array_equal(h[1:-1].reshape(full[key].shape), full[key]), key


def test_nan_poisons_only_its_item_and_unread_columns_nothing():
    case = POS_CASE
    ref = wc.case_ref(case)
    b = ref.batch
    full = gpu_runs(case)["u_lim"]
    pb = _pb(case, b)
    assert all(np.isfinite(full[key]).all() for key in full)
    # the never-read columns: NaN (the runs above), zero, and huge -- the same bits
    for fill in (0.0, 1e300):
        Kc = np.where(np.isnan(ref.Kc), fill, ref.Kc)
        r = _host(pb.policy_rollout_dec_wide(ref.X, ref.U, Kc, ref.words, b["x0s"], u_lim=ref.u_lim, trajectories=True))
        for key in full:
            assert np.array_equal(r[key], full[key]), (fill, key)
    # item 1 poisoned
    x0s = b["x0s"].copy()
    x0s[1] = np.nan
    r = _host(pb.policy_rollout_dec_wide(ref.X, ref.U, ref.Kc, ref.words, x0s, u_lim=ref.u_lim, trajectories=True))
    for key in full:
        assert np.array_equal(r[key][[0, 2]], full[key][[0, 2]]), key
    assert np.isnan(r["J"][1]).all() and np.isnan(r["X"][1]).all()


# ---- end to end
N_STARTS = 2


def _definition_tables(r, case, s):
    """Per agent of scenario s, stacked: its members' state columns, U^i's own rows, X^i and K^i's own rows (the solve's own)."""
    k, ns, nc, Tn = case.k, case.ns, case.nc, case.T
    aud, own, kc_max = r["info"]["audit"], owners(r["masks"], k), r["pol"].kc_max
    members = [own[s, i][2] for i in range(k)]
    idx, used = wc.gather_index(members, ns, kc_max)
    Ku = np.zeros((Tn, k, nc, kc_max * ns)); Xi_s = np.zeros((Tn, k, kc_max * ns)); Ui_s = np.zeros((Tn, k * nc))
    for i in range(k):
        kc, slot, mem, pos = own[s, i]
        Ku[:, i, :, :kc * ns] = aud[kc]["K"][slot][:, pos * nc:(pos + 1) * nc, :]
        Xi_s[:, i, :kc * ns] = aud[kc]["X"][slot][:Tn]
        Ui_s[:, i * nc:(i + 1) * nc] = aud[kc]["U"][slot][:, pos * nc:(pos + 1) * nc]
    return idx, used, Ku, Xi_s, Ui_s


def ref_definition(p, case, tables, xf, x0, W=None, u_lim=None, e=0.0):
    """The definition, unfolded: u_i = U^i[pos] + K^i[pos] (x_{C_i} - X^i); e: the relative perturbation of the sensitivity runs."""
    k, ns, nc, Tn = case.k, case.ns, case.nc, case.T
    idx, used, Ku, Xi_s, Ui_s = tables
    n_dims = [case.n_d] * k
    Xs = np.zeros((Tn + 1, k * ns)); Us = np.zeros((Tn, k * nc))
    Xs[0] = x0 * (1 + e)
    J, sep = 0.0, tc.separation(Xs[0], k, ns, n_dims)
    for t in range(Tn):
        dx = (Xs[t][idx] - Xi_s[t] * (1 + e)) * used
        u = Ui_s[t] * (1 - e) + np.einsum("acj,aj->ac", Ku[t] * (1 - e), dx).reshape(-1)
        if u_lim is not None:
            u = np.where(u < u_lim[0], u_lim[0], np.where(u > u_lim[1], u_lim[1], u))
        Us[t] = u
        J += float(p.cost(Xs[t], u))
        Xs[t + 1] = p.step(Xs[t], u)
        if W is not None:
            Xs[t + 1] += W[t]
        sep = min(sep, tc.separation(Xs[t + 1], k, ns, n_dims))
    J += float(p.cost(Xs[-1], np.zeros(k * nc), True))
    err = (Xs[-1] - xf).reshape(k, ns)
    return dict(X=Xs, U=Us, J=J, min_sep=sep, goal_dist=np.sqrt(np.sum(err[:, :case.n_d] ** 2, axis=1)))


def _starts(r, case):
    rng = np.random.default_rng(900 + case.k)
    scale = np.zeros((case.k, case.ns)); scale[:, :2] = 0.05
    return r["x0s"][:, None, :] + rng.normal(size=(sw.S, N_STARTS, case.k * case.ns)) * scale.reshape(-1)


def _check(got, r, case, x0s, W=None, u_lim=None):
    unchecked = 0
    p = sw.oracle_problem(case, r["xf"])
    for s in range(sw.S):
        tables = _definition_tables(r, case, s)
        for q in range(N_STARTS):
            Wq = None if W is None else W[s, q]
            ref = ref_definition(p, case, tables, r["xf"], x0s[s, q], Wq, u_lim)
            spread = max(pc.difference(ref_definition(p, case, tables, r["xf"], x0s[s, q], Wq, u_lim, e=sg * lc.PERTURB), ref) for sg in (1.0, -1.0))
            bound = pc.bound_of(spread)
            if bound is None:
                unchecked += 1
                continue
            g = dict(X=got["X"][s, q], U=got["U"][s, q], J=float(got["J"][s, q]), min_sep=float(got["min_sep"][s, q]),
                     goal_dist=got["goal_dist"][s, q])
            d = pc.difference(g, ref)
            print(f"{case.id} scenario {s} start {q}: difference {d:.3g}, bound {bound:.3g}")
            assert d <= bound, (s, q, d, bound)
    assert unchecked <= pc.MAX_UNCHECKED * sw.S * N_STARTS, unchecked


@pytest.mark.parametrize("case", sw.SOLVE_CASES, ids=lambda c: c.id)
def test_end_to_end_against_the_definition(case):
    r = swarm(case)
    k, ns, nc, Tn = case.k, case.ns, case.nc, case.T
    x0s = _starts(r, case)
    got = _host(r["pol"].rollout(x0s, trajectories=True))
    assert got["X"].shape == (sw.S, N_STARTS, Tn + 1, k * ns)
    _check(got, r, case, x0s)
    rng = np.random.default_rng(5)
    W = pc.W_SCALE * rng.normal(size=(sw.S, N_STARTS, Tn, k * ns))
    flat = got["U"].reshape(-1, k * nc)
    u_lim = np.stack([np.quantile(flat, pc.QUANTILES[0], axis=0), np.quantile(flat, pc.QUANTILES[1], axis=0)])
    got2 = _host(r["pol"].rollout(x0s, W=W, u_lim=u_lim, trajectories=True))
    assert np.mean((got2["U"] == u_lim[0]) | (got2["U"] == u_lim[1])) > 0.10
    _check(got2, r, case, x0s, W, u_lim)
    short = _host(r["pol"].rollout(x0s, W=W, u_lim=u_lim))
    assert set(short) == {"J", "min_sep", "goal_dist"} and all(np.array_equal(short[k_], got2[k_]) for k_ in short)


@pytest.mark.parametrize("case", sw.SOLVE_CASES, ids=lambda c: c.id)
def test_from_the_stitched_start_the_rollout_reproduces_the_plan(case):
    """Agent i's law is u_i = U^i_i + K^i_i (x_{C_i} - X^i).  Where every member of C_i has the neighbourhood C_i itself, the
    stitched X_dec over C_i IS X^i: from X_dec[0] and without disturbance the feedback term is exactly zero, U_ff_i = U_dec_i bit
    for bit, and the agent retraces its plan to the rollout tolerance (the plant's step is the solve's)."""
    r = swarm(case)
    k, ns, nc = case.k, case.ns, case.nc
    X_dec, U_dec, masks = r["X_dec"], r["U_dec"], r["masks"]
    got = _host(r["pol"].rollout(X_dec[:, :1, :].copy(), trajectories=True))
    U_ff = r["pol"].U_ff.cpu().numpy()
    n_closed = n_open = 0
    for s in range(sw.S):
        for i in range(k):
            closed = all(int(masks[s, j]) == int(masks[s, i]) for j in _members(masks[s, i], k))
            n_closed, n_open = n_closed + closed, n_open + (not closed)
            if closed:
                assert np.array_equal(U_ff[s][:, i * nc:(i + 1) * nc], U_dec[s][:, i * nc:(i + 1) * nc]), (s, i)
                assert np.array_equal(got["U"][s, 0][0, i * nc:(i + 1) * nc], U_dec[s][0, i * nc:(i + 1) * nc]), (s, i)      # dx = 0 exactly
                for a, b_ in ((got["U"][s, 0][:, i * nc:(i + 1) * nc], U_dec[s][:, i * nc:(i + 1) * nc]),
                              (got["X"][s, 0][:, i * ns:(i + 1) * ns], X_dec[s][:, i * ns:(i + 1) * ns])):
                    assert np.max(np.abs(a - b_)) <= pc.TOL_ROLLOUT * max(np.max(np.abs(b_)), 1.0), (s, i)
    print(f"{case.id}: {n_closed} agents retrace their plan, {n_open} have a neighbour with a plan of its own")
    assert n_closed >= k and (k <= 66 or n_open >= 1)


def test_closed_loop_distributed_wide_returns_scenario_zero():
    import dpilqr_amd as dp
    case = sw.SOLVE_CASES[0]
    r = swarm(case)
    x0s = _starts(r, case)
    got = _host(r["pol"].rollout(x0s, trajectories=True))
    one = dp.closed_loop_distributed(r["prob"], r["x0s"][0][None], r["U0"], sw.RADIUS, x0s[0], mu=pc.MU, trajectories=True, wide=True,
                                     n_lqr_iter=sw.N_LQR_ITER)
    assert np.array_equal(one["X_dec"], r["X_dec"][0]) and np.array_equal(one["U_dec"], r["U_dec"][0])
    for key in KEYS:
        assert np.array_equal(one[key], got[key][0]), key
    with pytest.raises(ValueError, match=r"policy=True is not built for teams of more than 64 agents \(this one has 65\)"):
        dp.closed_loop_distributed(r["prob"], r["x0s"][0][None], r["U0"], sw.RADIUS, x0s[0], mu=pc.MU)
