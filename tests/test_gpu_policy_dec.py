"""The neighbourhood-sparse closed-loop rollout (dpilqr_policy_rollout_dec, csrc/policy_dec.hpp) against the CPU reference, per
sample.  Cases, masks, reference and bound: tests/policy_dec_cases.py -- the reference is policy_cases.ref_sample fed the dense
gains with the off-mask blocks zeroed, the bound policy_cases.bound_of of its own +-PERTURB sensitivity; the kernel gets the
compact gains with every unused column filled with NaN.  Every case runs plain, with W, with u_lim, and with / without stored
trajectories.

kc_max: item 0 of every case has full masks, so the true maximum of the three-item batch is k and that run IS the kc_max = k
run; the items 1 and 2 alone (every agent alone; random masks, all smaller than k) run once with their true maximum and once with
kc_max = k: finite, equal to one another and to the same items of the three-item run.

With all masks full the results are held to ProblemBatch.policy_rollout on the same dense K: bit for bit -- the two kernels are
one rollout body (csrc/policy.hpp) with two descriptions of the gains, and with full masks both descriptions add the same
products in the same order -- and, as before, within the per-sample bound of tests/policy_cases.py."""
import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_dec_cases as dc

pytestmark = pytest.mark.gpu

B, T = pc.B, pc.T
VARIANTS = ["plain", "W", "u_lim"]


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
        ref = dc.case_ref(case)
        b, k, ns, nc = ref.batch, case.k, case.ns, case.nc
        pb = _pb(case, b)
        Kc = dc.compact_gains(ref.K, ref.masks, ns, nc, ref.true_kc_max(range(B)))
        assert Kc.shape[-1] == k * ns and (np.isnan(Kc).any() or k == 1)
        out = {}
        for v in VARIANTS:
            W, lim = ref.args(v)
            out[v] = _host(pb.policy_rollout_dec(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
            out[v + "-nostore"] = _host(pb.policy_rollout_dec(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim))
        if k > 1:
            items = [1, 2]
            pb2 = _pb(case, b, items)
            for kc_max in (ref.true_kc_max(items), k):
                Kc2 = dc.compact_gains(ref.K[items], ref.masks[items], ns, nc, kc_max)
                assert np.isnan(Kc2).any()
                for v in VARIANTS:
                    W, lim = ref.args(v)
                    out[(v, kc_max)] = _host(pb2.policy_rollout_dec(ref.X[items], ref.U[items], Kc2, ref.masks[items], b["x0s"][items],
                                                                    W=None if W is None else W[items], u_lim=lim, trajectories=True))
        _RUNS[case.id] = out
    return _RUNS[case.id]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_against_reference(case, variant):
    ref = dc.case_ref(case)
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


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_not_storing_trajectories_changes_nothing(case, variant):
    runs = gpu_runs(case)
    a, b_ = runs[variant], runs[variant + "-nostore"]
    assert set(b_) == {"J", "min_sep", "goal_dist"}
    for key in b_:
        assert np.array_equal(a[key], b_[key]), key


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", [c for c in dc.CASES if c.k > 1], ids=[c.id for c in dc.CASES if c.k > 1])
def test_unused_columns_never_enter_the_arithmetic(case, variant):
    """kc_max = the true maximum of the items 1 and 2 against kc_max = k, NaN in every unused column of both."""
    ref = dc.case_ref(case)
    runs = gpu_runs(case)
    true_max = ref.true_kc_max([1, 2])
    assert true_max < case.k
    tight, wide, full = runs[(variant, true_max)], runs[(variant, case.k)], runs[variant]
    for key in ("X", "U", "J", "goal_dist", "min_sep"):
        assert np.isfinite(tight[key]).all() and np.isfinite(wide[key]).all(), key
        assert np.array_equal(tight[key], wide[key]), key
        assert np.array_equal(tight[key], full[key][[1, 2]]), key


@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_full_masks_agree_with_the_dense_kernel(case):
    """Every case of tests/policy_cases.py (all five kernel instantiations): all masks full, Kc the dense K regrouped."""
    ref = pc.case_ref(case)
    b, k = ref.batch, case.k
    pb = _pb(case, b)
    masks = np.full((B, k), (1 << k) - 1, dtype=np.uint64)
    Kc = dc.compact_gains(ref.K, masks, case.ns, case.nc, k)
    assert np.array_equal(Kc.reshape(B, T, k * case.nc, k * case.ns), ref.K)
    for v in VARIANTS:
        W, lim = ref.args(v)
        dense = _host(pb.policy_rollout(ref.X, ref.U, ref.K, b["x0s"], W=W, u_lim=lim, trajectories=True))
        dec = _host(pb.policy_rollout_dec(ref.X, ref.U, Kc, masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
        assert set(dec) == set(dense) == {"X", "U", "J", "min_sep", "goal_dist"}
        for key in dense:
            assert np.array_equal(dense[key], dec[key]), (v, key)
        unchecked = 0
        for i in range(B):
            for s in range(case.S):
                bound = pc.bound_of(ref.spread[v][i, s])
                if bound is None:
                    unchecked += 1
                    continue
                g, r = ({key: (float(o[key][i, s]) if key in ("J", "min_sep") else o[key][i, s]) for key in o} for o in (dec, dense))
                assert pc.difference(g, r) <= bound, (v, i, s, pc.difference(g, r), bound)
        assert unchecked <= pc.MAX_UNCHECKED * B * case.S, (v, unchecked, B * case.S)
