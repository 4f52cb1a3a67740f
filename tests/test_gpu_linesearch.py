"""The solve loop's line-search kernels, per candidate, against the oracle.

k_linesearch_wave<MODEL, KA> (74 instantiations), k_linesearch_team<MODEL, KA> (30) and k_forward in kModeLineSearch (the
LDS-staged form and the large-cluster forms) run inside the device-resident solve loop and nowhere else: the stand-alone
forward pass of the API always runs kModeCandidates.  A ONE-ITERATION solve isolates them: one rollout, one backward pass at
mu = 1 and one line search per item, returning the GPU's own gains, the decision trace row (mu_before, acc, J_last, J_new,
n_eval) and the accepted iterate.  The oracle is then fed the GPU's gains -- an error of the sweep can neither be blamed on the
line search nor hide one -- and evaluates the candidates one by one up to its own first accepted one.

Bound: measured per item on the oracle, not fixed.  The pass of the last evaluated candidate is rerun with X0, K, d perturbed by
1e-15 relative (both sign patterns); spread = the largest relative change of X, U, J; the item's bound is
max(1e-9, 100 x spread) -- 1e-9 is the project's per-pass tolerance, 100 its ratio to the 1e-11 rollout tolerance.  An item
whose spread exceeds 1e-7 draws no bound (unchecked).  An item with an oracle candidate within its bound of J0 (or of the
convergence threshold) is a near tie: its decision need not match and its values are compared at the GPU's own acc.  Unchecked
plus near-tie items are at most 5 % of a case's checked items.  profiles/linesearch_oracle_sensitivity.txt
(scripts/linesearch_oracle_sensitivity.py) holds the same measurement with the oracle's own gains, and the GPU's worst errors.

Which kernel ran: the library's profile hook reports the line search as one phase, not its variants, so the route is derived
from what launch_forward (tu_forward.hip) and launch_linesearch_team (tu_lsteam.hip) branch on -- the model hint of the
descriptor, k against the instantiation tables, the launch width (window = B) against 1024, n_x against 60, and for the large
clusters forward_on_pipe's inputs -- with every route switch of the environment required to be unset.

Returned J: on a failed search the solve returns the cost of the LAST EVALUATED candidate (the reference's quirk Q2, as
oracle_solve does), so J is held to the oracle's tenth candidate there, while X, U and the trace's J_new are held to the
unchanged X0, U0, J0."""
import os

import numpy as np
import pytest

from tests import linesearch_cases as lc
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

CASES = lc.all_cases()
ROUTE_SWITCHES = ("DPILQR_FORWARD_GENERIC", "DPILQR_LS_NO_TEAM", "DPILQR_LS_TEAM_MAX", "DPILQR_FORCE_BIG", "DPILQR_FORWARD_NO_PACK")


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()   # loud failure if the HIP library or the GPU is missing
    return dpilqr_amd


def _assert_route(pb, case):
    """launch_forward's branches (tu_forward.hip) in its own order, on the descriptor the library was given."""
    assert not [v for v in ROUTE_SWITCHES if v in os.environ]
    assert case.expected_route() == case.route
    hint = (pb.desc.uniform_model & 0xff) - 1
    n, m, k = pb.n_x, pb.n_u, pb.k
    threads = ((k * 10 + 63) // 64) * 64
    big = n > 60 or ((lc.forward_lds_bytes(n, m, k) + 15) & ~15) > lc.K_MAX_LDS or (m * n + threads - 1) // threads > lc.K_MAX_STAGE
    assert big == (case.route == "big") and pb.fused_sweep == (n > 60)
    if big:
        assert lc.forward_on_pipe(n, m, k)      # k_forward<..., KDIRECT, PIPE>: tests/test_linesearch_cases.py shows no served size is off it
    elif case.route == "generic":
        assert hint == -1      # no model hint: neither table is tried
    else:
        assert hint == case.models[0] and (hint, k) in lc.WAVE_TABLE
        assert (case.B <= lc.TEAM_MAX and (hint, k) in lc.TEAM_TABLE) == (case.route == "team")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_line_search_against_oracle(dp, case):
    from oracle import oracle as orc
    b = lc.make_batch(case)
    B, T = case.B, b["T"]
    radius = b["radius"] if case.per_agent else float(b["radius"][0])
    pb = dp.ProblemBatch(b["models"], b["n_dims"], b["xf"], b["Q"], b["R"], b["Qf"], radius, b["dt"], T)
    _assert_route(pb, case)
    r = pb.solve(b["x0"], b["U0"], n_lqr_iter=1, trace=True, gains=True, window=B)
    import torch
    idx = case.checked()
    sel = torch.as_tensor(idx, device=r["X"].device)
    h = {key: r[key][sel].cpu().numpy() for key in ("X", "U", "J", "status", "n_bwd", "n_fwd", "trace", "K", "d")}
    al = orc.alphas()
    unchecked = ties = later = failed = 0
    worst, worst_bound, min_margin = 0.0, 0.0, np.inf
    for j, i in enumerate(idx):
        tr = h["trace"][j, 0]
        ref = lc.ItemRef(lc.item_problem(b, i), b["x0"][i], b["U0"][i], h["K"][j], h["d"][j], al)
        later += ref.acc >= 1; failed += ref.acc < 0
        # bookkeeping that holds whatever the numbers are
        acc, n_eval = int(tr[1]), int(tr[4])
        assert tr[0] == 1.0 and tr[1] == acc and -1 <= acc <= 9, (i, tr)
        assert n_eval == (acc + 1 if acc >= 0 else 10) and h["n_fwd"][j] == n_eval and h["n_bwd"][j] == 1, (i, tr, h["n_fwd"][j])
        if ref.bound is None:
            unchecked += 1
            continue
        bound, tie = ref.bound, ref.near_tie(ref.bound)
        ties += tie
        if not tie:
            assert acc == ref.acc, (i, acc, ref.acc, ref.J0, ref.Js)
            assert all(not (Ji < ref.J0) for Ji in ref.Js[:max(ref.acc, 0)])      # the oracle rejects what the GPU rejected
            assert h["status"][j] == ref.status(acc), (i, h["status"][j], ref.margin(acc) if acc >= 0 else None)
        elif acc != ref.acc:      # near tie decided the other way: every decision the GPU took is one the bound allows
            bound = ref.bound_of(ref.spread_of(n_eval - 1))
            assert bound is not None, i
            for c in range(n_eval):
                rejected = not (ref.J(c) < ref.J0)
                assert rejected == (c != acc) or ref.margin(c) < bound, (i, c, acc, ref.J(c), ref.J0)
        last = n_eval - 1
        Xc, Uc, Jc = ref.candidate(last)
        errs = [abs(tr[2] - Jc) / abs(Jc), abs(h["J"][j] - Jc) / abs(Jc)]      # J_last; the returned J (quirk Q2)
        if acc >= 0:
            assert tr[3] == tr[2], (i, tr)
            errs += [relerr(h["X"][j], Xc), relerr(h["U"][j], Uc)]
        else:      # a failed search leaves the iterate alone
            assert np.array_equal(h["U"][j], b["U0"][i]), i
            errs += [relerr(h["X"][j], ref.X0), abs(tr[3] - ref.J0) / abs(ref.J0)]
            assert h["status"][j] == ref.status(-1)
        err = max(errs)
        print(f"  item {i}: acc {acc} (oracle {ref.acc}) err {err:.2e} bound {bound:.2e} spread {ref.spread:.1e}{' tie' if tie else ''}")
        assert err < bound, (i, acc, errs, bound)
        margin = bound / err if err > 0 else np.inf
        if margin < min_margin or worst_bound == 0.0:
            min_margin, worst, worst_bound = margin, err, bound
    n = len(idx)
    print(f"LS_RESULT {case.id} items={n} ties={ties} unchecked={unchecked} worst_err={worst:.3e} its_bound={worst_bound:.3e} "
          f"min_margin={min_margin:.3g} later={later} failed={failed}")
    assert unchecked + ties <= 0.05 * n, (unchecked, ties, n)
    if case.later_candidates_expected():
        assert later >= 0.10 * n, (later, n)


@pytest.mark.parametrize("route,models,B", [("wave", [0] * 3, 1100), ("team", [0] * 3, 700), ("wave", [3] * 8, 260), ("team", [3] * 2, 37),
                                            ("generic", [0, 3, 0], 260), ("big", [3] * 16, 3)])
def test_exact_tie_is_rejected(dp, route, models, B):
    """Agents at rest at their goals, far apart, U0 = 0: the cost gradient is exactly zero, so d = 0, every candidate reproduces
    X0, U0 bit for bit and J_i == J0 exactly.  The reference accepts on J_i < J0 only (control.py:183): all ten are evaluated
    and the search fails -- with `<=` in linesearch_decide the first candidate would be accepted."""
    from oracle import oracle as orc
    case = lc.Case(route, models, B, 1, seed=900 + len(models))
    assert case.expected_route() == route
    k, T = case.k, 8
    xf = np.zeros((B, k, 4)); xf[:, :, 0] = 3.0 * np.arange(k); xf[:, :, 1] = np.arange(B)[:, None] * 0.25
    xf = xf.reshape(B, -1); x0 = xf.copy(); U0 = np.zeros((B, T, 2 * k))
    Q, R, Qf = np.eye(4) * 1.3, np.eye(2), 100.0 * np.eye(4)
    pb = dp.ProblemBatch(models, [2] * k, xf, Q, R, Qf, 0.6, 0.1, T)
    r = {key: v.cpu().numpy() for key, v in pb.solve(x0, U0, n_lqr_iter=1, trace=True, gains=True, window=B).items()}
    p = orc.Problem(models, [2] * k, xf[B - 1], Q, R, Qf, 0.6, 0.1, T)
    ref = lc.ItemRef(p, x0[B - 1], U0[B - 1], r["K"][B - 1], r["d"][B - 1], orc.alphas())
    assert ref.acc == -1 and all(Ji == ref.J0 for Ji in ref.Js)      # the oracle: ten exact ties, none accepted
    assert not r["d"].any()
    assert (r["trace"][:, 0, 1] == -1).all() and (r["trace"][:, 0, 4] == 10).all() and (r["n_fwd"] == 10).all()
    assert (r["status"] == 2).all() and (r["J"] == ref.J0).all() and (r["trace"][:, 0, 2] == ref.J0).all()
    assert np.array_equal(r["X"], np.broadcast_to(x0[:, None, :], r["X"].shape)) and not r["U"].any()
