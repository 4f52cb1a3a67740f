"""The solve loop's own backward pass -- its tile producers and every sweep as the loop launches it -- against the oracle, per item.

Inside the device-resident solve loop the backward pass takes routes no stand-alone entry point reaches: the sparse tile producer
(k_make_tiles<NS, NC, true>, on records whose zeros one memset put in place and whose slots later items of the window reuse), the
static part plus k_make_tiles_wave, and every sweep with an item list, gains_by_item, a per-item mu and a launch width equal to
the window.  Both ends of a solve are observable through the public API (tests/loop_gains_cases.py):

  first  solve(n_lqr_iter=1): every item's gains of the pass at (rollout(x0, U0), U0, mu = 1), at launch widths that select the
         team form and the 4-, 8- and 12-wavefront tiers;
  last   solve(n_lqr_iter=30, tol=0): an item that ends by a failed line search keeps its iterate, so the returned (X, U) are
         the point of its last backward pass, trace[n_bwd - 1, 0] its mu -- any of the schedule's seven values, exactly 0 on most --
         and (K, d) that pass's gains.  The window is a quarter of the batch (and 7, and 1100), so items are admitted and retired
         at staggered times and tile slots are reused.

Reference: the oracle's backward pass at the DEVICE's own linearisation point (X, U) and mu.  Bound, per item, K and d separately:
max(1e-9, 100 x spread), spread = the largest relative change of the oracle's own K (d) under X (1 +- 1e-15), U (1 -+ 1e-15); an
item whose spread exceeds 1e-7 draws no bound.  No other tolerance is fixed here.

Which kernels ran: derived from the descriptor by tests/loop_gains_cases.py's mirror of the loop's route selection, with every
route switch of the environment required unset, and held to the library's profile hook -- the tile producer's launches, and for
the wavefront sweeps the tier (wavefronts per workgroup) of the launches."""
import os

import numpy as np
import pytest

from tests import loop_gains_cases as lg
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

CASES = lg.all_cases()
FIRST = [c for c in CASES if c.mode == "first"]
LAST = [c for c in CASES if c.mode == "last"]


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()   # loud failure if the HIP library or the GPU is missing
    return dpilqr_amd


def _batch(dp, case):
    b = lg.make_batch(case)
    radius = b["radius"] if case.per_agent else float(b["radius"][0])
    return b, dp.ProblemBatch(b["models"], b["n_dims"], b["xf"], b["Q"], b["R"], b["Qf"], radius, b["dt"], b["T"])


def _assert_descriptor(pb, case):
    """The inputs of the loop's route selection, on the descriptor the library was given."""
    assert not [v for v in lg.ROUTE_SWITCHES if v in os.environ]
    um, und, shared, planar4 = case.hints()
    w = pb.desc.uniform_model
    assert ((w & 0xff) - 1, ((w >> 8) & 0xff) - 1, bool((w >> 16) & 1), bool((w >> 17) & 1)) == (um, und, shared, planar4)
    assert pb.desc.Q_bstride == pb.desc.R_bstride == pb.desc.Qf_bstride == 0
    assert (pb.n_x > lg.BIG_ABOVE) == (lg.loop_route(case) == ("big", "big")) == pb.fused_sweep


def _solve_profiled(pb, case, b, n_lqr_iter, tol):
    """The solve, with the profile hook's account of the producer's and the sweep's launches held to the case's route."""
    from dpilqr_amd import _lib
    _lib.profile_enable(True, classes=["tiles", "riccati"]); _lib.profile_read(reset=True)
    for w in (4, 8, 12):
        _lib.profile_read_sweep(w, reset=True)
    try:
        r = pb.solve(b["x0"], b["U0"], n_lqr_iter=n_lqr_iter, tol=tol, trace=True, gains=True, window=case.window)
        tot = _lib.profile_read(reset=True)
        var = {w: _lib.profile_read_sweep(w, reset=True)["launches"] for w in (4, 8, 12)}
    finally:
        _lib.profile_enable(False)
    producer, sweep = lg.loop_route(case)
    assert tot["riccati"]["launches"] >= 1 and tot["riccati"]["items"] == int(r["n_bwd"].sum().item())
    assert tot["tiles"]["launches"] == (0 if producer in ("none", "big") else tot["riccati"]["launches"]), (producer, tot)
    if sweep in lg.WAVE_SWEEPS:
        assert var[lg.sweep_tier(case)] >= 1 and sum(var.values()) == tot["riccati"]["launches"], (sweep, var, tot["riccati"])
    else:
        assert not any(var.values()), (sweep, var)
    return r


def _host(r, idx):
    import torch
    sel = torch.as_tensor(idx, device=r["X"].device)
    return {key: r[key][sel].cpu().numpy() for key in ("X", "U", "status", "n_bwd", "trace", "K", "d")}


class _Record:
    """The worst errors of a case against their bounds, and its LG_RESULT line."""

    def __init__(self):
        self.worst = {"K": (0.0, 0.0, np.inf), "d": (0.0, 0.0, np.inf)}      # (error, its bound, bound / error) of the smallest margin
        self.unchecked = {"K": 0, "d": 0}
        self.failures = []

    def hold(self, i, what, got, ref, bound, mu):
        if bound is None:
            self.unchecked[what] += 1
            return
        err = relerr(got, ref)
        margin = bound / err if err > 0 else np.inf
        if margin < self.worst[what][2] or self.worst[what][1] == 0.0:
            self.worst[what] = (err, bound, margin)
        if not err < bound:
            self.failures.append((i, what, err, bound, mu))

    def line(self, case, n, hist):
        (eK, bK, mK), (ed, bd, md) = self.worst["K"], self.worst["d"]
        return (f"LG_RESULT {case.id} route={'/'.join(lg.loop_route(case))} items={n} unchecked_K={self.unchecked['K']} "
                f"unchecked_d={self.unchecked['d']} worst_K={eK:.3e} its_bound={bK:.3e} worst_d={ed:.3e} its_bound={bd:.3e} "
                f"min_margin={min(mK, md):.3g} mu={ {f'{mu:g}': c for mu, c in hist.items()} }")


@pytest.mark.parametrize("case", FIRST, ids=[c.id for c in FIRST])
def test_first_pass_gains_against_oracle(dp, case):
    b, pb = _batch(dp, case)
    _assert_descriptor(pb, case)
    X0 = pb.rollout(b["x0"], b["U0"])[0]
    r = _solve_profiled(pb, case, b, 1, 1e-3)
    idx = case.checked()
    h = _host(r, idx)
    X0 = X0.cpu().numpy()
    rec = _Record()
    for j, i in enumerate(idx):
        assert h["n_bwd"][j] == 1 and h["trace"][j, 0, 0] == 1.0, (i, h["trace"][j, 0])
        ref = lg.GainsRef(lg.item_problem(b, i), X0[i], b["U0"][i], 1.0)
        rec.hold(i, "K", h["K"][j], ref.K, ref.bound_K, 1.0)
        rec.hold(i, "d", h["d"][j], ref.d, ref.bound_d, 1.0)
        if h["status"][j] == 2:      # a failed search leaves the iterate alone
            assert np.array_equal(h["X"][j], X0[i]) and np.array_equal(h["U"][j], b["U0"][i]), i
    print(rec.line(case, len(idx), {1.0: len(idx)}))
    assert not rec.failures, rec.failures
    assert max(rec.unchecked.values()) <= 0.10 * len(idx), rec.unchecked      # mu = 1, far from converged: the oracle alone leaves at most one item of a case without a bound


@pytest.mark.parametrize("case", LAST, ids=[c.id for c in LAST])
def test_last_pass_gains_against_oracle(dp, case):
    b, pb = _batch(dp, case)
    _assert_descriptor(pb, case)
    r = _solve_profiled(pb, case, b, lg.N_LQR_ITER_LAST, 0.0)
    idx = case.checked()
    h = _host(r, idx)
    rec, st = _Record(), lg.LastStats()
    for j, i in enumerate(idx):
        n_bwd = int(h["n_bwd"][j])
        assert 1 <= n_bwd <= lg.N_LQR_ITER_LAST and h["status"][j] in (2, 3), (i, n_bwd, h["status"][j])      # tol = 0: never converged
        if h["status"][j] != 2:
            st.add(int(h["status"][j]))
            continue
        tr = h["trace"][j, n_bwd - 1]
        mu = float(tr[0])
        assert tr[1] == -1 and tr[4] == 10 and mu in lg.MU_SCHEDULE, (i, tr)
        ref = lg.GainsRef(lg.item_problem(b, i), h["X"][j], h["U"][j], mu)
        st.add(2, mu, ref)
        rec.hold(i, "K", h["K"][j], ref.K, ref.bound_K, mu)
        rec.hold(i, "d", h["d"][j], ref.d, ref.bound_d, mu)
    print(rec.line(case, len(idx), st.histogram()) + f" failed_search={st.failed}")
    assert not rec.failures, rec.failures
    st.check()


@pytest.mark.parametrize("models", [[0] * 6, [3] * 6, [7] * 2, [2] * 8, [lg.BIKE] * 2], ids=lambda m: f"m{m[0]}k{len(m)}")
def test_window_invariance_on_record_fed_routes(dp, models):
    """An item's result does not depend on which tile slot it was given, which items held the slot before it, or how wide the
    launches were: windows of B, 37 and 1 give bit-identical results, the gains included."""
    case = lg.Case(models, 150, 150, "last", 1, seed=300 + len(models))
    assert lg.loop_route(case)[0] in ("sparse", "static+wave")
    b, pb = _batch(dp, case)
    _assert_descriptor(pb, case)
    keys = ("X", "U", "J", "status", "n_bwd", "n_fwd", "K", "d")
    ref = None
    for window in (150, 37, 1):
        r = pb.solve(b["x0"], b["U0"], n_lqr_iter=lg.N_LQR_ITER_LAST, tol=0.0, gains=True, window=window)
        got = {key: r[key].cpu().numpy() for key in keys}
        got = {key: a.view(np.int64) if a.dtype == np.float64 else a for key, a in got.items()}      # bit for bit, NaNs included
        if ref is None:
            ref = got
            assert int((ref["status"] == 2).sum()) >= 0.6 * case.B and ref["n_bwd"].min() < ref["n_bwd"].max()
            continue
        for key in keys:
            differ = np.flatnonzero((got[key] != ref[key]).reshape(case.B, -1).any(axis=1))
            assert differ.size == 0, (window, key, differ[:10])
