"""The zero-pivot path, end to end: every sweep's singular[] flag, the line searches' retirement with DPILQR_STATUS_SINGULAR, and
ilqrSolver.solve's LinAlgError -- on inputs whose Q_uu has an exactly zero pivot (tests/singular_cases.py: B = 0 tiles, an idle
control with zero weight, dt = 0), mixed with healthy items in one launch.

What is held, everywhere: the flags equal the oracle's verdict item by item, un-flagged entries are still 0; the gains (the
results) of the healthy items are the oracle's to the neighbouring tests' tolerance AND bit for bit what a launch (a solve) of
the healthy items alone gives -- a flagged item's NaNs do not reach the neighbour that shares its workgroup's LDS, and a retired
item does not upset the window's bookkeeping.  Nothing is asserted about a flagged item's gains.

The `tiny` control of the tile cases (a 2^-60 pivot: not zero, not flagged) is held to the tolerance like `healthy`: the oracle's
own gains for it agree with a longdouble replay to rounding (tests/test_singular_cases.py)."""
import numpy as np
import pytest

from tests import loop_gains_cases as lg
from tests import singular_cases as sc
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

TILE_CASES = sc.tile_cases()
SWEEP_CASES = sc.sweep_cases()
SOLVE_CASES = sc.solve_cases()
TOL_PASS = lg.TOL_PASS


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()   # loud failure if the HIP library or the GPU is missing
    return dpilqr_amd


def _bits(t):
    """Host copy for a bit-for-bit comparison, NaNs included."""
    a = t.cpu().numpy()
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool((a == b).all())


# ------------------------------------------------------------------ the tiles API
def _launch_tiles(dp, case, arrays):
    import torch
    Bn = arrays[1].shape[0]
    sing = torch.zeros(Bn, dtype=torch.int32, device="cuda")
    K, d = dp.backward_pass_tiles(dp.pack_tiles(*arrays), Bn, case.T, case.n, case.m, sc.TILE_MU, singular=sing, blocks=case.blocks)
    return sing.cpu().numpy(), K, d


@pytest.mark.parametrize("case", TILE_CASES, ids=[c.id for c in TILE_CASES])
def test_tiles_flags_and_healthy_neighbours(dp, case):
    arrays = sc.make_tiles(case)
    verdicts = sc.tile_verdicts(arrays)
    want = np.array([int(v[0]) for v in verdicts], dtype=np.int32)
    assert 0 < want.sum() < case.count
    sing, K, d = _launch_tiles(dp, case, arrays)
    assert np.array_equal(sing, want), np.flatnonzero(sing != want)[:10]
    keep = np.flatnonzero(want == 0)
    Kh, dh = K.cpu().numpy(), d.cpu().numpy()
    worst = 0.0
    for i in keep:
        eK, ed = relerr(Kh[i], verdicts[i][1]), relerr(dh[i], verdicts[i][2])
        worst = max(worst, eK, ed)
        assert eK < case.tol and ed < case.tol, (i, case.items()[i], eK, ed)
    print(f"SINGULAR_TILES {case.id} flagged={int(want.sum())} healthy={keep.size} worst={worst:.3e} tol={case.tol:g}")
    sing2, K2, d2 = _launch_tiles(dp, case, sc.tiles_subset(arrays, keep))
    assert not sing2.any()
    sel = np.asarray(keep)
    assert _same_bits(K[sel], K2) and _same_bits(d[sel], d2)


@pytest.mark.parametrize("case", [c for c in TILE_CASES if c.count < 100], ids=lambda c: c.id)
def test_tiles_listed_launch_flags_by_item_id(dp, case):
    """With an item list (include/dpilqr_hip.h) mu and singular[] are indexed by item id, the records, K and d by position in the
    list; what is not listed or beyond the live count is not touched."""
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle, to_dev
    arrays = sc.make_tiles(case)
    verdicts = sc.tile_verdicts(arrays)
    Bn, T, n, m = case.count, case.T, case.n, case.m
    rng = np.random.default_rng(case.n)
    order = rng.permutation(Bn)
    items = order[:2 * Bn // 3]
    live = items[:len(items) - 2]
    tiles = dp.pack_tiles(*sc.tiles_subset(arrays, order))      # a record for every slot of the launch, listed or not
    mu = to_dev(np.full(Bn, sc.TILE_MU))
    K = torch.full((Bn, T, m, n), -7.0, dtype=torch.float64, device="cuda"); d = torch.full((Bn, T, m), -7.0, dtype=torch.float64, device="cuda")
    sing = torch.zeros(Bn, dtype=torch.int32, device="cuda")
    items_t = torch.as_tensor(items, dtype=torch.int32, device="cuda"); n_items = torch.tensor([len(live)], dtype=torch.int32, device="cuda")
    bns, bnc = case.blocks or (0, 0)
    _lib.check(_lib.load().dpilqr_backward_pass_tiles_blocks(Bn, T, n, m, bns, bnc, ptr(tiles), ptr(mu), ptr(K), ptr(d), ptr(sing), ptr(items_t),
                                                            ptr(n_items), stream_handle()))
    torch.cuda.synchronize()
    want = np.zeros(Bn, dtype=np.int32)
    for i in live:
        want[i] = int(verdicts[i][0])
    assert want.any() and np.array_equal(sing.cpu().numpy(), want)
    Kh, dh = K.cpu().numpy(), d.cpu().numpy()
    for slot, i in enumerate(live):
        if not verdicts[i][0]:
            assert relerr(Kh[slot], verdicts[i][1]) < case.tol and relerr(dh[slot], verdicts[i][2]) < case.tol, (slot, i)
    assert (Kh[len(live):] == -7.0).all() and (dh[len(live):] == -7.0).all()


# ------------------------------------------------------------------ the descriptor sweeps
def _problem_batch(dp, b):
    return dp.ProblemBatch(b["models"], b["n_dims"], b["xf"], b["Q"], b["R"], b["Qf"], b["radius"], b["dt"], b["T"])


def _assert_descriptor(pb, case):
    """The inputs of the route mirrors (loop_gains_cases.loop_route, singular_cases.sweep_route) on the descriptor itself."""
    import os
    assert not [v for v in lg.ROUTE_SWITCHES if v in os.environ]
    um, und, shared, planar4 = case.hints()
    w = pb.desc.uniform_model
    assert ((w & 0xff) - 1, ((w >> 8) & 0xff) - 1, bool((w >> 16) & 1), bool((w >> 17) & 1)) == (um, und, shared, planar4)
    assert (pb.desc.R_bstride != 0) == (case.how == "per_item_R") and (pb.desc.model_bstride != 0) == (case.how == "models")


def _fused_sweep(dp, b):
    """dpilqr_backward_pass_fused at (rollout(x0, U0), U0, mu = 1): flags, K, d and the device's X."""
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import empty, ptr, stream_handle, to_dev
    pb = _problem_batch(dp, b)
    Bn, T, n, m = pb.B, pb.T, pb.n_x, pb.n_u
    U = to_dev(b["U0"])
    X = pb.rollout(b["x0"], U)[0]
    mu = to_dev(np.ones(Bn))
    K = empty((Bn, T, m, n)); d = empty((Bn, T, m)); sing = torch.zeros(Bn, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().dpilqr_backward_pass_fused(pb._d, ptr(X), ptr(U), ptr(mu), ptr(K), ptr(d), ptr(sing), stream_handle()))
    torch.cuda.synchronize()
    return pb, sing.cpu().numpy(), K, d, X.cpu().numpy()


def _hold_gains(b, idx, K, d, X, tag):
    Kh, dh = K.cpu().numpy(), d.cpu().numpy()
    worst = 0.0
    for i in idx:
        Ko, do = sc.item_problem(b, i).backward_pass(X[i], b["U0"][i], 1.0)
        eK, ed = relerr(Kh[i], Ko), relerr(dh[i], do)
        worst = max(worst, eK, ed)
        assert eK < TOL_PASS and ed < TOL_PASS, (tag, i, eK, ed)
    return worst


@pytest.mark.parametrize("case,route", SWEEP_CASES, ids=[c.id for c, _ in SWEEP_CASES])
def test_descriptor_sweep_flags_and_healthy_neighbours(dp, case, route):
    assert sc.sweep_route(case) == route
    b = sc.make_solve_batch(case)
    want = np.array([int(sc.item_verdict(b, i)[0]) for i in range(case.B)], dtype=np.int32)
    assert np.array_equal(want, b["singular"].astype(np.int32)) and want.any()
    pb, sing, K, d, X = _fused_sweep(dp, b)
    _assert_descriptor(pb, case)
    assert np.array_equal(sing, want), np.flatnonzero(sing != want)[:10]
    if case.how == "shared_R":      # one R for the batch: every item is singular; the healthy launch is the batch of the same shape under R = I
        h = sc.make_solve_batch(case, healthy_twin=True)
        keep = np.arange(case.B)
    else:
        keep = np.flatnonzero(want == 0)
        h = sc.batch_subset(b, keep)
    pbh, sing2, K2, d2, X2 = _fused_sweep(dp, h)
    assert not sing2.any()
    worst = _hold_gains(h, range(len(keep)), K2, d2, X2, case.id)
    print(f"SINGULAR_SWEEP {case.id} route={route} flagged={int(want.sum())} healthy={len(keep)} worst={worst:.3e}")
    if case.how != "shared_R":
        assert _same_bits(K[np.asarray(keep)], K2) and _same_bits(d[np.asarray(keep)], d2)


# ------------------------------------------------------------------ the solve loop
KEYS = ("X", "U", "J", "status", "n_bwd", "n_fwd", "trace")


def _dtype(case):
    import torch
    return torch.float32 if case.f32 else torch.float64


def _solve(dp, case, b, window=None):
    pb = _problem_batch(dp, b)
    seen = []
    r = pb.solve(b["x0"], b["U0"], n_lqr_iter=case.n_lqr_iter, trace=True, window=min(case.window, pb.B) if window is None else window,
                 dtype=_dtype(case), progress=lambda done, total: seen.append((done, total)))
    assert seen and seen[-1] == (pb.B, pb.B)
    return pb, r


def _hold_retired(pb, case, b, r, idx):
    """Every singular item: status 4, one backward pass counted and no forward pass (solve_state.hpp: retire_without_gains), the
    iterate it was given."""
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import to_dev
    assert _lib.STATUS_SINGULAR == sc.STATUS_SINGULAR
    U0 = to_dev(b["U0"], _dtype(case))
    Xr, Jr = pb.rollout(b["x0"], U0, dtype=_dtype(case))
    sel = torch.as_tensor(idx, device="cuda")
    assert (r["status"][sel] == sc.STATUS_SINGULAR).all().item(), r["status"][sel].cpu().numpy()
    assert (r["n_bwd"][sel] == 1).all().item() and (r["n_fwd"][sel] == 0).all().item()
    assert _same_bits(r["X"][sel], Xr[sel]) and _same_bits(r["U"][sel], U0[sel])
    Jg, Jw = r["J"][sel].cpu().numpy(), Jr[sel].cpu().numpy()
    assert np.isfinite(Jw).all() and (np.abs(Jg - Jw) <= 1e-14 * np.abs(Jw)).all()
    return Xr


def _hold_healthy(r, keep, rh, keys=KEYS):
    """The healthy items: bit for bit the solve of the healthy items alone, and none of them retired as singular."""
    import torch
    sel = torch.as_tensor(keep, device="cuda")
    st = rh["status"].cpu().numpy()
    assert np.isin(st, (1, 2, 3)).all(), st
    for key in keys:
        a, w = _bits(r[key][sel]), _bits(rh[key])
        differ = np.flatnonzero((a != w).reshape(len(keep), -1).any(axis=1))
        assert differ.size == 0, (key, [int(keep[j]) for j in differ[:10]])


@pytest.mark.parametrize("case", SOLVE_CASES, ids=[c.id for c in SOLVE_CASES])
def test_solve_retires_singular_items_and_leaves_the_healthy_alone(dp, case):
    from dpilqr_amd.batch import release_workspaces
    assert lg.loop_route(case)[1] == sc.SOLVE_ROUTES[case.id]
    b = sc.make_solve_batch(case)
    pb, r = _solve(dp, case, b)
    _assert_descriptor(pb, case)
    assert pb.fused_sweep == (lg.loop_route(case) == ("big", "big"))
    singular = np.flatnonzero(b["singular"]); keep = np.flatnonzero(~b["singular"])
    _hold_retired(pb, case, b, r, singular)
    if case.how == "shared_R":
        # the fused flagship sweep wants one R: every item above was singular.  Now the healthy batch of the same shape through the
        # pooled workspace the retired batch left behind -- and once more through a fresh one
        h = sc.make_solve_batch(case, healthy_twin=True)
        _, r1 = _solve(dp, case, h)
        release_workspaces()
        _, r2 = _solve(dp, case, h)
        _hold_healthy(r1, np.arange(case.B), r2)
        assert (r1["n_bwd"] >= 1).all().item() and (r1["n_fwd"] >= 1).all().item()
        return
    assert singular.size and keep.size
    _, rh = _solve(dp, case, sc.batch_subset(b, keep))
    _hold_healthy(r, keep, rh)


def test_solve_window_edge(dp):
    """B = 40 through a window of 8: singular items at index 0, on both sides of the window's edge, in the middle and at the last
    index.  Retired items free their slots for the items behind them like any finished item; list positions and item ids part
    from the second admission on."""
    case = sc.window_edge_case()
    b = sc.make_solve_batch(case)
    assert list(np.flatnonzero(b["singular"])) == [0, 7, 8, 22, 39]
    pb, r = _solve(dp, case, b, window=case.window)
    _hold_retired(pb, case, b, r, np.flatnonzero(b["singular"]))
    keep = np.flatnonzero(~b["singular"])
    for window in (case.window, len(keep)):
        _, rh = _solve(dp, case, sc.batch_subset(b, keep), window=window)
        _hold_healthy(r, keep, rh)


def test_solve_enqueue_retires_singular_items(dp):
    import torch
    case = sc.enqueue_case()
    b = sc.make_solve_batch(case)

    def run(bb):
        pb = _problem_batch(dp, bb)
        r, state = pb.solve_enqueue(bb["x0"], bb["U0"], pb.iterations_bound(case.n_lqr_iter, pb.B), n_lqr_iter=case.n_lqr_iter, window=pb.B)
        torch.cuda.synchronize()
        assert (r["status"] != 0).all().item()
        return pb, r
    pb, r = run(b)
    _hold_retired(pb, case, b, r, np.flatnonzero(b["singular"]))
    keep = np.flatnonzero(~b["singular"])
    _, rh = run(sc.batch_subset(b, keep))
    _hold_healthy(r, keep, rh, keys=KEYS[:-1])


def test_ilqr_solver_raises_linalgerror(dp):
    """ilqrSolver.solve turns DPILQR_STATUS_SINGULAR into what the reference's np.linalg.solve raises: one Human6D agent, whose
    third control is idle, with a zero weight on it."""
    from oracle import oracle as orc
    rng = np.random.default_rng(5)
    T, xf, x0, U0 = 6, rng.normal(size=6), rng.normal(size=6), 0.1 * rng.normal(size=(6, 3))
    Q, Qf = np.eye(6), 100.0 * np.eye(6)
    for R, singular in ((np.diag([1.0, 1.0, 0.0]), True), (np.eye(3), False)):
        dyn = dp.MultiDynamicalModel([dp.HumanDynamics6D(0.1, 0)])
        cost = dp.GameCost([dp.ReferenceCost(xf, Q, R, Qf, 0)], dp.ProximityCost([6], 0.5, [3]))
        s = dp.ilqrSolver(dp.ilqrProblem(dyn, cost), T)
        assert s.on_device
        o = orc.Problem([5], [3], xf, Q, R, Qf, 0.5, 0.1, T).solve(x0, U0, n_lqr_iter=6)
        assert (o["status"] == -1) == singular
        if singular:
            with pytest.raises(np.linalg.LinAlgError):
                s.solve(x0, U0, n_lqr_iter=6, verbose=False)
            assert s.status == sc.STATUS_SINGULAR and s.n_bwd == 1 and s.n_fwd == 0
        else:
            X, U, J = s.solve(x0, U0, n_lqr_iter=6, verbose=False)
            assert s.status in (1, 2, 3) and np.isfinite(J)
