"""The active list ordered by sweep cost (csrc/admit_order.hpp) on the device.

Keys: k_cost_keys counts, per listed item, the steps t in 0..T at which some pair of agents is near by the fused sweep's own
criterion !(dx*dx + dy*dy > r*r*(1 + 1e-12)); held to a NumPy count of the same expression (float64, no fused multiply-add on
either side) on trajectories built by hand, T = 6, k = 2, 3, 5 (and k = 1: no pairs, key 0).
Order: k_order_list gives a permutation of the list, heaviest class first, dealt by either order.
Loop: ordering is pure scheduling.  For cfg2's model (k = 5, T = 50) the default order, DPILQR_NO_COST_ORDER and each order
variant give bit-identical X, U, J, status, n_bwd, n_fwd and gains by item, and a solve enqueued in two calls (resume = 1) equals the
synchronous one.  Route switches are read once, so every variant runs in a fresh child process (tests/cost_order_child.py).  A lost
item would stay ACTIVE (status 0) and a duplicated one would be counted twice in n_bwd: equal counters are the permutation check."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
T, R = 6, 0.5


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()
    return dpilqr_amd


def numpy_keys(X, k, r):
    """[B][T+1][4k] -> near-step counts, the sweep's expression and criterion"""
    lim = r * r * (1.0 + 1e-12)
    near = np.zeros(X.shape[:2], dtype=bool)
    for i in range(k):
        for j in range(i + 1, k):
            ddx = X[:, :, 4 * i] - X[:, :, 4 * j]
            ddy = X[:, :, 4 * i + 1] - X[:, :, 4 * j + 1]
            s2 = ddx * ddx + ddy * ddy
            near |= ~(s2 > lim)
    return near.sum(1).astype(np.int32)


def hand_built(k):
    """cases x [T+1][4k]: never near; every step near; one pair at distance exactly r at one step; that pair at r (1 + 2e-12), just
    outside; only the terminal state near; and random clouds at the radius' scale.  Expected counts where they are known by hand."""
    rng = np.random.default_rng(100 + k)
    far = np.zeros((T + 1, 4 * k))
    far[:, 0::4] = 10.0 * np.arange(k)[None, :] + 0.01 * np.arange(T + 1)[:, None]      # agents 10 apart on the x axis, drifting together
    far[:, 1::4] = 3.0
    far[:, 2::4] = rng.normal(size=(T + 1, k)); far[:, 3::4] = rng.normal(size=(T + 1, k))   # velocities: not part of the criterion
    cases, want = [far.copy()], [0]
    close = far.copy(); close[:, 0::4] = 0.1 * np.arange(k)[None, :]
    cases.append(close); want.append(T + 1)
    last = k - 1      # the pair (0, k-1): the last of agent 0's pairs in combinations order
    exact = far.copy(); exact[3, 0] = 0.0; exact[3, 1] = 3.0; exact[3, 4 * last] = R; exact[3, 4 * last + 1] = 3.0
    if k > 2:
        exact[3, 4::4][: k - 2] = 50.0 + 10.0 * np.arange(k - 2)      # the others out of the way of both
    cases.append(exact); want.append(1)
    outside = exact.copy(); outside[3, 4 * last] = R * (1.0 + 2e-12)
    assert outside[3, 4 * last] > R
    cases.append(outside); want.append(0)
    term = far.copy(); term[T, 0::4] = 0.05 * np.arange(k)[None, :]
    cases.append(term); want.append(1)
    for _ in range(11):
        cloud = far.copy(); cloud[:, 0::4] = rng.normal(size=(T + 1, k)) * 0.6; cloud[:, 1::4] = rng.normal(size=(T + 1, k)) * 0.6
        cases.append(cloud); want.append(None)
    return np.stack(cases), want


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_device_keys_equal_a_numpy_count(dp, k):
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle, to_dev
    if k == 1:
        X = np.zeros((4, T + 1, 4)); want = [0] * 4
    else:
        X, want = hand_built(k)
    B = X.shape[0]
    ref = numpy_keys(X, k, R)
    for i, w in enumerate(want):
        assert w is None or ref[i] == w, (i, ref[i], w)      # the NumPy count itself, on the cases known by hand
    if k > 1:
        assert 0 < ref[5:].sum() < (B - 5) * (T + 1)         # the random clouds: some steps near, some not
    pb = dp.ProblemBatch([0] * k, [2] * k, np.zeros((B, 4 * k)), np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), R, 0.1, T)
    Xd = to_dev(X)
    keys = torch.full((B,), -7, dtype=torch.int32, device=Xd.device)
    _lib.check(_lib.load().dpilqr_cost_keys(pb._d, ptr(Xd), None, None, ptr(keys), stream_handle()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(keys.cpu().numpy(), ref)
    # through a list: keys by list position, entries beyond the count untouched
    items = torch.tensor([B - 1, 0, 2], dtype=torch.int32, device=Xd.device); cnt = torch.tensor([3], dtype=torch.int32, device=Xd.device)
    keys.fill_(-7)
    _lib.check(_lib.load().dpilqr_cost_keys(pb._d, ptr(Xd), ptr(items), ptr(cnt), ptr(keys), stream_handle()))
    torch.cuda.synchronize()
    got = keys.cpu().numpy()
    np.testing.assert_array_equal(got[:3], ref[[B - 1, 0, 2]])
    assert (got[3:] == -7).all()


@pytest.mark.parametrize("n,waves", [(3000, 12), (1500, 8), (1025, 8), (6145, 12), (5, 4)])
def test_order_list_is_a_permutation_heaviest_first(dp, n, waves):
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle
    L = _lib.load()
    rng = np.random.default_rng(n)
    T50, n_cus = 50, 256
    keys_h = rng.integers(0, T50 + 2, size=n).astype(np.int32)
    keys_h[rng.random(n) < 0.7] = 0                          # most items have no near step, as in cfg2
    items_h = (rng.permutation(n) + 1000).astype(np.int32)
    dev = torch.device("cuda")
    keys = torch.tensor(keys_h, device=dev); items = torch.tensor(items_h, device=dev); cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    key_of = dict(zip(items_h.tolist(), keys_h.tolist()))
    for order in (_lib.ORDER_SPREAD, _lib.ORDER_GROUPED):
        out = torch.full((n + 8,), -1, dtype=torch.int32, device=dev)
        _lib.check(L.dpilqr_order_list(ptr(items), ptr(cnt), ptr(keys), T50, n_cus, waves, order, ptr(out), stream_handle()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[n:] == -1).all()
        assert sorted(got[:n].tolist()) == sorted(items_h.tolist())
        by_rank = [key_of[int(got[L.dpilqr_order_position(r, n, n_cus, waves, order)])] for r in range(n)]
        assert all(a >= b for a, b in zip(by_rank, by_rank[1:])), order      # T + 1 < 64: a class is a count


VARIANTS = {"default": {}, "off": {"DPILQR_DEBUG_ROUTES": "1", "DPILQR_NO_COST_ORDER": "1"},
            "spread": {"DPILQR_DEBUG_ROUTES": "1", "DPILQR_COST_ORDER": "1"}, "grouped": {"DPILQR_DEBUG_ROUTES": "1", "DPILQR_COST_ORDER": "2"}}


@pytest.fixture(scope="module")
def variants(dp, tmp_path_factory):
    """every variant's child process, side by side (four processes with the GPU open)"""
    tmp = tmp_path_factory.mktemp("cost_order")
    procs = {}
    for name, env in VARIANTS.items():
        e = {k: v for k, v in os.environ.items() if not k.startswith("DPILQR_")}
        e.update(env)
        procs[name] = subprocess.Popen([sys.executable, str(ROOT / "tests" / "cost_order_child.py"), str(tmp / f"{name}.json")], env=e,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    for name, p in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (name, log[-3000:])
        out[name] = json.loads((tmp / f"{name}.json").read_text())
    return out


@pytest.mark.parametrize("shape", ["1100/1100/3", "3000/2100/3", "40/7/3"])
def test_ordering_is_pure_scheduling(variants, shape):
    """1100 / 1100: the 8-wavefront tier, then the list falls to the team tier, where ordering switches off.  3000 / 2100: the
    12-wavefront tier with admission in mid-solve (new items sorted among survivors).  40 / 7: a list far smaller than one layer."""
    ref = variants["off"][shape]
    st = np.array(ref["status"])
    assert (st != 0).all() and len(set(ref["n_bwd"])) > 1      # everything finished, after different numbers of iterations
    for name in ("default", "spread", "grouped"):
        got = variants[name][shape]
        for key in ("status", "n_bwd", "n_fwd"):
            differ = np.flatnonzero(np.array(got[key]) != np.array(ref[key]))
            assert differ.size == 0, (name, key, differ[:10])
        for key in ("X", "U", "J", "K", "d"):
            differ = np.flatnonzero(np.array(got[key]["per_item"]) != np.array(ref[key]["per_item"]))
            assert differ.size == 0 and got[key]["sha"] == ref[key]["sha"], (name, key, differ[:10])


@pytest.mark.parametrize("shape", ["1100/1100/3", "3000/2100/3", "40/7/3"])
def test_a_resumed_enqueue_equals_the_synchronous_solve(variants, shape):
    for name in VARIANTS:
        eq = variants[name][shape]["resumed_equal"]
        assert all(eq.values()), (name, eq)
