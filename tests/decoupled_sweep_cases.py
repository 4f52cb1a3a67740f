"""Hand-built trajectories for tests/test_gpu_decoupled_sweep.py, and that test's child process.

The fused DoubleInt4D sweep runs per-agent Riccati steps from t = T down to the first step at which some pair of agents is near
(csrc/riccati_mfma.hpp, "Decoupled prologue").  backward_pass_fused and backward_pass take X directly, so the trajectories are
built, not rolled out: agents far apart on the x axis, with the first pair (or the pair (0, k-1)) moved together at chosen steps.

As a script:  python tests/decoupled_sweep_cases.py OUT.npz  -- the same fused passes and the same windowed solve in a process of
its own, so that the parent can run it behind DPILQR_DEBUG_ROUTES=1 DPILQR_NO_DECOUPLED=1 (route switches are read once)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

T = 12
SIZES = (1100, 2100)          # the 8- and the 12-wavefront tier (launches of at most 1024 items go to the team kernel)
MUS = (0.0, 0.125, 1.0, 64.0)
Q = np.array([[1.0, 0.2, 0, 0], [0.1, 1.5, 0, 0.3], [0, 0, 0.4, 0], [0, 0.2, 0, 0.1]])     # non-symmetric: exercises Q + Q^T
R = np.array([[1.0, 0.1], [0.3, 2.0]])
QF = 50.0 * np.eye(4) + 0.5                                                               # dense in the block
# case name -> the steps at which the pair is near (inside the radius); "exact" / "outside": see trajectory()
CASES = {"never": [], "always": list(range(T + 1)), "terminal": [T], "one@0": [0], "one@1": [1], "one@6": [6], f"one@{T - 2}": [T - 2],
         f"one@{T - 1}": [T - 1], "interval+later": [3, 4, 5, 9], "exact@7": [], "outside@7": []}
NAMES = list(CASES)
DUPLICATES = ((3, 777), (40, 1099), (41, 2099), (500, 1500))      # (source, copy): the same item at two list positions
LISTED = [2099, 0, 2, 41, 1500]                                   # a list for the key kernel
NONFINITE = {17: np.inf, 18: np.nan}                               # item -> what one entry of its X becomes


def trajectory(name, k, r, rng):
    """[T+1][4k].  Far: agents 10 apart, drifting; velocities random (not part of the criterion).  Near at step t: agent 1 at 0.4 r from
    agent 0.  exact@7: the pair (0, k-1) at distance exactly r at step 7, the others out of the way; outside@7: that pair at
    r (1 + 2e-12), just beyond the sweep's margin of 1e-12 on r^2."""
    X = np.zeros((T + 1, 4 * k))
    X[:, 0::4] = 10.0 * np.arange(k)[None, :] + 0.01 * np.arange(T + 1)[:, None]
    X[:, 1::4] = 3.0
    X[:, 2::4] = rng.normal(size=(T + 1, k)); X[:, 3::4] = rng.normal(size=(T + 1, k))
    if k == 1:
        return X
    for t in CASES[name]:
        X[t, 4] = X[t, 0] + 0.4 * r * np.cos(0.3 * t); X[t, 5] = X[t, 1] + 0.4 * r * np.sin(0.3 * t)
    if name in ("exact@7", "outside@7"):
        last = k - 1
        X[7, 0] = 0.0; X[7, 1] = 3.0; X[7, 4 * last + 1] = 3.0
        if k > 2:
            X[7, 4::4][: k - 2] = 50.0 + 10.0 * np.arange(k - 2)
        X[7, 4 * last] = r if name == "exact@7" else r * (1.0 + 2e-12)
        assert name == "exact@7" or X[7, 4 * last] > r
    return X


def near_steps(X, k, radius):
    """[B][T+1] bool: the sweep's criterion !(dx*dx + dy*dy > r*r*(1 + 1e-12)) for some pair (float64, no fused multiply-add)"""
    lim = (radius * radius * (1.0 + 1e-12))[:, None]
    near = np.zeros(X.shape[:2], dtype=bool)
    for i in range(k):
        for j in range(i + 1, k):
            ddx = X[:, :, 4 * i] - X[:, :, 4 * j]
            ddy = X[:, :, 4 * i + 1] - X[:, :, 4 * j + 1]
            s2 = ddx * ddx + ddy * ddy
            near |= ~(s2 > lim)
    return near


def last_near(near):
    """[B]: the largest t at which some pair is near, -1: none"""
    t = np.arange(near.shape[1])[None, :]
    return np.where(near, t, -1).max(1)


def build(k):
    """The 2100-item batch of k agents (the 1100-item launch is its first 1100 items): cases in shuffled order, per-item radius, mu,
    goal and controls; the duplicates; the two items with a non-finite entry at step 9, behind their last near step 6."""
    rng = np.random.default_rng(4100 + k)
    B = max(SIZES)
    case = rng.permutation(np.arange(B) % len(NAMES))
    for i, v in NONFINITE.items():
        case[i] = NAMES.index("one@6")
    radius = rng.uniform(0.3, 0.9, size=B)
    mu = rng.choice(MUS, size=B)
    xf = rng.normal(size=(B, 4 * k))
    U = rng.normal(size=(B, T, 2 * k)) * 0.3
    X = np.stack([trajectory(NAMES[case[i]], k, radius[i], rng) for i in range(B)])
    for src, dst in DUPLICATES:
        case[dst] = case[src]; radius[dst] = radius[src]; mu[dst] = mu[src]; xf[dst] = xf[src]; U[dst] = U[src]; X[dst] = X[src]
    for i, v in NONFINITE.items():
        X[i, 9, 2] = v                       # a velocity: the criterion does not see it, the step's l_x does
    return dict(case=case, radius=radius, mu=mu, xf=xf, U=U, X=X)


def passes(dp, k, fused=True, record_fed=True):
    """{(route, B): (K, d)} as host arrays, for both launch sizes"""
    from dpilqr_amd.device import to_dev
    c = build(k)
    out = {}
    for B in SIZES:
        pb = dp.ProblemBatch([0] * k, [2] * k, c["xf"][:B], Q, R, QF, c["radius"][:B], 0.1, T)
        mu = to_dev(c["mu"][:B].copy())
        if fused:
            K, d = pb.backward_pass_fused(c["X"][:B].copy(), c["U"][:B].copy(), mu)
            out["fused", B] = (K.cpu().numpy(), d.cpu().numpy())
        if record_fed:
            K, d = pb.backward_pass(c["X"][:B].copy(), c["U"][:B].copy(), mu)
            out["record", B] = (K.cpu().numpy(), d.cpu().numpy())
    return out


def windowed_solve(dp):
    """cfg2's scenario distribution and weights at T = 12: 3000 items through a window of 2100, six iterations"""
    from dpilqr_amd.util import random_setup_batch
    from tests.golden_util import cfg2_params
    c = cfg2_params()
    x0, xf = random_setup_batch((52000, 3000), 5, 4, var=2.5, n_d=2, energy=10.0)
    pb = dp.ProblemBatch(c["model"], c["n_dims"], xf.cpu().numpy(), c["Q"], c["R"], c["Qf"], c["radius"], c["dt"], T)
    r = pb.solve(x0, np.zeros((3000, T, 10)), n_lqr_iter=6, window=2100)
    return {key: r[key].cpu().numpy() for key in ("X", "U", "J", "status", "n_bwd", "n_fwd")}


def device_keys(dp, k):
    """dpilqr_cost_keys on the 2100-item batch of k agents, in index order and through a list (keys by list position)"""
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle, to_dev
    c = build(k)
    B = max(SIZES)
    pb = dp.ProblemBatch([0] * k, [2] * k, c["xf"], Q, R, QF, c["radius"], 0.1, T)
    Xd = to_dev(c["X"])
    keys = torch.full((B,), -7, dtype=torch.int32, device=Xd.device)
    _lib.check(_lib.load().dpilqr_cost_keys(pb._d, ptr(Xd), None, None, ptr(keys), stream_handle()))
    torch.cuda.synchronize()
    whole = keys.cpu().numpy().copy()
    items = torch.tensor(LISTED, dtype=torch.int32, device=Xd.device); cnt = torch.tensor([len(LISTED)], dtype=torch.int32, device=Xd.device)
    keys.fill_(-7)
    _lib.check(_lib.load().dpilqr_cost_keys(pb._d, ptr(Xd), ptr(items), ptr(cnt), ptr(keys), stream_handle()))
    torch.cuda.synchronize()
    return whole, keys.cpu().numpy()


def main(out_path):
    import dpilqr_amd as dp
    from dpilqr_amd import _lib
    _lib.require_gpu()
    out = {}
    for k in (2, 5):
        for (route, B), (K, d) in passes(dp, k, record_fed=False).items():
            out[f"K/{k}/{B}"] = K; out[f"d/{k}/{B}"] = d
    for k in (1, 2, 3, 5):        # (with DPILQR_KEYS_DENSE_STEPS in the environment: the key kernel's second output)
        out[f"keys/{k}"], out[f"keys_listed/{k}"] = device_keys(dp, k)
    for key, v in windowed_solve(dp).items():
        out[f"solve/{key}"] = v
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
