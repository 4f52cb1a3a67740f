"""The distributed closed loop's host side, without a GPU: the conditions that keep the cases of tests/policy_dec_cases.py honest
(from the CPU reference alone), the declarations and argument checks of dpilqr_policy_rollout_dec and
dpilqr_dispatch_stitch_policy (fake, aligned device pointers, never dereferenced), the shape and mask checks of the three
Python wrappers before any device call, and the kernels' resources in the built library."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_dec_cases as dc

ROOT = Path(__file__).resolve().parent.parent
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


# ---- the cases, from the reference alone
@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_case_conditions(case):
    ref = dc.case_ref(case)
    f = ref.figures()
    print(case.id, f)
    assert 0.10 < f["clamped"] <= 0.90, f
    if case.k >= 2:
        assert f["near"] >= 0.10, f
    assert f["moved"] >= 0.5, f
    assert all(u <= pc.MAX_UNCHECKED for u in f["unchecked"].values()), f


@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_masks(case):
    k = case.k
    m = dc.make_masks(case)
    assert all((int(m[b, a]) >> a) & 1 for b in range(pc.B) for a in range(k))
    assert all(int(v) == (1 << k) - 1 for v in m[0]) and all(int(m[1, a]) == 1 << a for a in range(k))
    if k > 1:
        sizes = {dc.popcount(v) for v in m[2]}
        assert len(sizes) >= 2 and max(sizes) < k
        assert any((int(m[2, a]) >> j) & 1 and not (int(m[2, j]) >> a) & 1 for a in range(k) for j in range(k))
    # compact and masked gains say the same thing
    rng = np.random.default_rng(0)
    K = rng.normal(size=(pc.B, 2, k * case.nc, k * case.ns))
    Km, Kc = dc.mask_gains(K, m, case.ns, case.nc), dc.compact_gains(K, m, case.ns, case.nc, k, fill=0.0)
    assert np.array_equal(Kc[0].reshape(2, k * case.nc, k * case.ns), K[0]) and np.array_equal(Km[0], K[0])
    dx = rng.normal(size=k * case.ns)
    for b in range(pc.B):
        for a in range(k):
            cols = np.concatenate([dx[j * case.ns:(j + 1) * case.ns] for j in dc.members(m[b, a], k)])
            assert np.allclose(Kc[b, 0, a, :, :cols.size] @ cols, Km[b, 0, a * case.nc:(a + 1) * case.nc] @ dx, rtol=1e-13, atol=1e-13)


# ---- the C ABI
def _desc(lib, k, ns, nc, B=2, T=10):
    return lib.BatchDesc(B, k, ns, nc, T, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)


def _call(lib, d, X=P, U=P, K=P, kc_max=2, bits=P, S=4, x0s=P, W=None, u_lim=None, Xs=None, Us=None, J=P, sep=None, goal=None):
    return lib.load().dpilqr_policy_rollout_dec(C.byref(d), X, U, K, kc_max, bits, S, x0s, W, u_lim, Xs, Us, J, sep, goal, None)


def test_symbols_are_declared_and_exported(lib):
    ext = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dpilqr_policy.h").read_text(), flags=re.S)
    for name in ("dpilqr_policy_rollout_dec", "dpilqr_dispatch_stitch_policy"):
        assert re.search(rf"\bint32_t\s+{name}\s*\(", ext)
        assert name in lib.EXT_SIGNATURES and hasattr(lib.load(), name)
        n_args = len(re.search(rf"{name}\s*\((.*?)\)\s*;", ext, re.S).group(1).split(","))
        assert n_args == len(lib.EXT_SIGNATURES[name][1]), name
    assert "dpilqr_bucket_gains" in ext
    assert C.sizeof(lib.BucketGains) == 8 * (lib.MAX_AGENTS + 1)
    assert lib.load().dpilqr_abi_version() == 4      # additive: the ABI version stays


def test_rollout_dec_limits_and_bad_arguments(lib):
    L = lib.load()
    for k, ns, nc in ((16, 4, 2), (11, 6, 3), (6, 12, 4), (21, 3, 2)):
        assert _call(lib, _desc(lib, k, ns, nc)) == lib.EUNSUPPORTED
        assert b"policy_rollout_dec" in L.dpilqr_last_error()
    d = _desc(lib, 5, 4, 2)
    for kc_max in (0, -1, 6):
        assert _call(lib, d, kc_max=kc_max) == lib.EUNSUPPORTED and b"kc_max" in L.dpilqr_last_error()
    for name in ("X", "U", "K", "bits", "x0s", "J"):
        assert _call(lib, d, **{name: None}) == lib.EINVAL and b"NULL" in L.dpilqr_last_error(), name
    assert _call(lib, d, S=0) == lib.EINVAL and b"n_samples=0" in L.dpilqr_last_error()
    for name in ("X", "U", "K", "bits", "x0s", "W", "u_lim", "Xs", "Us", "J", "sep", "goal"):
        assert _call(lib, d, **{name: P + 4}) == lib.EINVAL and b"aligned" in L.dpilqr_last_error(), name
    assert L.dpilqr_policy_rollout_dec(None, P, P, P, 1, P, 1, P, None, None, None, None, P, None, None, None) == lib.EINVAL
    assert _call(lib, _desc(lib, 5, 4, 2, B=0), kc_max=5) == lib.OK      # an empty batch: nothing to launch


def test_stitch_policy_bad_arguments(lib):
    L = lib.load()
    R, G = lib.BucketResults(), lib.BucketGains()
    call = lambda S=3, k=4, kc_max=2, bits=P, R_=R, G_=G, X=P, Kc=P, U=P: L.dpilqr_dispatch_stitch_policy(
        S, k, 4, 2, 12, kc_max, bits, P, P, P, C.addressof(R_) if R_ is not None else None, C.addressof(G_) if G_ is not None else None,
        X, Kc, U, None)
    assert call(S=0) == lib.OK
    for kw in (dict(k=0), dict(k=65), dict(bits=None), dict(R_=None), dict(G_=None), dict(X=None), dict(Kc=None), dict(U=None),
               dict(kc_max=0), dict(kc_max=5), dict(S=-1)):
        assert call(**kw) == lib.EINVAL, kw
        assert b"dispatch_stitch_policy" in L.dpilqr_last_error()
    R.count[3] = 2; R.X[3] = P; R.U[3] = P; G.K[3] = P
    assert call(S=0, kc_max=2) == lib.EINVAL and b"kc_max" in L.dpilqr_last_error()      # a populated size above kc_max
    G.K[3] = None
    assert call(S=0, kc_max=3) == lib.EINVAL and b"NULL" in L.dpilqr_last_error()


# ---- the Python wrappers: every error before the device is touched
def _bare_batch():
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)      # no device state at all
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 2, 6, 3, 4, 2, 12, 6
    return pb


def test_policy_rollout_dec_validates_on_the_host():
    pb = _bare_batch()
    X, U, Kc = np.zeros((2, 7, 12)), np.zeros((2, 6, 6)), np.zeros((2, 6, 3, 2, 8))
    bits = np.array([[3, 3, 4], [1, 6, 5]], dtype=np.uint64)
    x0s = np.zeros((2, 5, 12))
    S, kc_max, b64 = pb._policy_dec_shapes(X, U, Kc, bits, x0s, None, None)
    assert (S, kc_max) == (5, 2) and b64.dtype == np.int64 and np.array_equal(b64, bits.astype(np.int64))
    assert pb._policy_dec_shapes(X, U, Kc, bits.astype(np.int64), x0s, np.zeros((2, 5, 6, 12)), np.array([[-1.0] * 6, [1.0] * 6]))[0] == 5
    bad = [dict(X=X[:, :6]), dict(U_ff=U[:, :, :5]), dict(Kc=np.zeros((2, 6, 6, 12))), dict(Kc=np.zeros((2, 6, 3, 2, 7))),
           dict(Kc=np.zeros((2, 6, 3, 2, 16))), dict(Kc=np.zeros((2, 6, 3, 2, 0))), dict(nbr_bits=bits[:, :2]),
           dict(nbr_bits=bits.astype(np.float64)), dict(x0s=np.zeros((2, 12))), dict(x0s=np.zeros((2, 0, 12))),
           dict(W=np.zeros((2, 5, 7, 12))), dict(u_lim=np.zeros((6, 2))), dict(u_lim=np.array([[1.0] * 6, [-1.0] * 6])),
           dict(nbr_bits=np.array([[3, 3, 4], [1, 4, 5]], dtype=np.uint64)),       # agent 1 of item 1 lacks its own bit
           dict(nbr_bits=np.array([[3, 3, 4], [7, 6, 5]], dtype=np.uint64))]       # three members, kc_max = 2
    for kw in bad:
        a = dict(X=X, U_ff=U, Kc=Kc, nbr_bits=bits, x0s=x0s, W=None, u_lim=None); a.update(kw)
        with pytest.raises(ValueError, match="policy_rollout_dec"):
            pb.policy_rollout_dec(a["X"], a["U_ff"], a["Kc"], a["nbr_bits"], a["x0s"], W=a["W"], u_lim=a["u_lim"])
    with pytest.raises(ValueError, match="own bit"):
        pb.policy_rollout_dec(X, U, Kc, np.array([[3, 3, 4], [1, 4, 5]], dtype=np.uint64), x0s)
    pb.k, pb.n_x, pb.n_u = 16, 64, 32
    with pytest.raises(ValueError, match="n_x = 60"):
        pb.policy_rollout_dec(np.zeros((2, 7, 64)), np.zeros((2, 6, 32)), np.zeros((2, 6, 16, 2, 4)), np.ones((2, 16), dtype=np.int64), np.zeros((2, 5, 64)))


def test_distributed_policy_rollout_validates_x0s():
    from dpilqr_amd.dispatch import DistributedPolicy
    pol = DistributedPolicy(dict(k=3), None, np.zeros((2, 7, 12)), np.zeros((2, 6, 6)), np.zeros((2, 6, 3, 2, 8)), np.ones((2, 3), dtype=np.int64), 2)
    assert pol.kc_max == 2
    for x0s in (np.zeros((5, 12)), np.zeros((3, 5, 12)), np.zeros((2, 5, 11)), np.zeros((2, 0, 12))):
        with pytest.raises(ValueError, match="DistributedPolicy.rollout"):
            pol.rollout(x0s)


def _problem(k=3):
    import dpilqr_amd as dp
    dp._reset_ids()
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(np.zeros(4), np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k)))


def test_policy_with_shard_or_ignore_ids_raises():
    import dpilqr_amd as dp
    prob = _problem()
    X, U = np.zeros((1, 1, 12)), np.zeros((1, 5, 6))
    with pytest.raises(ValueError, match="policy=True"):
        dp.solve_scenarios_distributed(prob, X, U, 0.5, policy=True, shard=(0, 2))
    with pytest.raises(ValueError, match="policy=True"):
        dp.solve_scenarios_distributed(prob, X, U, 0.5, policy=True, ignore_ids=[prob.ids[0]])


def test_default_signature_is_unchanged():
    import dpilqr_amd as dp
    sig = inspect.signature(dp.solve_scenarios_distributed)
    names = list(sig.parameters)
    assert names == ["problem", "X", "U", "radius", "xf", "window", "concurrent", "ignore_ids", "device_out", "shard", "audit", "desc",
                     "policy", "policy_mu", "kwargs"]
    assert sig.parameters["policy"].default is False and sig.parameters["policy_mu"].default == 0.0
    assert dp.closed_loop_distributed is dp.distributed.closed_loop_distributed and dp.DistributedPolicy is dp.dispatch.DistributedPolicy


def test_closed_loop_distributed_argument_errors():
    import dpilqr_amd as dp
    prob = _problem()
    with pytest.raises(ValueError, match="x0s"):
        dp.closed_loop_distributed(prob, np.zeros((6, 12)), np.zeros((5, 6)), 0.5, np.zeros((4, 11)))
    with pytest.raises(ValueError, match="closed_loop_distributed"):
        dp.closed_loop_distributed(prob, np.zeros((5, 12)), np.zeros((5, 6)), 0.5, np.zeros((4, 12)))

    class HostModel(dp.DynamicalModel):
        def __init__(self):
            super().__init__(4, 2, 0.1)

        def f(self, x, u):
            return np.zeros(4)

        def linearize(self, x, u):
            return np.eye(4), np.zeros((4, 2))

    dp._reset_ids()
    cost = dp.GameCost([dp.ReferenceCost(np.zeros(4), np.eye(4), np.eye(2), np.eye(4), 0)], dp.ProximityCost([4], 0.5, [2]))
    with pytest.raises(NotImplementedError, match="host plugins"):
        dp.closed_loop_distributed(dp.ilqrProblem(HostModel(), cost), np.zeros((6, 4)), np.zeros((5, 2)), 0.5, np.zeros((3, 4)))


# ---- the kernels in the built library
@pytest.fixture(scope="module")
def table(lib):
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("ns,nc", [(3, 2), (4, 2), (5, 2), (6, 3)])
def test_dec_kernels_do_not_spill(table, ns, nc):
    r = table[f"k_policy_rollout_dec<{ns}, {nc}>"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256 and r["group_segment_fixed_size"] == 0, r      # LDS is sized by the launcher


def test_twelve_state_dec_kernel_is_no_worse_than_the_dense_one(table):
    r, yard = table["k_policy_rollout_dec<12, 4>"], table["k_policy_rollout<12, 4>"]
    assert r["private_segment_fixed_size"] <= yard["private_segment_fixed_size"], (r, yard)
    assert r["vgpr_spill_count"] <= yard["vgpr_spill_count"], (r, yard)
