"""The team closed loop's host side, without a GPU: the conditions that keep the cases of tests/policy_dec_team_cases.py honest
(from the CPU reference alone) and its vectorised separation, the masks at k = 64, the argument checks of
dpilqr_policy_rollout_dec_team (fake, aligned device pointers, never dereferenced), the shape and mask checks of
ProblemBatch.policy_rollout_dec_team before any device call, the route DistributedPolicy.rollout takes by size, the kernels'
resources in the built library, and the refusals around it that stay."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_dec_cases as dc
from tests import policy_dec_team_cases as tc
from tests.policy_dec_wide_cases import kernel_name

ROOT = Path(__file__).resolve().parent.parent
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


# ---- the cases, from the reference alone
@pytest.mark.parametrize("case", tc.CASES, ids=tc.IDS)
def test_case_conditions(case):
    ref = tc.case_ref(case)
    f = ref.figures()
    print(case.id, f)
    assert 0.10 < f["clamped"] <= 0.90, f
    assert f["near"] >= 0.10, f
    assert f["moved"] >= 0.5, f
    assert all(u <= pc.MAX_UNCHECKED for u in f["unchecked"].values()), f


@pytest.mark.parametrize("case", tc.CASES + tc.CROSS, ids=tc.IDS + [c.id for c in tc.CROSS])
def test_vectorised_separation_is_policy_cases_separation(case):
    b = pc.make_batch(case)
    for x in (b["x0s"][0, 0], b["x0s"][2, case.S - 1], b["xf"][1]):
        assert tc.separation(x, case.k, case.ns, case.n_dims) == pc.separation(x, case.k, case.ns, case.n_dims)
    assert tc.separation(np.zeros(4), 1, 4, [2]) == np.inf


def test_every_case_lies_beyond_the_old_entry_and_the_cross_cases_within():
    assert all(c.k > 20 and c.k <= 64 for c in tc.CASES) and all(c.k * c.ns <= 60 and c.k <= 20 for c in tc.CROSS)
    assert [c.id for c in tc.CROSS] == ["dec-dint4_uni4-k5-S53", "dec-quad6_human6-k3-S6"]
    assert {(c.ns, c.nc) for c in tc.CASES} == {(3, 2), (4, 2), (6, 3), (12, 4)}
    assert len(set(tc.CROSS[1].n_dims)) == 2      # mixed n_dims


def test_masks_at_64_agents():
    case = next(c for c in tc.CASES if c.k == 64)
    k = 64
    m = dc.make_masks(case)
    assert m.dtype == np.uint64 and m.shape == (pc.B, k)
    assert all((int(m[b, a]) >> a) & 1 for b in range(pc.B) for a in range(k))                       # own bit everywhere
    assert all(int(v) == (1 << 64) - 1 for v in m[0]) and (m[0].view(np.int64) == -1).all()           # item 0 full
    assert all(int(m[1, a]) == 1 << a for a in range(k)) and m[1].view(np.int64)[63] < 0             # item 1 alone
    sizes = {dc.popcount(v) for v in m[2]}
    assert len(sizes) >= 2 and max(sizes) < k                                                        # item 2: max size < k
    assert any((int(m[2, a]) >> j) & 1 and not (int(m[2, j]) >> a) & 1 for a in range(k) for j in range(k))
    assert any((int(v) >> 63) & 1 for v in m[2][:63])      # bit 63 is a member of somebody else's neighbourhood too


# ---- the C ABI
def _desc(lib, k, ns=4, nc=2, B=2, T=10):
    return lib.BatchDesc(B, k, ns, nc, T, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)


def _call(lib, d, X=P, U=P, K=P, kc_max=2, bits=P, S=4, x0s=P, W=None, u_lim=None, Xs=None, Us=None, J=P, sep=None, goal=None):
    return lib.load().dpilqr_policy_rollout_dec_team(C.byref(d), X, U, K, kc_max, bits, S, x0s, W, u_lim, Xs, Us, J, sep, goal, None)


def test_symbol_is_declared_and_exported(lib):
    ext = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dpilqr_policy.h").read_text(), flags=re.S)
    name = "dpilqr_policy_rollout_dec_team"
    assert re.search(rf"\bint32_t\s+{name}\s*\(", ext)
    assert name in lib.EXT_SIGNATURES and hasattr(lib.load(), name)
    args = lambda n: [a.strip() for a in re.search(rf"{n}\s*\((.*?)\)\s*;", ext, re.S).group(1).split(",")]
    assert args(name) == args("dpilqr_policy_rollout_dec")                      # the argument list is identical
    assert lib.EXT_SIGNATURES[name] == lib.EXT_SIGNATURES["dpilqr_policy_rollout_dec"]
    assert lib.load().dpilqr_abi_version() == 4      # additive: the ABI version stays


def test_team_entry_argument_checks(lib):
    L = lib.load()
    d = _desc(lib, 64)
    assert L.dpilqr_policy_rollout_dec_team(None, P, P, P, 1, P, 1, P, None, None, None, None, P, None, None, None) == lib.EINVAL
    for name in ("X", "U", "K", "bits", "x0s", "J"):
        assert _call(lib, d, **{name: None}) == lib.EINVAL and b"NULL" in L.dpilqr_last_error(), name
        assert b"policy_rollout_dec_team" in L.dpilqr_last_error(), name
    for name in ("X", "U", "K", "bits", "x0s", "W", "u_lim", "Xs", "Us", "J", "sep", "goal"):      # every pointer
        assert _call(lib, d, **{name: P + 4}) == lib.EINVAL and b"aligned" in L.dpilqr_last_error(), name
    assert _call(lib, _desc(lib, 65)) == lib.EUNSUPPORTED and b"k=65" in L.dpilqr_last_error()
    assert _call(lib, _desc(lib, 13, 5, 2)) == lib.EUNSUPPORTED and b"BikeDynamics5D" in L.dpilqr_last_error()      # dpilqr_rollout's bike limit
    assert _call(lib, _desc(lib, 30, 7, 2)) == lib.EINVAL and b"model family" in L.dpilqr_last_error()             # no such family
    assert _call(lib, d, S=0) == lib.EINVAL and b"n_samples=0" in L.dpilqr_last_error()
    assert _call(lib, d, S=-3) == lib.EINVAL
    for kc_max in (0, -1, 65):
        assert _call(lib, d, kc_max=kc_max) == lib.EUNSUPPORTED and b"kc_max" in L.dpilqr_last_error()
    # more than 2^31 - 1 workgroups: 4 samples of 64 agents per workgroup
    assert _call(lib, _desc(lib, 64, B=8), S=(1 << 30) + 1, kc_max=64) == lib.EUNSUPPORTED and b"workgroups" in L.dpilqr_last_error()
    # an empty batch: nothing to launch, whatever the team's size within the limits
    for k, ns, nc in ((64, 4, 2), (21, 12, 4), (12, 5, 2), (1, 3, 2)):
        assert _call(lib, _desc(lib, k, ns, nc, B=0), kc_max=k) == lib.OK, (k, ns, nc)


# ---- the Python wrapper: every error before the device is touched
def _bare_batch(B=2, T=6, k=3, ns=4, nc=2):
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)      # no device state at all
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = B, T, k, ns, nc, k * ns, k * nc
    return pb


def test_policy_rollout_dec_team_validates_on_the_host():
    pb = _bare_batch()
    X, U, Kc = np.zeros((2, 7, 12)), np.zeros((2, 6, 6)), np.zeros((2, 6, 3, 2, 8))
    bits = np.array([[3, 3, 4], [1, 6, 5]], dtype=np.uint64)
    x0s = np.zeros((2, 5, 12))
    S, kc_max, b64 = pb._policy_dec_team_shapes(X, U, Kc, bits, x0s, None, None)
    assert (S, kc_max) == (5, 2) and b64.dtype == np.int64 and np.array_equal(b64, bits.astype(np.int64))
    assert pb._policy_dec_team_shapes(X, U, Kc, bits.astype(np.int64), x0s, np.zeros((2, 5, 6, 12)), np.array([[-1.0] * 6, [1.0] * 6]))[0] == 5
    bad = [dict(X=X[:, :6]), dict(U_ff=U[:, :, :5]), dict(Kc=np.zeros((2, 6, 6, 12))), dict(Kc=np.zeros((2, 6, 3, 2, 7))),
           dict(Kc=np.zeros((2, 6, 3, 2, 16))), dict(Kc=np.zeros((2, 6, 3, 2, 0))), dict(nbr_bits=bits[:, :2]),
           dict(nbr_bits=bits.astype(np.float64)), dict(x0s=np.zeros((2, 12))), dict(x0s=np.zeros((2, 0, 12))),
           dict(W=np.zeros((2, 5, 7, 12))), dict(u_lim=np.zeros((6, 2))), dict(u_lim=np.array([[1.0] * 6, [-1.0] * 6])),
           dict(nbr_bits=np.array([[3, 3, 4], [1, 4, 5]], dtype=np.uint64)),       # agent 1 of item 1 lacks its own bit
           dict(nbr_bits=np.array([[3, 3, 4], [7, 6, 5]], dtype=np.uint64))]       # three members, kc_max = 2
    for kw in bad:
        a = dict(X=X, U_ff=U, Kc=Kc, nbr_bits=bits, x0s=x0s, W=None, u_lim=None); a.update(kw)
        with pytest.raises(ValueError, match="policy_rollout_dec_team"):
            pb.policy_rollout_dec_team(a["X"], a["U_ff"], a["Kc"], a["nbr_bits"], a["x0s"], W=a["W"], u_lim=a["u_lim"])
    with pytest.raises(ValueError, match="own bit"):
        pb.policy_rollout_dec_team(X, U, Kc, np.array([[3, 3, 4], [1, 4, 5]], dtype=np.uint64), x0s)
    with pytest.raises(ValueError, match="3 members"):
        pb.policy_rollout_dec_team(X, U, Kc, np.array([[3, 3, 4], [7, 6, 5]], dtype=np.uint64), x0s)


def test_masks_of_64_agents_given_as_negative_int64_are_accepted():
    k, ns, nc, T = 64, 4, 2, 3
    pb = _bare_batch(B=3, T=T, k=k, ns=ns, nc=nc)
    case = next(c for c in tc.CASES if c.k == 64)
    masks = dc.make_masks(case)
    as_i64 = masks.view(np.int64)
    assert (as_i64 < 0).any() and (as_i64[0] == -1).all()
    args = lambda bits, kc=k: (np.zeros((3, T + 1, k * ns)), np.zeros((3, T, k * nc)), np.zeros((3, T, k, nc, kc * ns)), bits, np.zeros((3, 2, k * ns)), None, None)
    for given in (as_i64, masks):
        S, kc_max, b64 = pb._policy_dec_team_shapes(*args(given))
        assert (S, kc_max) == (2, 64) and b64.dtype == np.int64 and np.array_equal(b64.view(np.uint64), masks)
    # bit 63 counts as a member and as an own bit
    true_max = max(dc.popcount(v) for v in masks[1:].reshape(-1))
    pb2 = _bare_batch(B=2, T=T, k=k, ns=ns, nc=nc)
    sub = lambda bits, kc: (np.zeros((2, T + 1, k * ns)), np.zeros((2, T, k * nc)), np.zeros((2, T, k, nc, kc * ns)), bits, np.zeros((2, 2, k * ns)), None, None)
    assert pb2._policy_dec_team_shapes(*sub(as_i64[1:], true_max))[1] == true_max
    with pytest.raises(ValueError, match=f"{true_max} members"):
        pb2._policy_dec_team_shapes(*sub(as_i64[1:], true_max - 1))
    lacking = as_i64[1:].copy()
    lacking[0, 63] = 1      # agent 63 without bit 63
    with pytest.raises(ValueError, match="own bit"):
        pb2._policy_dec_team_shapes(*sub(lacking, true_max))
    alone63 = np.zeros((2, k), dtype=np.int64)
    alone63[:] = as_i64[1]
    alone63[:, 62] |= np.int64(-2 ** 63)      # agent 62 sees agent 63: two members, the sign bit one of them
    assert pb2._policy_dec_team_shapes(*sub(alone63, 2))[1] == 2
    with pytest.raises(ValueError, match="2 members"):
        pb2._policy_dec_team_shapes(*sub(alone63, 1))


def test_65_agents_and_13_bikes_are_refused():
    pb = _bare_batch(k=65)
    with pytest.raises(ValueError, match="policy_rollout_dec_team serves teams of up to 64 agents.*k = 65"):
        pb.policy_rollout_dec_team(np.zeros((2, 7, 260)), np.zeros((2, 6, 130)), np.zeros((2, 6, 65, 2, 4)), np.ones((2, 65), dtype=np.int64),
                                   np.zeros((2, 5, 260)))
    pb = _bare_batch(k=13, ns=5, nc=2)
    with pytest.raises(ValueError, match="policy_rollout_dec_team.*five-state.*k = 13"):
        pb.policy_rollout_dec_team(np.zeros((2, 7, 65)), np.zeros((2, 6, 26)), np.zeros((2, 6, 13, 2, 5)), np.ones((2, 13), dtype=np.int64),
                                   np.zeros((2, 5, 65)))


# ---- DistributedPolicy.rollout routes by size
class _StubBatch:
    def __init__(self):
        self.calls = []

    def policy_rollout_dec(self, *a, **kw):
        self.calls.append(("policy_rollout_dec", a, kw))
        return "dec"

    def policy_rollout_dec_team(self, *a, **kw):
        self.calls.append(("policy_rollout_dec_team", a, kw))
        return "team"


@pytest.mark.parametrize("k,ns,want", [(20, 3, "policy_rollout_dec"), (15, 4, "policy_rollout_dec"), (3, 4, "policy_rollout_dec"),
                                       (21, 3, "policy_rollout_dec_team"), (16, 4, "policy_rollout_dec_team"),
                                       (64, 4, "policy_rollout_dec_team"), (6, 12, "policy_rollout_dec_team")])
def test_distributed_policy_rollout_routes_by_size(k, ns, want):
    from dpilqr_amd.dispatch import DistributedPolicy
    nc, T, S = 2, 4, 2
    X_dec, U_ff, Kc, bits = np.zeros((S, T + 1, k * ns)), np.zeros((S, T, k * nc)), np.zeros((S, T, k, nc, ns)), np.ones((S, k), dtype=np.int64)
    pol = DistributedPolicy(dict(k=k), None, X_dec, U_ff, Kc, bits, 1)
    stub = pol._batch = _StubBatch()
    x0s, W, lim = np.zeros((S, 3, k * ns)), np.zeros((S, 3, T, k * ns)), np.zeros((2, k * nc))
    assert pol.rollout(x0s, W=W, u_lim=lim, trajectories=True) == ("dec" if want == "policy_rollout_dec" else "team")
    pol.rollout(x0s)
    assert [c[0] for c in stub.calls] == [want, want]
    name, a, kw = stub.calls[0]
    assert a[0] is X_dec and a[1] is U_ff and a[2] is Kc and a[3] is bits and a[4] is x0s
    assert kw["W"] is W and kw["u_lim"] is lim and kw["trajectories"] is True and kw["masks_checked"] is None
    assert stub.calls[1][2]["masks_checked"] is bits and stub.calls[1][2]["trajectories"] is False      # checked by the first call only
    with pytest.raises(ValueError, match="DistributedPolicy.rollout"):
        pol.rollout(np.zeros((S, 3, k * ns + 1)))


# ---- the kernels in the built library
@pytest.fixture(scope="module")
def table(lib):
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("ns,nc", [(3, 2), (4, 2), (5, 2), (6, 3), (12, 4)])
def test_team_kernels_keep_every_register(table, ns, nc):
    r = table[kernel_name(f"k_policy_rollout_dec_team<{ns}, {nc}>")]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256, r
    # static LDS: 256 (ns | 1) + 256 * 3 + 256 doubles and 64 ints (and the compiler's padding between them), under 64 KB
    assert 8 * 256 * ((ns | 1) + 4) + 4 * 64 <= r["group_segment_fixed_size"] < 64 * 1024, r


def test_no_further_team_kernel_was_built(table):
    """One kernel text, two word counts: the five one-word instantiations, the five four-word ones, and nothing else."""
    names = sorted(n for n in table if "k_policy_rollout_dec_team" in n or "k_policy_rollout_dec_wide" in n)
    assert names == sorted(kernel_name(f"k_policy_rollout_dec_{width}<{ns}, {nc}>") for width in ("team", "wide")
                           for ns, nc in ((3, 2), (4, 2), (5, 2), (6, 3), (12, 4)))


# ---- what stays exactly as it is
def _problem(k):
    import dpilqr_amd as dp
    dp._reset_ids()
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(np.zeros(4), np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k)))


def test_the_pinned_refusals_still_raise(lib):
    import dpilqr_amd as dp
    from dpilqr_amd.dispatch import DistributedPolicy, ScenarioFrontEnd, solve_scenarios_distributed
    from dpilqr_amd.util import random_setup_batch
    # policy_rollout_dec and policy_advance_dec beyond n_x <= 60, k <= 20
    for k, ns in ((16, 4), (20, 4), (21, 3)):
        pb = _bare_batch(k=k, ns=ns)
        n, m = pb.n_x, pb.n_u
        with pytest.raises(ValueError, match="policy_rollout_dec serves clusters up to n_x = 60 and k = 20"):
            pb.policy_rollout_dec(np.zeros((2, 7, n)), np.zeros((2, 6, m)), np.zeros((2, 6, k, 2, ns)), np.ones((2, k), dtype=np.int64), np.zeros((2, 5, n)))
        with pytest.raises(ValueError, match="policy_advance_dec serves clusters up to n_x = 60 and k = 20"):
            pb.policy_advance_dec(np.zeros((2, 7, n)), np.zeros((2, 6, m)), np.zeros((2, 6, k, 2, ns)), np.ones((2, k), dtype=np.int64), 1, {})
    # DistributedPolicy.advance for a large team keeps raising (policy_advance_dec's refusal)
    k = 24
    pol = DistributedPolicy(dict(k=k), None, np.zeros((2, 7, 4 * k)), np.zeros((2, 6, 2 * k)), np.zeros((2, 6, k, 2, 4)), np.ones((2, k), dtype=np.int64), 1)
    pol._batch = _bare_batch(k=k)
    with pytest.raises(ValueError, match="policy_advance_dec serves clusters up to n_x = 60"):
        pol.advance(1, {})
    # solve_rhc_closed_loop beyond n_x = 60
    big = _problem(16)
    with pytest.raises(ValueError, match="n_x = 60.*large=True"):
        dp.solve_rhc_closed_loop(big, np.zeros((2, 64)), 10, dist_converge=0.1, max_steps=4)
    with pytest.raises(ValueError, match="large=True.*distributed loop.*not built"):
        dp.solve_rhc_closed_loop(big, np.zeros((2, 64)), 10, radius=1.0, dist_converge=0.1, max_steps=4, centralized=False, large=True)
    # teams of more than 64 agents
    p65, T = _problem(65), 4
    X, U = np.zeros((2, 1, 65 * 4)), np.zeros((2, T, 65 * 2))
    with pytest.raises(ValueError, match=r"policy=True is not built for teams of more than 64 agents \(this one has 65\)"):
        solve_scenarios_distributed(p65, X, U, 0.5, policy=True)
    with pytest.raises(ValueError, match=r"shard= is not built for teams of more than 64 agents \(this one has 65\)"):
        solve_scenarios_distributed(p65, X, U, 0.5, shard=(0, 2))
    with pytest.raises(ValueError, match="65 agents"):
        random_setup_batch((0, 4), 65, 4, 1.0)
    with pytest.raises(ValueError, match="solve_rhc_scenarios is not built for teams of more than 64 agents"):
        dp.distributed.solve_rhc_scenarios(p65, np.zeros((2, 65 * 4)), T, 0.5, dist_converge=0.1)
    fe = ScenarioFrontEnd.__new__(ScenarioFrontEnd)      # a wide front end, no device state
    fe.k, fe.wide = 65, True
    with pytest.raises(ValueError, match="stitch_policy is not built for teams of more than 64 agents"):
        fe.stitch_policy({}, {}, None)
    assert lib.load().dpilqr_abi_version() == 4
