"""The closed-loop rollout for teams of up to 256 agents, the host side, without a GPU: the conditions that keep the cases of
tests/policy_dec_wide_cases.py honest (from the CPU reference alone), the structure of their multi-word masks, the compact-gain
layout against a dense product, the two new entries of include/dpilqr_swarm_policy.h (declared, bound, exported; every refusal
before any launch, with fake, aligned device pointers that are never dereferenced), the Python layers' refusals before any
device work, and the new kernels' resources in the built library."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_dec_wide_cases as wc

ROOT = Path(__file__).resolve().parent.parent
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test
NAMES = {"dpilqr_dispatch_stitch_policy_wide": 17, "dpilqr_policy_rollout_dec_wide": 17}
FAMILIES = [(3, 2), (4, 2), (5, 2), (6, 3), (12, 4)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


# ---- the cases, from the reference alone
@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_case_conditions(case):
    ref = wc.case_ref(case)
    f = ref.figures()
    print(case.id, f)
    assert 0.10 < f["clamped"] <= 0.90, f
    assert f["near"] >= 0.10, f
    assert f["moved"] >= 0.5, f
    assert all(u <= pc.MAX_UNCHECKED for u in f["unchecked"].values()), f


def test_the_cases_are_the_shapes_the_kernel_can_go_wrong_at():
    by = {c.id: c for c in wc.CASES}
    assert [(c.k, c.S, c.kc_max, c.n_words) for c in wc.CASES] == [(65, 4, 8, 2), (86, 3, 5, 2), (65, 3, 4, 2), (65, 2, 3, 2), (129, 2, 8, 3),
                                                                     (256, 2, 8, 4)]
    assert {(c.ns, c.nc) for c in wc.CASES} == {(3, 2), (4, 2), (12, 4)}
    assert 256 // 65 == 3 and by["wide-dint4-k65-S4"].S > 3          # a second workgroup that holds one sample
    assert 256 // 86 == 2 and 256 // 129 == 1
    assert len(set(by["wide-dint4_uni4-k86-S3"].models)) == 2 and by["wide-dint4_uni4-k86-S3"].weights == "per_item"
    assert by["wide-quad12-k65-S2"].n_dims == [3] * 65


@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_mask_structure(case):
    k, kc_max, nw = case.k, case.kc_max, case.n_words
    mem = wc.make_members(case)
    words = wc.words_of(mem, k)
    assert words.shape == (pc.B, k, nw) and words.dtype == np.uint64
    for b in range(pc.B):
        assert wc.members_of(words[b], k) == mem[b]                                      # the words say what the lists say
        assert all(a in mem[b][a] and mem[b][a] == sorted(set(mem[b][a])) and max(mem[b][a]) < k for a in range(k))
    assert all(len(m) == kc_max for m in mem[0])                                        # item 0: exactly kc_max members
    assert mem[1] == [[a] for a in range(k)]                                            # item 1: alone
    sizes = {len(m) for m in mem[2]}
    assert sizes <= set(range(1, kc_max)) and len(sizes) >= 2                           # item 2: 1 .. kc_max - 1
    assert any(j != a and a not in mem[2][j] for a in range(k) for j in mem[2][a])      # ... asymmetric
    # members on both sides of bit 64 in one neighbourhood; the top agent and every word edge in somebody else's
    assert any(min(m) < 64 <= max(m) for m in mem[0])
    for e in (0, 63, 64, k - 1):
        assert any(e in mem[0][a] for a in range(k) if a != e), e
    assert int(words[0, :, nw - 1].max()) >> ((k - 1) % 64) == 1                         # bit k - 1 is the highest bit anywhere
    # nothing at or past bit k
    top = (k - 1) % 64 + 1
    assert top == 64 or not (words[:, :, nw - 1] >> np.uint64(top)).any()


def test_compact_gains_and_member_lists_are_a_dense_product():
    case = wc.CASES[0]
    k, ns, nc, kc_max = case.k, case.ns, case.nc, case.kc_max
    rng = np.random.default_rng(3)
    for mem in wc.make_members(case):
        Kc = rng.normal(size=(k, nc, kc_max * ns))
        for a, m in enumerate(mem):
            Kc[a, :, len(m) * ns:] = np.nan                                             # never read
        U, dx = rng.normal(size=k * nc), rng.normal(size=k * ns)
        idx, used = wc.gather_index(mem, ns, kc_max)
        got = wc.apply_law(U, Kc, idx, used, dx)
        want = U + wc.dense_gains(Kc, mem, ns, nc) @ dx
        assert np.isfinite(got).all() and np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


def test_case_gains_are_the_sub_problems_rows():
    """Agent a's compact rows are rows pos of the backward pass of its own neighbourhood's sub-problem; the rest is NaN."""
    case = wc.CASES[0]
    ref = wc.case_ref(case)
    ns, nc = case.ns, case.nc
    for i, a in ((0, 0), (0, 64), (1, 7), (2, 33)):
        mem = ref.members[i][a]
        K = wc.sub_gains(ref.batch, i, ref.X[i], ref.U[i], mem, ns, nc)
        pos = mem.index(a)
        assert np.array_equal(ref.Kc[i, :, a, :, :len(mem) * ns], K[:, pos * nc:(pos + 1) * nc, :])
        assert np.isnan(ref.Kc[i, :, a, :, len(mem) * ns:]).all()


# ---- the C ABI
def _desc(lib, k, ns=4, nc=2, B=2, T=10):
    return lib.BatchDesc(B, k, ns, nc, T, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)


def _call(lib, d, X=P, U=P, K=P, kc_max=2, bits=P, S=4, x0s=P, W=None, u_lim=None, Xs=None, Us=None, J=P, sep=None, goal=None, n_words=None):
    n_words = (d.k + 63) // 64 if n_words is None else n_words
    return lib.load().dpilqr_policy_rollout_dec_wide(C.byref(d), X, U, K, kc_max, bits, S, x0s, W, u_lim, Xs, Us, J, sep, goal, n_words, None)


def test_symbols_are_declared_bound_and_exported(lib):
    """Fails on a build without the feature: there is no include/dpilqr_swarm_policy.h, no binding and no symbol."""
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    core, ext = strip((ROOT / "include" / "dpilqr_hip.h").read_text()), strip((ROOT / "include" / "dpilqr_swarm_policy.h").read_text())
    assert re.search(r'^\s*#\s*include\s+"dpilqr_swarm_policy.h"', core, re.M)
    decl = dict(re.findall(r"\bint32_t\s+(dpilqr_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", ext))
    assert sorted(decl) == sorted(NAMES) == sorted(lib.SWARM_POLICY_SIGNATURES)
    assert not set(lib.SWARM_POLICY_SIGNATURES) & (set(lib.SIGNATURES) | set(lib.EXT_SIGNATURES) | set(lib.SWARM_SIGNATURES))
    for name, n_args in NAMES.items():
        assert len(decl[name].split(",")) == n_args == len(lib.SWARM_POLICY_SIGNATURES[name][1]), name
        fn = getattr(lib.load(), name)
        assert fn.argtypes == lib.SWARM_POLICY_SIGNATURES[name][1] and fn.restype is C.c_int32
    # each entry: its one-word counterpart's arguments plus n_words before the stream
    for wide, narrow in (("dpilqr_dispatch_stitch_policy_wide", "dpilqr_dispatch_stitch_policy"),
                         ("dpilqr_policy_rollout_dec_wide", "dpilqr_policy_rollout_dec_team")):
        assert lib.SWARM_POLICY_SIGNATURES[wide][1] == lib.EXT_SIGNATURES[narrow][1][:-1] + [C.c_int32, C.c_void_p]
        narrow_decl = strip((ROOT / "include" / "dpilqr_policy.h").read_text())
        args = lambda text, n: [" ".join(a.split()) for a in re.search(rf"\b{n}\s*\((.*?)\)\s*;", text, re.S).group(1).split(",")]
        assert args(ext, wide) == args(narrow_decl, narrow)[:-1] + ["int32_t n_words", "void* stream"]
    assert lib.load().dpilqr_abi_version() == 4 and lib.ABI_VERSION == 4      # additive: the ABI version stays


def test_the_header_compiles_as_c(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dpilqr_hip.h"\nvoid* p[] = {(void*)dpilqr_policy_rollout_dec_wide, (void*)dpilqr_dispatch_stitch_policy_wide};\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_rollout_entry_argument_checks(lib):
    L = lib.load()
    d = _desc(lib, 130)
    who = b"policy_rollout_dec_wide"
    assert L.dpilqr_policy_rollout_dec_wide(None, P, P, P, 1, P, 1, P, None, None, None, None, P, None, None, 1, None) == lib.EINVAL
    for name in ("X", "U", "K", "bits", "x0s", "J"):
        assert _call(lib, d, **{name: None}) == lib.EINVAL and b"NULL" in L.dpilqr_last_error(), name
        assert who in L.dpilqr_last_error(), name
    for name in ("X", "U", "K", "bits", "x0s", "W", "u_lim", "Xs", "Us", "J", "sep", "goal"):      # every pointer
        assert _call(lib, d, **{name: P + 4}) == lib.EINVAL and b"aligned" in L.dpilqr_last_error(), name
    assert _call(lib, d, S=0) == lib.EINVAL and b"n_samples=0" in L.dpilqr_last_error()
    assert _call(lib, d, S=-3) == lib.EINVAL
    for k, w in ((65, 1), (64, 2), (128, 3), (129, 2), (256, 5), (200, 0), (1, 0)):
        assert _call(lib, _desc(lib, k), kc_max=1, n_words=w) == lib.EINVAL
        msg = L.dpilqr_last_error().decode()
        assert f"n_words={w}" in msg and f"= {(k + 63) // 64} words" in msg, msg
    assert _call(lib, _desc(lib, 70, 7, 2)) == lib.EINVAL and b"model family" in L.dpilqr_last_error()             # no such family
    for k in (257, 1000):
        assert _call(lib, _desc(lib, k)) == lib.EUNSUPPORTED
        assert f"k={k}" in L.dpilqr_last_error().decode() and "256" in L.dpilqr_last_error().decode()
    assert _call(lib, _desc(lib, 13, 5, 2)) == lib.EUNSUPPORTED and b"BikeDynamics5D" in L.dpilqr_last_error()      # dpilqr_rollout's bike limit
    for kd, kc_max in ((130, 0), (130, -1), (130, 65), (256, 65), (40, 41), (1, 2)):                               # 1 .. min(k, 64)
        assert _call(lib, _desc(lib, kd), kc_max=kc_max) == lib.EUNSUPPORTED and b"kc_max" in L.dpilqr_last_error(), (kd, kc_max)
    # more than 2^31 - 1 workgroups: one sample of 200 agents per workgroup
    assert _call(lib, _desc(lib, 200, B=8), S=(1 << 28) + 1, kc_max=64) == lib.EUNSUPPORTED and b"workgroups" in L.dpilqr_last_error()
    assert _call(lib, _desc(lib, 64, B=8), S=(1 << 30) + 1, kc_max=64) == lib.EUNSUPPORTED and b"workgroups" in L.dpilqr_last_error()
    # an empty batch: nothing to launch, whatever the team's size within the limits
    for k, ns, nc, kc_max in ((256, 4, 2, 64), (129, 12, 4, 3), (65, 3, 2, 64), (64, 6, 3, 64), (12, 5, 2, 12), (1, 3, 2, 1)):
        assert _call(lib, _desc(lib, k, ns, nc, B=0), kc_max=kc_max) == lib.OK, (k, ns, nc)


def _stitch(lib, S=3, k=130, kc_max=2, bits=P, R_=None, G_=None, X=P, Kc=P, U=P, n_words=None, ns=4, nc=2, T=5):
    R = lib.BucketResults() if R_ is None else R_
    G = lib.BucketGains() if G_ is None else G_
    n_words = (k + 63) // 64 if n_words is None else n_words
    return lib.load().dpilqr_dispatch_stitch_policy_wide(S, k, ns, nc, T, kc_max, bits, P, P, P, C.addressof(R), C.addressof(G), X, Kc, U,
                                                         n_words, None)


def test_stitch_entry_argument_checks(lib):
    L = lib.load()
    for k, w in ((0, 1), (-3, 1), (257, 5), (1000, 16)):
        assert _stitch(lib, k=k, n_words=w) == lib.EINVAL
        assert f"k={k}" in L.dpilqr_last_error().decode() and "256" in L.dpilqr_last_error().decode()
    for k, w in ((65, 1), (64, 2), (128, 3), (129, 2), (256, 5), (200, 0)):
        assert _stitch(lib, k=k, n_words=w) == lib.EINVAL
        msg = L.dpilqr_last_error().decode()
        assert f"n_words={w}" in msg and f"= {(k + 63) // 64} words" in msg, msg
    for k, kc_max in ((130, 0), (130, -2), (130, 65), (256, 65), (40, 41), (1, 2)):      # 1 .. min(k, 64)
        assert _stitch(lib, k=k, kc_max=kc_max) == lib.EINVAL and b"kc_max" in L.dpilqr_last_error(), (k, kc_max)
    for bad in (dict(S=-1), dict(bits=None), dict(X=None), dict(Kc=None), dict(U=None), dict(ns=0), dict(nc=0), dict(T=0)):
        assert _stitch(lib, **bad) == lib.EINVAL and b"dispatch_stitch_policy_wide" in L.dpilqr_last_error(), bad
    R = lib.BucketResults()
    R.count[3] = 1; R.X[3] = P; R.U[3] = P
    assert _stitch(lib, kc_max=2, R_=R) == lib.EINVAL and b"sub-problems of 3 agents, kc_max=2" in L.dpilqr_last_error()
    assert _stitch(lib, kc_max=3, R_=R) == lib.EINVAL and b"NULL results of size 3" in L.dpilqr_last_error()      # no gains of that size
    assert _stitch(lib, S=0, kc_max=64, k=256) == lib.OK and _stitch(lib, S=0, kc_max=1, k=1) == lib.OK            # nothing to launch


# ---- the Python layers: every error before the device is touched
def _bare_batch(B=2, T=6, k=70, ns=4, nc=2):
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)      # no device state at all
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = B, T, k, ns, nc, k * ns, k * nc
    return pb


def _alone(B, k):
    return wc.words_of([[[a] for a in range(k)]] * B, k)


def test_policy_rollout_dec_wide_validates_on_the_host():
    k, ns, nc = 70, 4, 2
    pb = _bare_batch(k=k)
    X, U, Kc, x0s = np.zeros((2, 7, k * ns)), np.zeros((2, 6, k * nc)), np.zeros((2, 6, k, nc, 2 * ns)), np.zeros((2, 5, k * ns))
    bits = _alone(2, k)
    bits[0, 3, 1] |= np.uint64(1)       # agent 3 sees agent 64: a member in the second word
    bits[1, 69, 0] |= np.uint64(1) << np.uint64(63)
    b64 = pb._checked_masks_wide("policy_rollout_dec_wide", bits, 2)
    assert b64.dtype == np.int64 and b64.shape == (2, k, 2) and np.array_equal(b64.view(np.uint64), bits) and (b64 < 0).any()
    assert np.array_equal(pb._checked_masks_wide("w", bits.view(np.int64), 2), b64)      # negative int64 words are words
    three = bits.copy(); three[0, 3, 1] |= np.uint64(2)
    past = bits.copy(); past[1, 2, 1] |= np.uint64(1) << np.uint64(6)      # agent 70 of a team of 70
    lacking = bits.copy(); lacking[1, 65, 1] = np.uint64(1)                # agent 65 with agent 64's bit instead of its own
    bad = [dict(X=X[:, :6]), dict(U_ff=U[:, :, :5]), dict(Kc=np.zeros((2, 6, k * nc, k * ns))), dict(Kc=np.zeros((2, 6, k, nc, 7))),
           dict(Kc=np.zeros((2, 6, k, nc, 65 * ns))), dict(Kc=np.zeros((2, 6, k, nc, 0))), dict(nbr_bits=bits[:, :, 0]),
           dict(nbr_bits=bits[:, :, :1]), dict(nbr_bits=bits.astype(np.float64)), dict(x0s=np.zeros((2, k * ns))),
           dict(x0s=np.zeros((2, 0, k * ns))), dict(W=np.zeros((2, 5, 7, k * ns))), dict(u_lim=np.zeros((k * nc, 2))),
           dict(u_lim=np.array([[1.0] * (k * nc), [-1.0] * (k * nc)])), dict(nbr_bits=three), dict(nbr_bits=past), dict(nbr_bits=lacking)]
    for kw in bad:
        a = dict(X=X, U_ff=U, Kc=Kc, nbr_bits=bits, x0s=x0s, W=None, u_lim=None); a.update(kw)
        with pytest.raises(ValueError, match="policy_rollout_dec_wide"):
            pb.policy_rollout_dec_wide(a["X"], a["U_ff"], a["Kc"], a["nbr_bits"], a["x0s"], W=a["W"], u_lim=a["u_lim"])
    with pytest.raises(ValueError, match="3 members, Kc holds kc_max = 2"):
        pb.policy_rollout_dec_wide(X, U, Kc, three, x0s)
    with pytest.raises(ValueError, match="at or past agent k = 70"):
        pb.policy_rollout_dec_wide(X, U, Kc, past, x0s)
    with pytest.raises(ValueError, match="own bit"):
        pb.policy_rollout_dec_wide(X, U, Kc, lacking, x0s)
    with pytest.raises(ValueError, match="1 <= kc_max <= 64"):
        pb.policy_rollout_dec_wide(X, U, np.zeros((2, 6, k, nc, 65 * ns)), bits, x0s)


def test_257_agents_and_13_bikes_are_refused():
    pb = _bare_batch(k=257)
    with pytest.raises(ValueError, match="policy_rollout_dec_wide serves teams of up to 256 agents.*k = 257"):
        pb.policy_rollout_dec_wide(np.zeros((2, 7, 1028)), np.zeros((2, 6, 514)), np.zeros((2, 6, 257, 2, 4)), np.ones((2, 257, 5), dtype=np.int64),
                                   np.zeros((2, 5, 1028)))
    pb = _bare_batch(k=13, ns=5, nc=2)
    with pytest.raises(ValueError, match="policy_rollout_dec_wide.*five-state.*k = 13"):
        pb.policy_rollout_dec_wide(np.zeros((2, 7, 65)), np.zeros((2, 6, 26)), np.zeros((2, 6, 13, 2, 5)), np.ones((2, 13, 1), dtype=np.int64),
                                   np.zeros((2, 5, 65)))


def _problem(k):
    import dpilqr_amd as dp
    ids = [100 + i for i in range(k)]
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1, i) for i in ids])
    refs = [dp.ReferenceCost(np.zeros(4), np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), i) for i in ids]
    return dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([4] * k, 0.5, [2] * k)))


class _StubBatch:
    def __init__(self):
        self.calls = []

    def policy_rollout_dec_wide(self, *a, **kw):
        self.calls.append(("policy_rollout_dec_wide", a, kw))
        return "wide"


def test_python_refusals_come_before_any_device_work(lib):
    from dpilqr_amd.dispatch import DistributedPolicy, ScenarioFrontEnd, solve_scenarios_distributed
    p65, T = _problem(65), 4
    X, U = np.zeros((2, 1, 65 * 4)), np.zeros((2, T, 65 * 2))
    # today's text, word for word
    with pytest.raises(ValueError, match=r"^solve_scenarios_distributed: policy=True is not built for teams of more than 64 agents \(this one has 65\)$"):
        solve_scenarios_distributed(p65, X, U, 0.5, policy=True)
    with pytest.raises(ValueError, match=r"^solve_scenarios_distributed: shard= is not built for teams of more than 64 agents \(this one has 65\)$"):
        solve_scenarios_distributed(p65, X, U, 0.5, shard=(0, 2))
    with pytest.raises(ValueError, match="serves neither shard= nor ignore_ids"):
        solve_scenarios_distributed(p65, X, U, 0.5, policy="wide", shard=(0, 2))
    with pytest.raises(ValueError, match="serves neither shard= nor ignore_ids"):
        solve_scenarios_distributed(_problem(5), np.zeros((2, 1, 20)), np.zeros((2, T, 10)), 0.5, policy="wide", shard=(0, 2))
    with pytest.raises(ValueError, match="serves neither shard= nor ignore_ids"):
        solve_scenarios_distributed(p65, X, U, 0.5, policy="wide", ignore_ids=[100])
    with pytest.raises(ValueError, match="expected False, True or 'wide'"):
        solve_scenarios_distributed(p65, X, U, 0.5, policy="narrow")
    with pytest.raises(ValueError, match="at most 256 agents per problem, this one has 257"):
        solve_scenarios_distributed(_problem(257), np.zeros((1, 1, 257 * 4)), np.zeros((1, T, 257 * 2)), 0.5, policy="wide")
    # a wide policy: rollout goes to policy_rollout_dec_wide whatever the size, advance is not built
    for k in (5, 64, 65, 256):
        nw = (k + 63) // 64
        bits = np.ones((2, k, nw), dtype=np.int64)
        pol = DistributedPolicy(dict(k=k), None, np.zeros((2, T + 1, 4 * k)), np.zeros((2, T, 2 * k)), np.zeros((2, T, k, 2, 4)), bits, 1, wide=True)
        stub = pol._batch = _StubBatch()
        assert pol.rollout(np.zeros((2, 3, 4 * k))) == "wide" and pol.rollout(np.zeros((2, 3, 4 * k)), trajectories=True) == "wide"
        assert stub.calls[0][1][3] is bits and stub.calls[0][2]["masks_checked"] is None and stub.calls[1][2]["masks_checked"] is bits
        with pytest.raises(ValueError, match="the wide advance is not built"):
            pol.advance(1, {})
    # stitch_policy keeps its refusal; stitch_policy_wide asks for a front end on the wide entries
    fe = ScenarioFrontEnd.__new__(ScenarioFrontEnd)      # no device state
    fe.k, fe.wide = 65, True
    with pytest.raises(ValueError, match="stitch_policy is not built for teams of more than 64 agents"):
        fe.stitch_policy({}, {}, None)
    fe.k, fe.wide = 24, False
    with pytest.raises(ValueError, match="stitch_policy_wide needs a front end on the wide entries"):
        fe.stitch_policy_wide({}, {}, None)
    assert lib.load().dpilqr_abi_version() == 4


def test_the_pinned_tables_are_untouched():
    from dpilqr_amd import _lib
    from dpilqr_amd.batch import ROUTES, ProblemBatch
    assert "policy_rollout_dec_wide" not in ProblemBatch.CLOSED_LOOP and len(ProblemBatch.CLOSED_LOOP) == 8 and sorted(ROUTES) == ["large", "small", "team"]
    assert not any("wide" in n for n in _lib.EXT_SIGNATURES) and len(_lib.SWARM_SIGNATURES) == 4


# ---- the kernels in the built library
@pytest.fixture(scope="module")
def table(lib):
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("ns,nc", FAMILIES)
def test_wide_kernels_keep_every_register(table, ns, nc):
    r = table[wc.kernel_name(f"k_policy_rollout_dec_wide<{ns}, {nc}>")]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256, r
    # static LDS: 256 (ns | 1) + 256 * 3 + 256 doubles and 256 ints (and the compiler's padding between them), under 64 KB
    assert 8 * 256 * ((ns | 1) + 4) + 4 * 256 <= r["group_segment_fixed_size"] < 64 * 1024, r


def test_the_stitch_kernel_and_no_further_wide_kernel(table):
    r = next(v for n, v in table.items() if n.endswith("k_stitch_policy_wide"))
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    # one kernel text, two word counts: the five four-word instantiations beside the five one-word ones, and nothing else
    names = sorted(n for n in table if "k_policy_rollout_dec_team" in n or "k_policy_rollout_dec_wide" in n)
    assert names == sorted(wc.kernel_name(f"k_policy_rollout_dec_{width}<{ns}, {nc}>") for width in ("team", "wide") for ns, nc in FAMILIES)


def test_the_team_kernels_keep_their_figures(table):
    """The one-word instantiations of the shared kernel text: registers and LDS are what the team kernel's were
    (profiles/policy_dec_team_checks.txt)."""
    r = table[wc.kernel_name("k_policy_rollout_dec_team<12, 4>")]
    assert (r["vgpr_count"], r["agpr_count"], r["group_segment_fixed_size"]) == (352, 96, 35328), r
    r = table[wc.kernel_name("k_policy_rollout_dec_team<4, 2>")]
    assert (r["vgpr_count"], r["agpr_count"], r["group_segment_fixed_size"]) == (179, 0, 18944), r
