"""The team receding-horizon advance's host side, without a GPU: the symbol is declared, bound and exported; the argument
checks of dpilqr_policy_advance_dec_team answer before any launch (fake, aligned device pointers, never dereferenced);
ProblemBatch.policy_advance_dec_team validates on the host; DistributedPolicy.advance and solve_rhc_closed_loop route by size
and by `team=` (stub batches, tensors on the host); the refusals that are pinned for the default arguments stay; the built
kernels keep their registers; and the cases of tests/policy_dec_team_cases.py are honest on the prefixes the GPU tests execute."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import policy_advance_dec_team_cases as atc
from tests import policy_cases as pc
from tests import policy_dec_team_cases as tc
from tests.policy_dec_wide_cases import kernel_name

ROOT = Path(__file__).resolve().parent.parent
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test
NAME = "dpilqr_policy_advance_dec_team"
FAMILIES = ((3, 2), (4, 2), (5, 2), (6, 3), (12, 4))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


# ---- the C ABI
def _desc(lib, k, ns=4, nc=2, B=2, T=10):
    return lib.BatchDesc(B, k, ns, nc, T, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)


_DEFAULT = dict(X=P, U=P, K=P, kc_max=1, bits=P, h=1, scen=None, n_scen=4, L=5, n_d=2, W=None, u_lim=None, x_cur=P, n_done=P, X_exec=P,
                U_exec=P, J_exec=P, min_sep=P, dist_left=P, U_next=P, X_next=P)
_REQUIRED = ("X", "U", "x_cur", "n_done", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left", "U_next", "X_next")


def _call(lib, d, **kw):
    a = dict(_DEFAULT); a.update(kw)
    return lib.load().dpilqr_policy_advance_dec_team(C.byref(d), a["X"], a["U"], a["K"], a["kc_max"], a["bits"], a["h"], a["scen"], a["n_scen"],
                                                     a["L"], a["n_d"], a["W"], a["u_lim"], a["x_cur"], a["n_done"], a["X_exec"], a["U_exec"],
                                                     a["J_exec"], a["min_sep"], a["dist_left"], a["U_next"], a["X_next"], None)


def test_symbol_is_declared_bound_and_exported(lib):
    ext = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dpilqr_policy.h").read_text(), flags=re.S)
    assert re.search(rf"\bint32_t\s+{NAME}\s*\(", ext)
    assert NAME in lib.EXT_SIGNATURES and NAME not in lib.SIGNATURES
    fn = getattr(lib.load(), NAME)
    assert fn.argtypes == lib.EXT_SIGNATURES[NAME][1] and fn.restype is C.c_int32 and len(fn.argtypes) == 23
    args = lambda n: [a.strip() for a in re.search(rf"\b{n}\s*\((.*?)\)\s*;", ext, re.S).group(1).split(",")]
    assert args(NAME) == args("dpilqr_policy_advance_dec")                      # the argument list is identical
    assert lib.EXT_SIGNATURES[NAME] == lib.EXT_SIGNATURES["dpilqr_policy_advance_dec"]
    assert sorted(set(re.findall(r"\b(dpilqr_[a-z_0-9]+)\s*\(", ext))) == sorted(lib.EXT_SIGNATURES)
    assert lib.load().dpilqr_abi_version() == 4      # additive: the ABI version stays


def test_bad_arguments_are_einval(lib):
    L = lib.load()
    d = _desc(lib, 64)                # T = 10, B = 2
    assert L.dpilqr_policy_advance_dec_team(None, P, P, P, 1, P, 1, None, 4, 5, 2, None, None, P, P, P, P, P, P, P, P, P, None) == lib.EINVAL
    for name in _REQUIRED:
        assert _call(lib, d, **{name: None}) == lib.EINVAL, name
        assert b"NULL" in L.dpilqr_last_error() and b"policy_advance_dec_team" in L.dpilqr_last_error(), name
    for kw in (dict(h=0), dict(h=11), dict(h=-1), dict(L=0), dict(n_d=0), dict(n_d=5), dict(n_scen=1)):
        assert _call(lib, d, **kw) == lib.EINVAL, kw
        assert (next(iter(kw)) + "=").encode() in L.dpilqr_last_error(), (kw, L.dpilqr_last_error())
    for name in tuple(f for f in _REQUIRED if f != "n_done") + ("K", "W", "u_lim", "bits"):      # the alignment rule of the sibling entries
        assert _call(lib, d, **{name: P + 4}) == lib.EINVAL, name
        assert b"aligned" in L.dpilqr_last_error(), name
    assert _call(lib, d, scen=P + 2) == lib.EINVAL and _call(lib, d, n_done=P + 2) == lib.EINVAL      # int32 words
    assert _call(lib, d, bits=None) == lib.EINVAL and b"nbr_bits" in L.dpilqr_last_error()              # gains without masks
    assert _call(lib, _desc(lib, 30, 7, 2)) == lib.EINVAL and b"model family" in L.dpilqr_last_error()   # no such family
    bad = lib.BatchDesc(2, 5, 4, 2, 10, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P + 4, 0, P, 0, P, 0, P, 0, P, 0)      # a misaligned xf
    assert _call(lib, bad) == lib.EINVAL


def test_beyond_the_limits_is_unsupported_before_any_launch(lib):
    """With the fake pointers of this file a launch would not come back with these answers."""
    L = lib.load()
    assert _call(lib, _desc(lib, 65)) == lib.EUNSUPPORTED and b"k=65" in L.dpilqr_last_error()
    assert _call(lib, _desc(lib, 13, 5, 2)) == lib.EUNSUPPORTED and b"BikeDynamics5D" in L.dpilqr_last_error()      # dpilqr_rollout's bike limit
    for k, kc_max in ((64, 0), (64, -1), (64, 65), (21, 22)):
        assert _call(lib, _desc(lib, k), kc_max=kc_max) == lib.EUNSUPPORTED, (k, kc_max)
        assert b"kc_max" in L.dpilqr_last_error() and b"policy_advance_dec_team" in L.dpilqr_last_error()
    assert _call(lib, _desc(lib, 64), K=None, bits=None, kc_max=0) == lib.EUNSUPPORTED      # open loop or not: kc_max is 1 .. k


def test_an_empty_batch_launches_nothing(lib):
    """B = 0 is DPILQR_OK, whatever the team's size within the limits."""
    for k, ns, nc in ((64, 4, 2), (21, 12, 4), (33, 4, 2), (12, 5, 2), (1, 3, 2)):
        assert _call(lib, _desc(lib, k, ns, nc, B=0), kc_max=k, n_scen=0) == lib.OK, (k, ns, nc)
        assert _call(lib, _desc(lib, k, ns, nc, B=0), K=None, bits=None) == lib.OK      # open loop: no gains, no masks


# ---- the Python wrapper: every error before the device is touched
def _bare_batch(B=2, T=6, k=3, ns=4, nc=2):
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)      # no device state at all
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = B, T, k, ns, nc, k * ns, k * nc
    return pb


def _host_state(S=4, L=5, T=6, k=3, n=12, m=6, **over):
    import torch
    f64 = torch.float64
    st = dict(x_cur=torch.zeros((S, n), dtype=f64), n_done=torch.zeros((S,), dtype=torch.int32), X_exec=torch.zeros((S, L + 1, n), dtype=f64),
              U_exec=torch.zeros((S, L, m), dtype=f64), J_exec=torch.zeros((S,), dtype=f64), min_sep=torch.zeros((S,), dtype=f64),
              dist_left=torch.zeros((S, k), dtype=f64), U_next=torch.zeros((S, T, m), dtype=f64), X_next=torch.zeros((S, T + 1, n), dtype=f64))
    st.update(over)
    return st


def test_policy_advance_dec_team_validates_on_the_host():
    import torch
    k, ns, nc, T = 21, 4, 2, 6
    n, m = k * ns, k * nc
    pb = _bare_batch(k=k, ns=ns, nc=nc, T=T)
    X, U, Kc = np.zeros((2, T + 1, n)), np.zeros((2, T, m)), np.zeros((2, T, k, nc, 2 * ns))
    own = (np.uint64(1) << np.arange(k, dtype=np.uint64))[None].repeat(2, axis=0)
    st = lambda **kw: _host_state(T=T, k=k, n=n, m=m, **kw)
    ok = dict(X=X, U_ff=U, Kc=Kc, nbr_bits=own, h=2, state=st(), scen=None, W=None, u_lim=None, n_d=2)
    bad = [dict(X=X[:, :T]), dict(U_ff=U[:, :, :5]), dict(Kc=np.zeros((2, T, m, n))), dict(Kc=np.zeros((2, T, k, nc, 2 * ns + 1))),
           dict(Kc=np.zeros((2, T, k, nc, (k + 1) * ns))), dict(Kc=np.zeros((2, T, k, nc, 0))), dict(nbr_bits=own[:, :2]),
           dict(nbr_bits=own.astype(np.float64)), dict(nbr_bits=None), dict(h=0), dict(h=T + 1), dict(h=1.5), dict(n_d=0), dict(n_d=5),
           dict(scen=[0]), dict(scen=[0, 4]), dict(scen=[1, 1]), dict(W=np.zeros((4, 6, n))), dict(u_lim=np.zeros((m, 2))),
           dict(u_lim=np.array([[1.0] * m, [-1.0] * m])), dict(state={}), dict(state=st(S=1)),
           dict(state=st(n_done=torch.zeros((4,), dtype=torch.int64))),
           dict(nbr_bits=own ^ np.uint64(1)),                            # agent 0 lacks its own bit (and agent j > 0 sees agent 0: two members)
           dict(nbr_bits=own | np.uint64(7))]                            # up to four members, kc_max = 2
    for kw in bad:
        a = dict(ok); a.update(kw)
        with pytest.raises(ValueError, match="policy_advance_dec_team"):
            pb.policy_advance_dec_team(a["X"], a["U_ff"], a["Kc"], a["nbr_bits"], a["h"], a["state"], scen=a["scen"], W=a["W"], u_lim=a["u_lim"],
                                       n_d=a["n_d"])
    with pytest.raises(ValueError, match="policy_advance_dec_team: a neighbourhood mask lacks its agent's own bit"):
        pb.policy_advance_dec_team(X, U, Kc, own ^ np.uint64(1), 1, st())
    with pytest.raises(ValueError, match="policy_advance_dec_team: a neighbourhood mask has 4 members"):
        pb.policy_advance_dec_team(X, U, Kc, own | np.uint64(7), 1, st())
    with pytest.raises(ValueError, match="policy_advance_dec_team: h = 9"):
        pb.policy_advance_dec_team(X, U, None, None, 9, st())
    # the shared checks accept what the team entry serves: the size rule is the third one of _advance_shapes
    assert pb._advance_shapes("policy_advance_dec_team", X, 2, st(), [3, 1], np.zeros((4, 5, n)), None, 2, (("U_ff", U, (2, T, m)),), team=True) == (4, 5)
    with pytest.raises(ValueError, match="policy_advance_dec serves clusters up to n_x = 60 and k = 20"):
        pb._advance_shapes("policy_advance_dec", X, 2, st(), None, None, None, 2, (("U_ff", U, (2, T, m)),))


def test_65_agents_and_13_bikes_are_refused():
    pb = _bare_batch(k=65)
    with pytest.raises(ValueError, match="policy_advance_dec_team serves teams of up to 64 agents.*k = 65"):
        pb.policy_advance_dec_team(np.zeros((2, 7, 260)), np.zeros((2, 6, 130)), np.zeros((2, 6, 65, 2, 4)), np.ones((2, 65), dtype=np.int64), 1, {})
    with pytest.raises(ValueError, match="policy_advance_dec_team serves teams of up to 64 agents.*k = 65"):
        pb.policy_advance_dec_team(np.zeros((2, 7, 260)), np.zeros((2, 6, 130)), None, None, 1, {})
    pb = _bare_batch(k=13, ns=5, nc=2)
    with pytest.raises(ValueError, match="policy_advance_dec_team.*five-state.*k = 13"):
        pb.policy_advance_dec_team(np.zeros((2, 7, 65)), np.zeros((2, 6, 26)), np.zeros((2, 6, 13, 2, 5)), np.ones((2, 13), dtype=np.int64), 1, {})


# ---- DistributedPolicy.advance routes by size and by team=
class _StubBatch:
    def __init__(self):
        self.calls = []

    def policy_advance_dec(self, *a, **kw):
        self.calls.append(("policy_advance_dec", a, kw))
        return "dec"

    def policy_advance_dec_team(self, *a, **kw):
        self.calls.append(("policy_advance_dec_team", a, kw))
        return "team"


@pytest.mark.parametrize("k,ns,team,want", [(20, 3, True, "policy_advance_dec"), (15, 4, True, "policy_advance_dec"), (3, 4, True, "policy_advance_dec"),
                                            (21, 3, True, "policy_advance_dec_team"), (16, 4, True, "policy_advance_dec_team"),
                                            (64, 4, True, "policy_advance_dec_team"), (6, 12, True, "policy_advance_dec_team"),
                                            (24, 4, False, "policy_advance_dec"), (64, 4, False, "policy_advance_dec"), (3, 4, False, "policy_advance_dec")])
def test_distributed_policy_advance_routes_by_size_and_team(k, ns, team, want):
    from dpilqr_amd.dispatch import DistributedPolicy
    nc, T, S = 2, 4, 2
    X_dec, U_ff, Kc, bits = np.zeros((S, T + 1, k * ns)), np.zeros((S, T, k * nc)), np.zeros((S, T, k, nc, ns)), np.ones((S, k), dtype=np.int64)
    pol = DistributedPolicy(dict(k=k), None, X_dec, U_ff, Kc, bits, 1)
    stub = pol._batch = _StubBatch()
    state, scen, W, lim = {}, [1, 0], np.zeros((S, 5, k * ns)), np.zeros((2, k * nc))
    kw = dict(team=True) if team else {}
    assert pol.advance(2, state, scen=scen, W=W, u_lim=lim, n_d=3, **kw) == ("dec" if want == "policy_advance_dec" else "team")
    pol.advance(1, state, **kw)
    assert [c[0] for c in stub.calls] == [want, want]
    name, a, got = stub.calls[0]
    assert a[0] is X_dec and a[1] is U_ff and a[2] is Kc and a[3] is bits and a[4] == 2 and a[5] is state
    assert got["scen"] is scen and got["W"] is W and got["u_lim"] is lim and got["n_d"] == 3 and got["masks_checked"] is None
    assert stub.calls[1][2]["masks_checked"] is bits and "team" not in got      # the masks are checked by the first call only


# ---- solve_rhc_closed_loop routes by size and by team=: the device replaced by the host, the batch and the solve by stubs
def _problem(k):
    import dpilqr_amd as dp
    dp._reset_ids()
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(np.zeros(4), np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k)))


@pytest.fixture
def stubbed_loop(monkeypatch):
    import torch
    import dpilqr_amd.batch as batch_mod
    import dpilqr_amd.device as device_mod
    import dpilqr_amd.dispatch as dispatch_mod
    import dpilqr_amd.distributed as dist_mod
    calls = []

    class StubPB:
        advance_state = batch_mod.ProblemBatch.advance_state

        def __init__(self, model, n_dims, xf, Q, R, Qf, radius, dt, T, w_ref=1.0, w_prox=1.0, B=None, hints=None):
            self.T, self.B = T, B
            self.k, self.n_s, self.n_c = hints[:3]
            self.n_x, self.n_u = self.k * self.n_s, self.k * self.n_c

        def _advance(self, name, X, U, Kc, bits, h, state, scen=None, **kw):
            calls.append((name, Kc, bits, h, kw))
            state["n_done"][scen.long()] += h
            return state

        def policy_advance_dec(self, *a, **kw):
            return self._advance("policy_advance_dec", *a, **kw)

        def policy_advance_dec_team(self, *a, **kw):
            return self._advance("policy_advance_dec_team", *a, **kw)

        def cost(self, x, u, terminal=False):
            return torch.zeros((x.shape[0], x.shape[1]), dtype=torch.float64)

    class StubPolicy:
        def __init__(self, pb):
            self.pb = pb

        def advance(self, h, state, scen=None, team=False, **kw):
            calls.append(("DistributedPolicy.advance", team, h))
            state["n_done"][scen.long()] += h
            return state

    def solve_stub(problem, X, U, radius, xf=None, policy=False, **kw):
        S, T, m = U.shape
        n = X.shape[2]
        calls.append(("solve_scenarios_distributed", policy))
        return torch.zeros((S, T + 1, n), dtype=torch.float64), U.clone(), torch.ones((S,), dtype=torch.float64), dict(policy=StubPolicy(None) if policy else None)

    def constants_stub(d, kc=None):
        return dict(model=d["model"], n_dims=d["n_dims"], Q=d["Q"], R=d["R"], Qf=d["Qf"], word=0)

    monkeypatch.setattr(device_mod, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(batch_mod, "ProblemBatch", StubPB)
    monkeypatch.setattr(dispatch_mod, "device_constants", constants_stub)
    monkeypatch.setattr(dist_mod, "solve_scenarios_distributed", solve_stub)
    return calls


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("k,team,want", [(16, True, "team"), (24, True, "team"), (64, True, "team"), (3, True, "dec"), (15, True, "dec"), (3, False, "dec")])
def test_the_loop_routes_by_size_and_team(stubbed_loop, k, team, want, feedback):
    import dpilqr_amd as dp
    calls = stubbed_loop
    out = dp.solve_rhc_closed_loop(_problem(k), np.ones((2, 4 * k)), 6, radius=1.0, centralized=False, feedback=feedback, step_size=2,
                                   dist_converge=1e-3, max_steps=4, **(dict(team=True) if team else {}))
    assert (out["n_rounds"] == 2).all() and not out["converged"].any()
    solves = [c for c in calls if c[0] == "solve_scenarios_distributed"]
    advances = [c for c in calls if c[0] != "solve_scenarios_distributed"]
    assert len(solves) == 2 and all(c[1] is feedback for c in solves) and len(advances) == 2      # one launch of the advance per round
    if feedback:
        assert advances == [("DistributedPolicy.advance", want == "team", 2)] * 2
    else:
        assert [c[0] for c in advances] == ["policy_advance_dec_team" if want == "team" else "policy_advance_dec"] * 2
        assert all(c[1] is None and c[2] is None and c[3] == 2 for c in advances)      # the stitched plan, open loop


def test_the_loop_refuses_what_the_team_route_does_not_serve(stubbed_loop):
    import dpilqr_amd as dp
    kw = dict(dist_converge=0.1, max_steps=4)
    with pytest.raises(ValueError, match=r"team=True is the distributed loop \(centralized=False\)"):
        dp.solve_rhc_closed_loop(_problem(16), np.zeros((2, 64)), 10, radius=1.0, team=True, **kw)
    with pytest.raises(ValueError, match=r"team=True is the distributed loop \(centralized=False\)"):
        dp.solve_rhc_closed_loop(_problem(3), np.zeros((2, 12)), 10, radius=1.0, team=True, centralized=True, **kw)
    with pytest.raises(ValueError, match=r"solve_rhc_closed_loop is not built for teams of more than 64 agents \(this one has 65\)"):
        dp.solve_rhc_closed_loop(_problem(65), np.zeros((2, 260)), 10, radius=1.0, team=True, centralized=False, **kw)
    with pytest.raises(ValueError, match="radius"):
        dp.solve_rhc_closed_loop(_problem(16), np.zeros((2, 64)), 10, team=True, centralized=False, **kw)
    assert not stubbed_loop      # nothing was solved or launched


# ---- what stays exactly as it is with default arguments
def test_the_pinned_refusals_still_raise(lib):
    import dpilqr_amd as dp
    from dpilqr_amd.dispatch import DistributedPolicy
    for k, ns in ((16, 4), (20, 4), (21, 3)):
        pb = _bare_batch(k=k, ns=ns)
        n, m = pb.n_x, pb.n_u
        with pytest.raises(ValueError, match="policy_advance_dec serves clusters up to n_x = 60 and k = 20"):
            pb.policy_advance_dec(np.zeros((2, 7, n)), np.zeros((2, 6, m)), np.zeros((2, 6, k, 2, ns)), np.ones((2, k), dtype=np.int64), 1, {})
    k = 24
    pol = DistributedPolicy(dict(k=k), None, np.zeros((2, 7, 4 * k)), np.zeros((2, 6, 2 * k)), np.zeros((2, 6, k, 2, 4)), np.ones((2, k), dtype=np.int64), 1)
    pol._batch = _bare_batch(k=k)
    with pytest.raises(ValueError, match="policy_advance_dec serves clusters up to n_x = 60"):
        pol.advance(1, {})
    big = _problem(16)
    with pytest.raises(ValueError, match="n_x = 60.*large=True"):
        dp.solve_rhc_closed_loop(big, np.zeros((2, 64)), 10, dist_converge=0.1, max_steps=4)
    with pytest.raises(ValueError, match="n_x = 60.*large=True"):
        dp.solve_rhc_closed_loop(big, np.zeros((2, 64)), 10, radius=1.0, dist_converge=0.1, max_steps=4, centralized=False)
    with pytest.raises(ValueError, match="large=True.*distributed loop.*not built"):
        dp.solve_rhc_closed_loop(big, np.zeros((2, 64)), 10, radius=1.0, dist_converge=0.1, max_steps=4, centralized=False, large=True)
    assert lib.load().dpilqr_abi_version() == 4


# ---- the kernels in the built library
@pytest.fixture(scope="module")
def table(lib):
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("ns,nc", FAMILIES)
def test_team_advance_kernels_keep_every_register(table, ns, nc):
    r = table[kernel_name(f"k_policy_advance_dec_team<{ns}, {nc}>")]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256, r
    # static LDS: 256 (ns | 1) + 256 * 3 + 3 * 256 doubles and 3 * 256 ints (and the compiler's padding between them), under 64 KB
    assert 8 * 256 * ((ns | 1) + 6) + 4 * 3 * 256 <= r["group_segment_fixed_size"] < 64 * 1024, r


def test_no_further_team_advance_kernel_was_built(table):
    """One kernel text, two word counts: the five one-word instantiations, the five four-word ones, and nothing else."""
    names = sorted(n for n in table if "k_policy_advance_dec_team" in n or "k_policy_advance_dec_wide" in n)
    assert names == sorted(kernel_name(f"k_policy_advance_dec_{width}<{ns}, {nc}>") for width in ("team", "wide") for ns, nc in FAMILIES)


# ---- the cases, on the prefixes the GPU tests execute: from the reference alone
@pytest.mark.parametrize("case", atc.CASES, ids=atc.IDS)
def test_the_cases_are_honest_on_a_prefix(case):
    ref = tc.case_ref(case)
    f3, f1 = atc.prefix_figures(case, ref, 3), atc.prefix_figures(case, ref, 1)
    print(case.id, "h=3", f3, "h=1", f1)
    assert 0.0 < f3["clamped"] < 1.0 and 0.0 < f1["clamped"] < 1.0, (f3, f1)      # the limits clamp some entries within the prefix, not all
    assert f3["near"] > 0.0, f3                                                  # W brings a share of the samples inside the radius
    assert all(u <= pc.MAX_UNCHECKED for u in f3["unchecked"].values()), f3      # within the cap the GPU test holds


def test_the_case_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    shape = {c.id: (c.k, 256 // c.k, pc.B * c.S) for c in atc.CASES}
    assert shape["team-dint4_uni4-k21-S13"] == (21, 12, 39) and shape["team-dint4-k33-S8"] == (33, 7, 24) and shape["team-dint4-k64-S5"] == (64, 4, 15)
    assert all(n % ipw for _, ipw, n in shape.values())                        # a last workgroup that is partly full, in every case
    assert sum(n > ipw for _, ipw, n in shape.values()) >= 4                   # more than one workgroup in four of them, k = 33 and 64 included
    assert {(c.ns, c.nc) for c in atc.CASES} == {(3, 2), (4, 2), (6, 3), (12, 4)}
    assert [c.id for c in atc.CROSS] == ["dec-dint4_uni4-k5-S53", "dec-quad6_human6-k3-S6"] and len(set(atc.CROSS[1].n_dims)) == 2


def test_the_loops_scenarios_have_the_cluster_sizes_they_are_placed_for():
    """On the CPU, with the package's own NumPy graph function."""
    from dpilqr_amd.distributed import define_inter_graph_threshold
    x0, xf = atc.placement()
    sizes = [[len(v) for v in define_inter_graph_threshold(x0[s][None], atc.RADIUS, [atc.NS] * atc.K_AG, list(range(atc.K_AG))).values()]
             for s in range(atc.S_LOOP)]
    assert sizes == atc.SIZES
    assert atc.K_AG * atc.NS == 96 and len({kc for row in sizes for kc in row}) >= 4      # beyond n_x = 60; several cluster sizes
    assert atc.L_LOOP // atc.H_LOOP == 2 and atc.N_LOOP == pc.T
