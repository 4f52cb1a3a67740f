"""The receding-horizon advance for teams of up to 256 agents, the host side, without a GPU: the two entries of
include/dpilqr_swarm_advance.h (declared, bound, exported; every refusal before any launch, with fake, aligned device pointers
that are never dereferenced), the Python layers' refusals before any device work, the pinned tables, the new kernels' resources
in the built library beside the figures the team advance and the wide rollout keep, the conditions that keep the cases of
tests/policy_advance_dec_wide_cases.py honest on the prefixes the GPU tests execute (from the CPU reference alone), and the
kernel's member walk in NumPy."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import policy_advance_dec_wide_cases as awc
from tests import policy_cases as pc
from tests import policy_dec_wide_cases as wc

ROOT = Path(__file__).resolve().parent.parent
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test
ADVANCE, COST = "dpilqr_policy_advance_dec_wide", "dpilqr_cost_eval_wide"
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
                U_exec=P, J_exec=P, min_sep=P, dist_left=P, U_next=P, X_next=P, n_words=None)
_REQUIRED = ("X", "U", "x_cur", "n_done", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left", "U_next", "X_next")


def _call(lib, d, **kw):
    a = dict(_DEFAULT); a.update(kw)
    n_words = (d.k + 63) // 64 if a["n_words"] is None else a["n_words"]
    return lib.load().dpilqr_policy_advance_dec_wide(C.byref(d), a["X"], a["U"], a["K"], a["kc_max"], a["bits"], a["h"], a["scen"], a["n_scen"],
                                                     a["L"], a["n_d"], a["W"], a["u_lim"], a["x_cur"], a["n_done"], a["X_exec"], a["U_exec"],
                                                     a["J_exec"], a["min_sep"], a["dist_left"], a["U_next"], a["X_next"], n_words, None)


def test_symbols_are_declared_bound_and_exported(lib):
    """Fails on a build without the feature: there is no include/dpilqr_swarm_advance.h, no binding and no symbol."""
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    core, ext = strip((ROOT / "include" / "dpilqr_hip.h").read_text()), strip((ROOT / "include" / "dpilqr_swarm_advance.h").read_text())
    lines = [l.strip() for l in core.splitlines()]
    assert lines.index('#include "dpilqr_swarm_advance.h"') == lines.index('#include "dpilqr_swarm_policy.h"') + 1
    decl = dict(re.findall(r"\bint32_t\s+(dpilqr_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", ext))
    assert sorted(decl) == sorted([ADVANCE, COST]) == sorted(lib.SWARM_ADVANCE_SIGNATURES)
    older = set(lib.SIGNATURES) | set(lib.EXT_SIGNATURES) | set(lib.SWARM_SIGNATURES) | set(lib.SWARM_POLICY_SIGNATURES) | set(lib.ORDER_SIGNATURES)
    assert not set(lib.SWARM_ADVANCE_SIGNATURES) & older
    for name, n_args in ((ADVANCE, 24), (COST, 7)):
        assert len(decl[name].split(",")) == n_args == len(lib.SWARM_ADVANCE_SIGNATURES[name][1]), name
        fn = getattr(lib.load(), name)
        assert fn.argtypes == lib.SWARM_ADVANCE_SIGNATURES[name][1] and fn.restype is C.c_int32
    args = lambda text, n: [" ".join(a.split()) for a in re.search(rf"\b{n}\s*\((.*?)\)\s*;", text, re.S).group(1).split(",")]
    # the advance: the team entry's arguments plus n_words before the stream
    team = args(strip((ROOT / "include" / "dpilqr_policy.h").read_text()), "dpilqr_policy_advance_dec_team")
    assert args(ext, ADVANCE) == team[:-1] + ["int32_t n_words", "void* stream"]
    assert lib.SWARM_ADVANCE_SIGNATURES[ADVANCE][1] == lib.EXT_SIGNATURES["dpilqr_policy_advance_dec_team"][1][:-1] + [C.c_int32, C.c_void_p]
    # the cost: dpilqr_cost_eval's arguments
    assert args(ext, COST) == args(core, "dpilqr_cost_eval")
    assert lib.SWARM_ADVANCE_SIGNATURES[COST][1] == lib.SIGNATURES["dpilqr_cost_eval"][1]
    assert lib.load().dpilqr_abi_version() == 4 and lib.ABI_VERSION == 4      # additive: the ABI version stays


def test_the_header_compiles_as_c(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dpilqr_hip.h"\nvoid* p[] = {(void*)dpilqr_policy_advance_dec_wide, (void*)dpilqr_cost_eval_wide};\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_bad_arguments_are_einval(lib):
    L = lib.load()
    d = _desc(lib, 130)                # T = 10, B = 2
    who = b"policy_advance_dec_wide"
    assert L.dpilqr_policy_advance_dec_wide(None, P, P, P, 1, P, 1, None, 4, 5, 2, None, None, P, P, P, P, P, P, P, P, P, 3, None) == lib.EINVAL
    for name in _REQUIRED:
        assert _call(lib, d, **{name: None}) == lib.EINVAL, name
        assert b"NULL" in L.dpilqr_last_error() and who in L.dpilqr_last_error(), name
    for kw in (dict(h=0), dict(h=11), dict(h=-1), dict(L=0), dict(n_d=0), dict(n_d=5), dict(n_scen=1)):
        assert _call(lib, d, **kw) == lib.EINVAL, kw
        assert (next(iter(kw)) + "=").encode() in L.dpilqr_last_error(), (kw, L.dpilqr_last_error())
    for name in tuple(f for f in _REQUIRED if f != "n_done") + ("K", "W", "u_lim", "bits"):
        assert _call(lib, d, **{name: P + 4}) == lib.EINVAL, name
        assert b"aligned" in L.dpilqr_last_error(), name
    assert _call(lib, d, scen=P + 2) == lib.EINVAL and _call(lib, d, n_done=P + 2) == lib.EINVAL      # int32 words
    assert _call(lib, d, bits=None) == lib.EINVAL and b"nbr_bits" in L.dpilqr_last_error()              # gains without masks
    assert _call(lib, _desc(lib, 70, 7, 2)) == lib.EINVAL and b"model family" in L.dpilqr_last_error()   # no such family
    for k, w in ((65, 1), (64, 2), (128, 3), (129, 2), (256, 5), (200, 0), (1, 0)):
        assert _call(lib, _desc(lib, k), n_words=w) == lib.EINVAL
        msg = L.dpilqr_last_error().decode()
        assert f"n_words={w}" in msg and f"= {(k + 63) // 64} words" in msg and "policy_advance_dec_wide" in msg, msg


def test_beyond_the_limits_is_unsupported_before_any_launch(lib):
    """With the fake pointers of this file a launch would not come back with these answers."""
    L = lib.load()
    for k in (257, 1000):
        assert _call(lib, _desc(lib, k)) == lib.EUNSUPPORTED
        assert f"k={k}" in L.dpilqr_last_error().decode() and "256" in L.dpilqr_last_error().decode()
    assert _call(lib, _desc(lib, 13, 5, 2)) == lib.EUNSUPPORTED and b"BikeDynamics5D" in L.dpilqr_last_error()      # dpilqr_rollout's bike limit
    for kd, kc_max in ((130, 0), (130, -1), (130, 65), (256, 65), (40, 41), (1, 2)):                               # 1 .. min(k, 64)
        assert _call(lib, _desc(lib, kd), kc_max=kc_max) == lib.EUNSUPPORTED, (kd, kc_max)
        assert b"kc_max" in L.dpilqr_last_error() and b"policy_advance_dec_wide" in L.dpilqr_last_error()
    assert _call(lib, _desc(lib, 130), K=None, bits=None, kc_max=0) == lib.EUNSUPPORTED      # open loop or not, as the team entry: kc_max is 1 ..
    # (more than 2^31 - 1 workgroups: the launcher's test stands, but with at least one item per workgroup and B an int32 no
    # descriptor reaches it -- as for the team entry)
    # the one-word entries keep their answer for such a team
    args = [C.byref(_desc(lib, 65)), P, P, P, 1, P, 1, None, 4, 5, 2, None, None, P, P, P, P, P, P, P, P, P, None]
    assert L.dpilqr_policy_advance_dec_team(*args) == lib.EUNSUPPORTED and b"k=65" in L.dpilqr_last_error()
    assert L.dpilqr_cost_eval(C.byref(_desc(lib, 65)), 1, P, P, 0, P, None) == lib.EUNSUPPORTED and b"k=65" in L.dpilqr_last_error()


def test_an_empty_batch_launches_nothing(lib):
    """B = 0 is DPILQR_OK, whatever the team's size within the limits."""
    for k, ns, nc in ((256, 4, 2), (129, 12, 4), (65, 3, 2), (64, 6, 3), (12, 5, 2), (1, 3, 2)):
        assert _call(lib, _desc(lib, k, ns, nc, B=0), kc_max=min(k, 64), n_scen=0) == lib.OK, (k, ns, nc)
        assert _call(lib, _desc(lib, k, ns, nc, B=0), K=None, bits=None) == lib.OK      # open loop: no gains, no masks


def test_cost_eval_wide_argument_checks(lib):
    L = lib.load()
    cost = lambda d, n_pts=1, x=P, u=P, out=P: L.dpilqr_cost_eval_wide(None if d is None else C.byref(d), n_pts, x, u, 0, out, None)
    assert cost(None) == lib.EINVAL
    for k in (257, 1000):
        assert cost(_desc(lib, k)) == lib.EUNSUPPORTED and f"k={k}".encode() in L.dpilqr_last_error() and b"256" in L.dpilqr_last_error()
    assert cost(_desc(lib, 13, 5, 2)) == lib.EUNSUPPORTED and b"BikeDynamics5D" in L.dpilqr_last_error()
    assert cost(_desc(lib, 70, 7, 2)) == lib.EINVAL and b"model family" in L.dpilqr_last_error()
    for bad in (dict(n_pts=-1), dict(x=None), dict(u=None), dict(out=None)):
        assert cost(_desc(lib, 256), **bad) == lib.EINVAL and b"cost_eval_wide" in L.dpilqr_last_error(), bad
    assert cost(_desc(lib, 256, B=0)) == lib.OK and cost(_desc(lib, 256), n_pts=0) == lib.OK and cost(_desc(lib, 65, 12, 4, B=0)) == lib.OK


# ---- the Python layers: every error before the device is touched
def _bare_batch(B=2, T=6, k=70, ns=4, nc=2):
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)      # no device state at all
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = B, T, k, ns, nc, k * ns, k * nc
    return pb


def _host_state(S=4, L=5, T=6, k=70, n=280, m=140, **over):
    import torch
    f64 = torch.float64
    st = dict(x_cur=torch.zeros((S, n), dtype=f64), n_done=torch.zeros((S,), dtype=torch.int32), X_exec=torch.zeros((S, L + 1, n), dtype=f64),
              U_exec=torch.zeros((S, L, m), dtype=f64), J_exec=torch.zeros((S,), dtype=f64), min_sep=torch.zeros((S,), dtype=f64),
              dist_left=torch.zeros((S, k), dtype=f64), U_next=torch.zeros((S, T, m), dtype=f64), X_next=torch.zeros((S, T + 1, n), dtype=f64))
    st.update(over)
    return st


def test_policy_advance_dec_wide_validates_on_the_host():
    import torch
    k, ns, nc, T = 70, 4, 2, 6
    n, m = k * ns, k * nc
    pb = _bare_batch(k=k, T=T)
    X, U, Kc = np.zeros((2, T + 1, n)), np.zeros((2, T, m)), np.zeros((2, T, k, nc, 2 * ns))
    own = wc.words_of([[[a] for a in range(k)]] * 2, k)
    own[0, 3, 1] |= np.uint64(1)       # agent 3 sees agent 64: a member in the second word
    three = own.copy(); three[0, 3, 1] |= np.uint64(2)
    past = own.copy(); past[1, 2, 1] |= np.uint64(1) << np.uint64(6)      # agent 70 of a team of 70
    lacking = own.copy(); lacking[1, 65, 1] = np.uint64(1)                # agent 65 with agent 64's bit instead of its own
    st = lambda **kw: _host_state(T=T, k=k, n=n, m=m, **kw)
    ok = dict(X=X, U_ff=U, Kc=Kc, nbr_bits=own, h=2, state=st(), scen=None, W=None, u_lim=None, n_d=2)
    bad = [dict(X=X[:, :T]), dict(U_ff=U[:, :, :5]), dict(Kc=np.zeros((2, T, m, n))), dict(Kc=np.zeros((2, T, k, nc, 2 * ns + 1))),
           dict(Kc=np.zeros((2, T, k, nc, 65 * ns))), dict(Kc=np.zeros((2, T, k, nc, 0))), dict(nbr_bits=own[:, :, 0]), dict(nbr_bits=own[:, :, :1]),
           dict(nbr_bits=own.astype(np.float64)), dict(nbr_bits=None), dict(h=0), dict(h=T + 1), dict(h=1.5), dict(n_d=0), dict(n_d=5),
           dict(scen=[0]), dict(scen=[0, 4]), dict(scen=[1, 1]), dict(W=np.zeros((4, 6, n))), dict(u_lim=np.zeros((m, 2))),
           dict(u_lim=np.array([[1.0] * m, [-1.0] * m])), dict(state={}), dict(state=st(S=1)),
           dict(state=st(n_done=torch.zeros((4,), dtype=torch.int64))), dict(nbr_bits=three), dict(nbr_bits=past), dict(nbr_bits=lacking)]
    for kw in bad:
        a = dict(ok); a.update(kw)
        with pytest.raises(ValueError, match="policy_advance_dec_wide"):
            pb.policy_advance_dec_wide(a["X"], a["U_ff"], a["Kc"], a["nbr_bits"], a["h"], a["state"], scen=a["scen"], W=a["W"], u_lim=a["u_lim"],
                                       n_d=a["n_d"])
    with pytest.raises(ValueError, match="policy_advance_dec_wide: a neighbourhood mask has 3 members, Kc holds kc_max = 2"):
        pb.policy_advance_dec_wide(X, U, Kc, three, 1, st())
    with pytest.raises(ValueError, match="at or past agent k = 70"):
        pb.policy_advance_dec_wide(X, U, Kc, past, 1, st())
    with pytest.raises(ValueError, match="policy_advance_dec_wide: a neighbourhood mask lacks its agent's own bit"):
        pb.policy_advance_dec_wide(X, U, Kc, lacking, 1, st())
    with pytest.raises(ValueError, match="1 <= kc_max <= 64"):
        pb.policy_advance_dec_wide(X, U, np.zeros((2, T, k, nc, 65 * ns)), own, 1, st())
    with pytest.raises(ValueError, match="policy_advance_dec_wide: h = 9"):
        pb.policy_advance_dec_wide(X, U, None, None, 9, st())      # open loop: no masks needed, the rest is checked all the same
    # the shared checks accept a team of 70 for the wide entry, and keep the routes' refusals for the others
    assert pb._advance_shapes("policy_advance_dec_wide", X, 2, st(), [3, 1], np.zeros((4, 5, n)), None, 2, (("U_ff", U, (2, T, m)),), wide=True) == (4, 5)
    with pytest.raises(ValueError, match="policy_advance_dec_team serves teams of up to 64 agents.*k = 70"):
        pb._advance_shapes("policy_advance_dec_team", X, 2, st(), None, None, None, 2, (("U_ff", U, (2, T, m)),), team=True)


def test_257_agents_and_13_bikes_are_refused():
    pb = _bare_batch(k=257)
    with pytest.raises(ValueError, match="policy_advance_dec_wide serves teams of up to 256 agents.*k = 257"):
        pb.policy_advance_dec_wide(np.zeros((2, 7, 1028)), np.zeros((2, 6, 514)), np.zeros((2, 6, 257, 2, 4)), np.ones((2, 257, 5), dtype=np.int64), 1, {})
    with pytest.raises(ValueError, match="policy_advance_dec_wide serves teams of up to 256 agents.*k = 257"):
        pb.policy_advance_dec_wide(np.zeros((2, 7, 1028)), np.zeros((2, 6, 514)), None, None, 1, {})
    with pytest.raises(ValueError, match="cost_wide serves teams of up to 256 agents.*k = 257"):
        pb.cost_wide(np.zeros((2, 1, 1028)), np.zeros((2, 1, 514)))
    pb = _bare_batch(k=13, ns=5, nc=2)
    with pytest.raises(ValueError, match="policy_advance_dec_wide.*five-state.*k = 13"):
        pb.policy_advance_dec_wide(np.zeros((2, 7, 65)), np.zeros((2, 6, 26)), np.zeros((2, 6, 13, 2, 5)), np.ones((2, 13, 1), dtype=np.int64), 1, {})


class _StubBatch:
    def __init__(self):
        self.calls = []

    def policy_advance_dec_wide(self, *a, **kw):
        self.calls.append(("policy_advance_dec_wide", a, kw))
        return "wide"

    def policy_advance_dec(self, *a, **kw):
        self.calls.append(("policy_advance_dec", a, kw))
        return "dec"


@pytest.mark.parametrize("k", [5, 64, 65, 256])
def test_distributed_policy_advance_routes_by_wide(k):
    from dpilqr_amd.dispatch import DistributedPolicy
    T, S = 4, 2
    X_dec, U_ff, Kc = np.zeros((S, T + 1, 4 * k)), np.zeros((S, T, 2 * k)), np.zeros((S, T, k, 2, 4))
    bits = np.ones((S, k, (k + 63) // 64), dtype=np.int64)
    pol = DistributedPolicy(dict(k=k), None, X_dec, U_ff, Kc, bits, 1, wide=True)
    stub = pol._batch = _StubBatch()
    state, scen, W, lim = {}, [1, 0], np.zeros((S, 5, 4 * k)), np.zeros((2, 2 * k))
    # the default on a wide policy: the pinned words, and a pointer at wide=True
    with pytest.raises(ValueError, match=r"the wide advance is not built.*wide=True"):
        pol.advance(1, state)
    with pytest.raises(ValueError, match="the wide advance is not built"):
        pol.advance(1, state, team=True)
    assert not stub.calls
    assert pol.advance(2, state, scen=scen, W=W, u_lim=lim, n_d=3, wide=True) == "wide"
    assert pol.advance(1, state, wide=True, team=True) == "wide"      # whatever team says
    assert [c[0] for c in stub.calls] == ["policy_advance_dec_wide"] * 2
    _, a, got = stub.calls[0]
    assert a[0] is X_dec and a[1] is U_ff and a[2] is Kc and a[3] is bits and a[4] == 2 and a[5] is state
    assert got["scen"] is scen and got["W"] is W and got["u_lim"] is lim and got["n_d"] == 3 and got["masks_checked"] is None
    assert stub.calls[1][2]["masks_checked"] is bits and "wide" not in got and "team" not in got      # the masks are checked by the first call only
    # wide=True on a one-word policy: solve with policy="wide"
    if k <= 64:
        narrow = DistributedPolicy(dict(k=k), None, X_dec, U_ff, Kc, np.ones((S, k), dtype=np.int64), 1)
        narrow._batch = _StubBatch()
        with pytest.raises(ValueError, match=r'wide=True needs a wide policy.*policy="wide"'):
            narrow.advance(1, state, wide=True)
        assert not narrow._batch.calls


# ---- solve_rhc_closed_loop(wide=True): the device replaced by the host, the batch and the solve by stubs
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

        def policy_advance_dec_wide(self, *a, **kw):
            return self._advance("policy_advance_dec_wide", *a, **kw)

        def cost(self, x, u, terminal=False):
            calls.append(("cost", terminal))
            return torch.zeros((x.shape[0], x.shape[1]), dtype=torch.float64)

        def cost_wide(self, x, u, terminal=False):
            calls.append(("cost_wide", terminal))
            return torch.zeros((x.shape[0], x.shape[1]), dtype=torch.float64)

    class StubPolicy:
        def advance(self, h, state, scen=None, team=False, wide=False, **kw):
            calls.append(("DistributedPolicy.advance", team, wide, h))
            state["n_done"][scen.long()] += h
            return state

    def solve_stub(problem, X, U, radius, xf=None, policy=False, **kw):
        S, T, m = U.shape
        n = X.shape[2]
        calls.append(("solve_scenarios_distributed", policy))
        return torch.zeros((S, T + 1, n), dtype=torch.float64), U.clone(), torch.ones((S,), dtype=torch.float64), dict(policy=StubPolicy() if policy else None)

    def constants_stub(d, kc=None):
        return dict(model=d["model"], n_dims=d["n_dims"], Q=d["Q"], R=d["R"], Qf=d["Qf"], word=0)

    monkeypatch.setattr(device_mod, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(batch_mod, "ProblemBatch", StubPB)
    monkeypatch.setattr(dispatch_mod, "device_constants", constants_stub)
    monkeypatch.setattr(dist_mod, "solve_scenarios_distributed", solve_stub)
    return calls


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("k", [3, 24, 64, 65, 256])
def test_the_loop_goes_through_the_wide_entries_whatever_the_size(stubbed_loop, k, feedback):
    import dpilqr_amd as dp
    calls = stubbed_loop
    out = dp.solve_rhc_closed_loop(_problem(k), np.ones((2, 4 * k)), 6, radius=1.0, centralized=False, feedback=feedback, step_size=2,
                                   dist_converge=1e-3, max_steps=4, wide=True)
    assert (out["n_rounds"] == 2).all() and not out["converged"].any()
    solves = [c for c in calls if c[0] == "solve_scenarios_distributed"]
    advances = [c for c in calls if c[0] not in ("solve_scenarios_distributed", "cost", "cost_wide")]
    assert solves == [("solve_scenarios_distributed", "wide" if feedback else False)] * 2 and len(advances) == 2
    if feedback:
        assert advances == [("DistributedPolicy.advance", False, True, 2)] * 2
    else:
        assert [c[0] for c in advances] == ["policy_advance_dec_wide"] * 2
        assert all(c[1] is None and c[2] is None and c[3] == 2 for c in advances)      # the stitched plan, open loop, no masks
    assert calls[-1] == ("cost_wide", True) and ("cost", True) not in calls            # the terminal cost of the final state


def test_the_loop_without_wide_is_as_before(stubbed_loop):
    import dpilqr_amd as dp
    kw = dict(dist_converge=0.1, max_steps=4)
    with pytest.raises(ValueError, match=r"^solve_rhc_closed_loop is not built for teams of more than 64 agents \(this one has 65\)$"):
        dp.solve_rhc_closed_loop(_problem(65), np.zeros((2, 260)), 10, radius=1.0, team=True, centralized=False, **kw)
    with pytest.raises(ValueError, match="n_x = 60.*large=True"):
        dp.solve_rhc_closed_loop(_problem(65), np.zeros((2, 260)), 10, radius=1.0, centralized=False, **kw)
    # ... and what wide=True does not serve
    with pytest.raises(ValueError, match=r"wide=True is the distributed loop \(centralized=False\)"):
        dp.solve_rhc_closed_loop(_problem(65), np.zeros((2, 260)), 10, radius=1.0, wide=True, **kw)
    with pytest.raises(ValueError, match=r"wide=True serves teams of up to 256 agents \(this one has 257\)"):
        dp.solve_rhc_closed_loop(_problem(257), np.zeros((2, 1028)), 10, radius=1.0, wide=True, centralized=False, **kw)
    with pytest.raises(ValueError, match="wide=True serves neither shard= nor ignore_ids"):
        dp.solve_rhc_closed_loop(_problem(65), np.zeros((2, 260)), 10, radius=1.0, wide=True, centralized=False, ignore_ids=[3], **kw)
    with pytest.raises(ValueError, match="wide=True serves neither shard= nor ignore_ids"):
        dp.solve_rhc_closed_loop(_problem(65), np.zeros((2, 260)), 10, radius=1.0, wide=True, centralized=False, shard=(0, 2), **kw)
    with pytest.raises(ValueError, match="radius"):
        dp.solve_rhc_closed_loop(_problem(65), np.zeros((2, 260)), 10, wide=True, centralized=False, **kw)
    assert not stubbed_loop      # nothing was solved or launched
    # a default-route loop of a small team still ends in cost, not cost_wide
    dp.solve_rhc_closed_loop(_problem(3), np.ones((2, 12)), 6, radius=1.0, centralized=False, step_size=2, dist_converge=1e-3, max_steps=2)
    assert stubbed_loop[-1] == ("cost", True) and not any(c[0] in ("cost_wide", "policy_advance_dec_wide") for c in stubbed_loop)


def test_the_pinned_tables_are_untouched():
    from dpilqr_amd import _lib
    from dpilqr_amd.batch import ROUTES, ProblemBatch
    assert "policy_advance_dec_wide" not in ProblemBatch.CLOSED_LOOP and len(ProblemBatch.CLOSED_LOOP) == 8 and sorted(ROUTES) == ["large", "small", "team"]
    assert not any("wide" in n for n in _lib.EXT_SIGNATURES) and len(_lib.SWARM_SIGNATURES) == 4 and len(_lib.SWARM_POLICY_SIGNATURES) == 2
    assert sorted(_lib.SWARM_ADVANCE_SIGNATURES) == [COST, ADVANCE]


# ---- the kernels in the built library
@pytest.fixture(scope="module")
def table(lib):
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("ns,nc", FAMILIES)
def test_wide_advance_kernels_keep_every_register(table, ns, nc):
    r = table[wc.kernel_name(f"k_policy_advance_dec_wide<{ns}, {nc}>")]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256, r
    # static LDS: the team advance's 256 (ns | 1) + 256 * 3 + 3 * 256 doubles and 3 * 256 ints at the least, under 64 KB
    assert 8 * 256 * ((ns | 1) + 6) + 4 * 3 * 256 <= r["group_segment_fixed_size"] < 64 * 1024, r


def test_no_further_wide_advance_kernel_was_built(table):
    # one kernel text, two word counts: the five four-word instantiations beside the five one-word ones, and nothing else
    names = sorted(n for n in table if "k_policy_advance_dec_team" in n or "k_policy_advance_dec_wide" in n)
    assert names == sorted(wc.kernel_name(f"k_policy_advance_dec_{width}<{ns}, {nc}>") for width in ("team", "wide") for ns, nc in FAMILIES)


def _recorded(path):
    """{kernel: (vgpr, agpr, static lds)} of a checks file's resource table."""
    rows = re.findall(r"^(k_policy_\w+<\d+, \d+>)\s+vgpr\s+(\d+) agpr\s+(\d+) .*static lds\s+(\d+) B", (ROOT / "profiles" / path).read_text(), re.M)
    return {n: (int(v), int(a), int(l)) for n, v, a, l in rows}


def test_the_restated_kernels_keep_their_recorded_figures(table):
    """The team advance and the wide rollout -- the one-word advance and the four-word rollout of the shared kernel texts, under
    the names their checks files recorded them by: registers and LDS are what those files record."""
    team = {n: f for n, f in _recorded("policy_advance_dec_team_checks.txt").items() if n.startswith("k_policy_advance_dec_team<")}
    wide = {n: f for n, f in _recorded("policy_dec_wide_checks.txt").items() if n.startswith("k_policy_rollout_dec_wide<")}
    assert len(team) == 5 and len(wide) == 5
    for name, want in {**team, **wide}.items():
        r = table[wc.kernel_name(name)]
        assert (r["vgpr_count"], r["agpr_count"], r["group_segment_fixed_size"]) == want, (name, r)
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r


# ---- the cases, on the prefixes the GPU tests execute: from the reference alone
@pytest.mark.parametrize("case", awc.CASES, ids=awc.IDS)
def test_the_cases_are_honest_on_a_prefix(case):
    ref = wc.case_ref(case)
    f3, f1 = awc.prefix_figures(case, ref, 3), awc.prefix_figures(case, ref, 1)
    print(case.id, "h=3", f3, "h=1", f1)
    assert 0.0 < f3["clamped"] < 1.0 and 0.0 < f1["clamped"] < 1.0, (f3, f1)      # the limits clamp some entries within the prefix, not all
    assert f3["near"] > 0.0 and f1["near"] > 0.0, (f3, f1)                       # W brings a share of the samples inside the radius
    assert all(u <= pc.MAX_UNCHECKED for u in f3["unchecked"].values()), f3      # within the cap the GPU test holds


def test_the_case_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    shape = {c.id: (c.k, 256 // c.k, len(awc.kept(c)), c.n_words) for c in awc.CASES}
    assert shape == {"wide-dint4-k65-S4": (65, 3, 11, 2), "wide-dint4_uni4-k86-S3": (86, 2, 9, 2), "wide-car3-k65-S3": (65, 3, 9, 2),
                     "wide-quad12-k65-S2": (65, 3, 6, 2), "wide-dint4-k129-S2": (129, 1, 6, 3), "wide-dint4-k256-S2": (256, 1, 6, 4)}
    assert {ipw for _, ipw, _, _ in shape.values()} == {1, 2, 3}                       # every ipw tier
    assert shape["wide-dint4-k65-S4"][2] % 3 == 2 and shape["wide-dint4_uni4-k86-S3"][2] % 2 == 1      # a partly filled last workgroup at ipw 3 and 2
    assert all(n > ipw for _, ipw, n, _ in shape.values())                             # more than one workgroup everywhere
    assert {(c.ns, c.nc) for c in awc.CASES} == {(3, 2), (4, 2), (12, 4)}              # (6, 3), (5, 2): the one-word cross-check
    assert awc.HS == (1, 3) and awc.SPARE == 3 and awc.N_D == 2
    assert (awc.LOOP_CASE.k, awc.N_LOOP, awc.S_LOOP, awc.H_LOOP, awc.L_LOOP) == (65, 10, 2, 2, 4)


# ---- the member walk
def test_the_member_walk_is_the_words_members():
    """The kernel's walk, in NumPy, against policy_dec_wide_cases.members_of: members on both sides of every word edge, every
    word count, k not a multiple of 64; with fewer than kc_max members all are kept, with more the lowest kc_max."""
    for case in awc.CASES:
        k, kc_max = case.k, case.kc_max
        words = wc.words_of(wc.make_members(case), k)
        for b in range(pc.B):
            want = wc.members_of(words[b], k)
            assert [awc.member_walk(words[b, a], k, kc_max) for a in range(k)] == want
            assert [awc.member_walk(words[b, a], k, 2) for a in range(k)] == [m[:2] for m in want]      # truncated: the lowest
    k = 256
    edges = [0, 63, 64, 127, 128, 191, 192, 255]
    w = wc.words_of([[edges]], k)[0, 0]
    assert awc.member_walk(w, k, 64) == edges and awc.member_walk(w, k, 3) == edges[:3] and awc.member_walk(w, k, 5) == edges[:5]
    # bits at and past k are not members; words past n_words do not exist
    w = np.array([np.uint64(1) << np.uint64(63), np.uint64(0b111)], dtype=np.uint64)
    assert awc.member_walk(w, 66, 8) == [63, 64, 65] and awc.member_walk(w, 65, 8) == [63, 64] and awc.member_walk(w, 64, 8) == [63]
    assert awc.member_walk(w[:1], 65, 8) == [63]
