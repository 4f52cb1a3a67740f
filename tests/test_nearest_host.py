"""Neighbourhoods capped at their m nearest agents, the host side, without a GPU: the entry is declared (include/dpilqr_nearest.h),
bound and exported; every refusal arrives before any launch (fake, aligned device pointers or NULL, in the style of
tests/test_swarm_host.py) with its message; the host layers raise for a bad cap before any device work; every layer hands the cap
on; and with the default max_cluster=None the front end calls the entries it always called, with the arguments it always gave them.
The kernel carries no scratch and no spills."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.test_policy_advance_dec_team_host import stubbed_loop  # noqa: F401  (the loop with the device replaced by the host)

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test
NAME = "dpilqr_dispatch_graph_nearest"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


def test_symbol_is_declared_bound_and_exported(lib):
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    core, ext = strip((ROOT / "include" / "dpilqr_hip.h").read_text()), strip((ROOT / "include" / "dpilqr_nearest.h").read_text())
    assert re.search(r'^\s*#\s*include\s+"dpilqr_nearest.h"', core, re.M)
    decl = dict(re.findall(r"\bint32_t\s+(dpilqr_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", ext))
    assert sorted(decl) == [NAME] == sorted(lib.NEAREST_SIGNATURES)
    names = [a.split()[-1].lstrip("*") for a in decl[NAME].split(",")]
    assert names == ["S", "N", "k", "n_s", "X", "radius", "radius_stride", "ignore", "max_cluster", "bits", "rep", "size", "order", "slot",
                     "bucket_start", "bucket_count", "dropped", "n_words", "stream"]
    fn = getattr(lib.load(), NAME)
    assert fn.argtypes == lib.NEAREST_SIGNATURES[NAME][1] and len(fn.argtypes) == 19 and fn.restype is C.c_int32
    wide = lib.SWARM_SIGNATURES["dpilqr_dispatch_graph_wide"][1]      # the wide entry's arguments plus max_cluster and dropped
    assert fn.argtypes == wide[:8] + [C.c_int32] + wide[8:15] + [C.c_void_p] + wide[15:]
    others = set(lib.SIGNATURES) | set(lib.EXT_SIGNATURES) | set(lib.SWARM_SIGNATURES) | set(lib.SWARM_POLICY_SIGNATURES) | set(lib.SWARM_ADVANCE_SIGNATURES)
    assert NAME not in others
    assert lib.load().dpilqr_abi_version() == 4 and lib.ABI_VERSION == 4      # additive: the ABI version stays


def test_the_header_compiles_as_c(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dpilqr_hip.h"\nint32_t (*p)(int32_t, int32_t, int32_t, int32_t, const double*, const double*, int64_t, const int32_t*, '
                   'int32_t, uint64_t*, int32_t*, int32_t*, int32_t*, int32_t*, int32_t*, int32_t*, int32_t*, int32_t, void*) = '
                   'dpilqr_dispatch_graph_nearest;\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def _call(L, k, m, n_words=None, S=2, N=1, n_s=4, ptrs=P, null=()):
    """The entry with fake pointers (NULL for the positions in `null`, 0 = X ... ); nothing is launched by a refused call"""
    p = [None if i in null else ptrs for i in range(9)]      # X, radius, bits, rep, size, order, slot, bucket_start, bucket_count
    nw = (k + 63) // 64 if n_words is None else n_words
    return L.dpilqr_dispatch_graph_nearest(S, N, k, n_s, p[0], p[1], 1, None, m, *p[2:], None, nw, None)


def test_every_refusal_arrives_before_any_launch(lib):
    L = lib.load()
    msg = lambda: L.dpilqr_last_error().decode()
    # the wide entry's conditions: k, n_words ...
    for k, w in ((0, 1), (-3, 1), (257, 5), (1000, 16)):
        assert _call(L, k, 1, w, ptrs=None) == lib.EINVAL and f"k={k}" in msg() and "256" in msg() and "dispatch_graph_nearest" in msg()
    for k, w in ((65, 1), (64, 2), (128, 3), (129, 2), (256, 5), (200, 0)):
        assert _call(L, k, 1, w, ptrs=None) == lib.EINVAL
        assert f"n_words={w}" in msg() and f"= {(k + 63) // 64} words" in msg(), msg()
    # ... the cap, named with its bound, with NULL pointers (it is checked before them) and with plausible ones
    for k, m, bound in ((6, 0, 6), (6, -1, 6), (6, 7, 6), (64, 65, 64), (65, 65, 64), (256, 65, 64), (256, 256, 64), (1, 2, 1)):
        for ptrs in (None, P):
            assert _call(L, k, m, ptrs=ptrs) == lib.EINVAL
            assert f"max_cluster={m}" in msg() and f"min(k, 64) = {bound}" in msg(), msg()
    # ... S, N, n_s and every NULL pointer
    for kw in (dict(S=-1), dict(N=0), dict(n_s=1)):
        assert _call(L, 65, 4, **kw) == lib.EINVAL and "dispatch_graph_nearest: bad argument" in msg()
    for i in range(9):
        assert _call(L, 65, 4, null=(i,)) == lib.EINVAL and "dispatch_graph_nearest: bad argument" in msg(), i
    # the other graph entries are as they were: no cap, no 65 agents on the narrow one
    assert L.dpilqr_dispatch_graph(2, 1, 65, 4, P, P, 1, None, P, P, P, P, P, P, P, None) == lib.EINVAL and "dispatch_graph:" in msg()


def _problem(k):
    import dpilqr_amd as dp
    ids = [100 + i for i in range(k)]
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1, i) for i in ids])
    refs = [dp.ReferenceCost(np.zeros(4), np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), i) for i in ids]
    return dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([4] * k, 0.5, [2] * k)))


BAD_CAPS = (0, -2, 65, 1000, 2.0, "3", True, [3])


def test_a_bad_cap_is_a_value_error_before_any_device_work(lib):
    """None of these reaches the device (there is none here): the ValueError is the first thing that happens."""
    import dpilqr_amd as dp
    from dpilqr_amd.dispatch import ScenarioFrontEnd, checked_max_cluster, solve_scenarios_distributed
    from dpilqr_amd.lowering import describe
    k, T = 6, 4
    p = _problem(k)
    X, U = np.zeros((2, 1, k * 4)), np.zeros((2, T, k * 2))
    for bad in BAD_CAPS:
        match = re.escape(f"max_cluster={bad!r}")
        with pytest.raises(ValueError, match=match):
            ScenarioFrontEnd(describe(p), X, U, 0.5, None, max_cluster=bad)
        with pytest.raises(ValueError, match=match):
            solve_scenarios_distributed(p, X, U, 0.5, max_cluster=bad)
        with pytest.raises(ValueError, match=match):
            dp.closed_loop_distributed(p, X[0], U[0], 0.5, np.zeros((1, k * 4)), max_cluster=bad)
        with pytest.raises(ValueError, match=match):
            dp.solve_rhc_scenarios(p, np.zeros((2, k * 4)), T, 0.5, dist_converge=0.1, max_cluster=bad)
        with pytest.raises(ValueError, match=match):
            dp.solve_rhc_closed_loop(p, np.zeros((2, k * 4)), T, radius=0.5, centralized=False, dist_converge=0.1, max_steps=2, max_cluster=bad)
        with pytest.raises(ValueError, match=match):
            dp.nearest_neighbourhoods(X[0], 0.5, [4] * k, p.ids, bad)
        with pytest.raises(ValueError, match=match):
            dp.solve_distributed(p, X[0], U[0], 0.5, verbose=False, max_cluster=bad)
    assert [checked_max_cluster(m, 6) for m in (1, 5, 6, 7, 64, np.int32(3))] == [1, 5, 6, 6, 6, 3]      # clamped to min(m, k)
    with pytest.raises(ValueError, match=r"max_cluster caps the neighbourhoods of the distributed loop \(centralized=False\)"):
        dp.solve_rhc_closed_loop(p, np.zeros((2, k * 4)), T, dist_converge=0.1, max_steps=2, max_cluster=3)
    with pytest.raises(ValueError, match=r"max_cluster caps the neighbourhoods of the distributed solve \(centralized=False\)"):
        dp.solve_rhc_scenarios(p, np.zeros((2, k * 4)), T, 0.5, centralized=True, dist_converge=0.1, max_cluster=3)
    # the wide team's refusals are as they were, cap or not
    p65 = _problem(65)
    X65, U65 = np.zeros((2, 1, 260)), np.zeros((2, T, 130))
    with pytest.raises(ValueError, match=r"policy=True is not built for teams of more than 64 agents \(this one has 65\)"):
        solve_scenarios_distributed(p65, X65, U65, 0.5, policy=True, max_cluster=4)
    with pytest.raises(ValueError, match=r"shard= is not built for teams of more than 64 agents \(this one has 65\)"):
        solve_scenarios_distributed(p65, X65, U65, 0.5, shard=(0, 2), max_cluster=4)


class _Recorder:
    """Stands in for the loaded library: every entry records (name, args) and answers DPILQR_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("dpilqr_"):
            raise AttributeError(name)
        return lambda *a: (self.calls.append((name, a)), 0)[1]


@pytest.fixture
def host_front_end(monkeypatch, lib):
    """ScenarioFrontEnd with the device replaced by the host and the library by a recorder (buffers are zeroed: no bucket is populated)"""
    import torch
    import dpilqr_amd.device as device_mod
    import dpilqr_amd.dispatch as dispatch_mod
    rec = _Recorder()
    monkeypatch.setattr(device_mod, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(dispatch_mod, "empty", lambda shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype))
    monkeypatch.setattr(dispatch_mod, "stream_handle", lambda: 77)
    monkeypatch.setattr(lib, "load", lambda: rec)
    return rec


def test_default_reaches_the_old_entries_and_a_cap_the_new_one(host_front_end, lib):
    from dpilqr_amd.dispatch import ScenarioFrontEnd
    from dpilqr_amd.lowering import describe
    rec, T = host_front_end, 4
    for k, wide, entry in ((6, None, "dpilqr_dispatch_graph"), (6, True, "dpilqr_dispatch_graph_wide"), (65, None, "dpilqr_dispatch_graph_wide"),
                           (130, None, "dpilqr_dispatch_graph_wide")):
        d = describe(_problem(k))
        X, U = np.zeros((2, 1, k * 4)), np.zeros((2, T, k * 2))
        nw = (k + 63) // 64
        is_wide = wide or k > 64
        del rec.calls[:]
        fe = ScenarioFrontEnd(d, X, U, 0.5, None, wide=wide)      # max_cluster=None: the default
        (name, old), = rec.calls
        assert name == entry and fe.max_cluster is None and fe.dropped is None
        assert len(old) == (17 if is_wide else 16) and old[:4] == (2, 1, k, 4) and old[6:8] == (1, None) and old[-1] == 77
        assert not is_wide or old[-2] == nw
        assert tuple(fe.bits.shape) == ((2 * k, nw) if is_wide else (2 * k,))
        for m, m_eff in ((3, 3), (64, min(64, k)), (np.int64(5), 5)):
            del rec.calls[:]
            fe = ScenarioFrontEnd(d, X, U, 0.5, None, wide=wide, max_cluster=m)
            (name, new), = rec.calls
            assert name == NAME and len(new) == 19 and fe.max_cluster == m_eff and tuple(fe.dropped.shape) == (2 * k,)
            assert new[:4] == old[:4] and new[6:8] == old[6:8] and new[8] == m_eff and type(new[8]) is int
            assert new[16] == fe.dropped.data_ptr() and new[17] == nw and new[18] == 77
            assert tuple(fe.bits.shape) == ((2 * k, nw) if is_wide else (2 * k,))      # k <= 64 without wide=: one word, bits stays (S*k,)


class _Stop(Exception):
    pass


def test_every_layer_hands_the_cap_on(monkeypatch, stubbed_loop, lib):  # noqa: F811
    import dpilqr_amd as dp
    import dpilqr_amd.dispatch as dispatch_mod
    import dpilqr_amd.distributed as dist_mod
    k, T = 6, 4
    p = _problem(k)
    seen = []

    def solve_stub(problem, X, U, radius, **kw):
        seen.append(kw.get("max_cluster", "absent"))
        raise _Stop

    def through(call):
        del seen[:]
        with pytest.raises(_Stop):
            call()
        return seen[-1]

    x0 = np.ones((2, k * 4))
    for mod in (dist_mod, dispatch_mod):
        monkeypatch.setattr(mod, "solve_scenarios_distributed", solve_stub)
    for want, kw in ((None, {}), (3, dict(max_cluster=3)), (64, dict(max_cluster=64))):
        assert through(lambda: dp.closed_loop_distributed(p, x0[:1], np.zeros((T, k * 2)), 0.5, x0[:1], **kw)) == want
        assert through(lambda: dp.closed_loop_distributed(p, x0[:1], np.zeros((T, k * 2)), 0.5, x0[:1], wide=True, **kw)) == want
        assert through(lambda: dp.solve_rhc_scenarios(p, x0, T, 0.5, U0=np.zeros((2, T, k * 2)), dist_converge=0.1, **kw)) == want
        for route in (dict(), dict(team=True), dict(wide=True)):
            assert through(lambda: dp.solve_rhc_closed_loop(p, x0, T, radius=0.5, U0=np.zeros((2, T, k * 2)), centralized=False, dist_converge=0.1,
                                                            max_steps=2, **route, **kw)) == want
    assert through(lambda: dp.solve_rhc_closed_loop(_problem(24), np.ones((2, 96)), T, radius=0.5, U0=np.zeros((2, T, 48)), centralized=False,
                                                    dist_converge=0.1, max_steps=2, team=True, max_cluster=5)) == 5

    # solve_scenarios_distributed itself -> the front end
    class FrontEndStub:
        def __init__(self, d, X, U, radius, xf, ignore=None, wide=None, max_cluster=None):
            seen.append((wide, max_cluster))
            raise _Stop

    monkeypatch.undo()
    monkeypatch.setattr(dispatch_mod, "ScenarioFrontEnd", FrontEndStub)
    X, U = np.zeros((2, 1, k * 4)), np.zeros((2, T, k * 2))
    assert through(lambda: dispatch_mod.solve_scenarios_distributed(p, X, U, 0.5)) == (None, None)
    assert through(lambda: dispatch_mod.solve_scenarios_distributed(p, X, U, 0.5, max_cluster=3)) == (None, 3)
    assert through(lambda: dispatch_mod.solve_scenarios_distributed(p, X, U, 0.5, policy="wide", max_cluster=3)) == (True, 3)
    assert through(lambda: dispatch_mod.solve_scenarios_distributed(p, X, U, 0.5, policy=True, max_cluster=2)) == (None, 2)
    assert through(lambda: dispatch_mod.solve_scenarios_distributed(p, X, U, 0.5, shard=(0, 2), ignore_ids=[101], max_cluster=2)) == (None, 2)


def test_solve_distributed_prunes_its_host_graph(monkeypatch, lib):
    """solve_distributed(max_cluster=m) splits the problem over nearest_neighbourhoods' graph; solve_rhc reaches it through **kwargs."""
    import dpilqr_amd as dp
    import dpilqr_amd.distributed as dist_mod
    from tests import nearest_cases as nc
    k = 6
    x0, xf, X = nc.scenario(k)
    p = _problem(k)
    graphs = []

    def solve_stub(problems, x0s, U0s, keys=None, **kw):
        graphs.append((keys, kw))
        raise _Stop

    monkeypatch.setattr(dist_mod, "solve_problem_list", solve_stub)
    want = nc.reference(X[0], k, nc.NS, nc.GRAPH_RADIUS, 3)[0]
    for call in (lambda **kw: dp.solve_distributed(p, X[0], np.zeros((10, k * 2)), nc.GRAPH_RADIUS, verbose=False, n_lqr_iter=7, **kw),
                 lambda **kw: dp.solve_rhc(p, x0[0], 10, nc.GRAPH_RADIUS, centralized=False, dist_converge=0.01, n_lqr_iter=7, **kw)):
        X_in = X[0] if not graphs else x0[0][None]
        for m in (None, 3):
            with pytest.raises(_Stop):
                call(**({} if m is None else dict(max_cluster=m)))
            keys, kw = graphs[-1]
            ref = nc.reference(X_in, k, nc.NS, nc.GRAPH_RADIUS, 64 if m is None else m)[0]
            assert [[p.ids.index(int(j)) for j in key] for key in keys] == [ref[i] for i in range(k)]
            assert kw == dict(n_lqr_iter=7)      # the cap is an argument of its own, not a solver keyword
        graphs.append(None)
    assert max(len(v) for v in want.values()) == 3


@pytest.fixture(scope="module")
def table(lib):
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("nw", [1, 2, 3, 4])
def test_the_kernel_keeps_every_register(table, nw):
    r = table[f"k_graph_bits_nearest<{nw}>"]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256 and r["group_segment_fixed_size"] == 0      # the LDS is dynamic: at most 86,016 B


def test_the_lds_budget_is_what_the_header_says():
    src = (ROOT / "dpilqr_amd" / "csrc" / "frontend_nearest.hpp").read_text()
    assert "graph_wide_lds_bytes(N, k) + sizeof(double) * kNearestWaves * kWideMaxAgents" in src
    rows = max((N + max(N // 10, 1) - 1) // max(N // 10, 1) for N in range(1, 2000))
    assert rows == 19 and 8 * 2 * rows * 256 + 8 * 4 * 256 == 86016 < 160 * 1024
