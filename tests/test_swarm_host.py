"""Teams of more than 64 agents, the host side, without a GPU: the four new entries are declared (include/dpilqr_swarm.h), bound
and exported; every refusal arrives before any launch (fake, aligned device pointers in the style of tests/test_policy_host.py)
or before any device work, with its message; the narrow entries still refuse k = 65; the new kernels carry no scratch."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test
NAMES = {"dpilqr_dispatch_graph_wide": 17, "dpilqr_dispatch_gather_wide": 20, "dpilqr_dispatch_stitch_wide": 14, "dpilqr_rollout_wide": 8}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


def test_symbols_are_declared_bound_and_exported(lib):
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    core, ext = strip((ROOT / "include" / "dpilqr_hip.h").read_text()), strip((ROOT / "include" / "dpilqr_swarm.h").read_text())
    assert re.search(r'^\s*#\s*include\s+"dpilqr_swarm.h"', core, re.M)
    decl = dict(re.findall(r"\bint32_t\s+(dpilqr_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", ext))
    assert sorted(decl) == sorted(NAMES) == sorted(lib.SWARM_SIGNATURES)
    assert not set(lib.SWARM_SIGNATURES) & (set(lib.SIGNATURES) | set(lib.EXT_SIGNATURES))
    for name, n_args in NAMES.items():
        assert len(decl[name].split(",")) == n_args == len(lib.SWARM_SIGNATURES[name][1]), name
        fn = getattr(lib.load(), name)
        assert fn.argtypes == lib.SWARM_SIGNATURES[name][1] and fn.restype is C.c_int32
    # each wide dispatch entry: its narrow counterpart's arguments plus n_words
    for narrow in ("graph", "gather", "stitch"):
        a, b = lib.SIGNATURES[f"dpilqr_dispatch_{narrow}"][1], lib.SWARM_SIGNATURES[f"dpilqr_dispatch_{narrow}_wide"][1]
        assert b == a[:-1] + [C.c_int32, C.c_void_p]
    assert lib.load().dpilqr_abi_version() == 4 and lib.ABI_VERSION == 4      # additive: the ABI version stays
    assert lib.MAX_AGENTS == 64 and lib.MAX_TEAM == 256
    assert re.search(r"#define\s+DPILQR_MAX_TEAM\s+256\b", ext) and re.search(r"#define\s+DPILQR_MAX_AGENTS\s+64\b", core)


def test_the_header_compiles_as_c(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dpilqr_hip.h"\nint32_t (*p)(const dpilqr_batch_desc*, const double*, const double*, double*, double*, double*, double*, '
                   'void*) = dpilqr_rollout_wide;\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def _graph(L, k, n_words=None, wide=True):
    args = [2, 1, k, 4, P, P, 1, None, P, P, P, P, P, P, P]
    return L.dpilqr_dispatch_graph_wide(*args, n_words, None) if wide else L.dpilqr_dispatch_graph(*args, None)


def _gather(L, k, n_words=None, wide=True, kc=1):
    args = [k, 4, 2, 5, 1, kc, P, 0, 1, P, P, P, P, 4 * k, P, P, P, None]
    return L.dpilqr_dispatch_gather_wide(*args, n_words, None) if wide else L.dpilqr_dispatch_gather(*args, None)


def _stitch(L, lib, k, n_words=None, wide=True):
    R = lib.BucketResults()
    args = [2, k, 4, 2, 5, P, P, P, P, C.addressof(R), P, P]
    return L.dpilqr_dispatch_stitch_wide(*args, n_words, None) if wide else L.dpilqr_dispatch_stitch(*args, None)


def test_wide_entries_check_k_and_n_words_before_any_launch(lib):
    L = lib.load()
    for call in (lambda k, w: _graph(L, k, w), lambda k, w: _gather(L, k, w), lambda k, w: _stitch(L, lib, k, w)):
        for k, w in ((0, 1), (-3, 1), (257, 5), (1000, 16)):
            assert call(k, w) == lib.EINVAL
            assert f"k={k}" in L.dpilqr_last_error().decode() and "256" in L.dpilqr_last_error().decode()
        for k, w in ((65, 1), (64, 2), (128, 3), (129, 2), (256, 5), (200, 0)):
            assert call(k, w) == lib.EINVAL
            msg = L.dpilqr_last_error().decode()
            assert f"n_words={w}" in msg and f"= {(k + 63) // 64} words" in msg, msg
    assert _gather(L, 130, 3, kc=65) == lib.EINVAL and "kc=65" in L.dpilqr_last_error().decode()      # a sub-problem has <= 64 agents


def test_narrow_entries_still_refuse_65_agents(lib):
    L = lib.load()
    assert _graph(L, 65, wide=False) == lib.EINVAL and b"dispatch_graph" in L.dpilqr_last_error()
    assert _gather(L, 65, wide=False) == lib.EINVAL and _stitch(L, lib, 65, wide=False) == lib.EINVAL
    d = lib.BatchDesc(1, 65, 4, 2, 5, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)
    assert L.dpilqr_rollout(C.byref(d), P, P, P, P, None) == lib.EUNSUPPORTED and b"exceeds 64" in L.dpilqr_last_error()


def test_rollout_wide_argument_checks(lib):
    L = lib.load()
    desc = lambda k, ns=4, nc=2: lib.BatchDesc(1, k, ns, nc, 5, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)
    for k in (257, 1000):
        assert L.dpilqr_rollout_wide(C.byref(desc(k)), P, P, None, P, None, None, None) == lib.EUNSUPPORTED
        assert f"k={k}" in L.dpilqr_last_error().decode() and "256" in L.dpilqr_last_error().decode()
    d = desc(200)
    assert L.dpilqr_rollout_wide(None, P, P, None, P, None, None, None) == lib.EINVAL
    for bad in ((None, P, P), (P, None, P), (P, P, None)):      # x0, U, J
        assert L.dpilqr_rollout_wide(C.byref(d), bad[0], bad[1], None, bad[2], None, None, None) == lib.EINVAL
        assert b"rollout_wide: NULL" in L.dpilqr_last_error()
    for i in range(6):      # check_desc's alignment rule, every pointer
        ptrs = [P] * 6
        ptrs[i] = P + 4
        assert L.dpilqr_rollout_wide(C.byref(d), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], None) == lib.EINVAL
        assert b"aligned" in L.dpilqr_last_error()
    assert L.dpilqr_rollout_wide(C.byref(desc(13, 5, 2)), P, P, None, P, None, None, None) == lib.EUNSUPPORTED      # dpilqr_rollout's bike limit
    assert L.dpilqr_rollout_wide(C.byref(desc(70, 7, 2)), P, P, None, P, None, None, None) == lib.EINVAL          # no such family


def _problem(k):
    import dpilqr_amd as dp
    ids = [100 + i for i in range(k)]
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1, i) for i in ids])
    refs = [dp.ReferenceCost(np.zeros(4), np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), i) for i in ids]
    return dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([4] * k, 0.5, [2] * k)))


def test_python_refusals_come_before_any_device_work(lib):
    """None of these reaches the device (there is none here): the ValueError is the first thing that happens."""
    import dpilqr_amd as dp
    from dpilqr_amd.batch import ProblemBatch
    from dpilqr_amd.dispatch import ScenarioFrontEnd, solve_scenarios_distributed
    from dpilqr_amd.lowering import describe
    from dpilqr_amd.util import random_setup_batch
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
    with pytest.raises(ValueError, match="policy=True"):
        dp.distributed.closed_loop_distributed(p65, X[0], U[0], 0.5, np.zeros((1, 65 * 4)))
    d257 = dict(describe(_problem(2)), k=257)
    with pytest.raises(ValueError, match="at most 256 agents per problem, this one has 257"):
        ScenarioFrontEnd(d257, np.zeros((1, 1, 257 * 4)), np.zeros((1, T, 257 * 2)), 0.5, None)
    with pytest.raises(ValueError, match="65 agents need the wide entries"):
        ScenarioFrontEnd(describe(p65), X, U, 0.5, None, wide=False)
    pb = ProblemBatch.__new__(ProblemBatch)
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 1, T, 257, 4, 2, 257 * 4, 257 * 2
    with pytest.raises(ValueError, match="rollout_wide serves teams of up to 256 agents, this batch has k = 257"):
        pb.rollout_wide(np.zeros((1, 257 * 4)), np.zeros((1, T, 257 * 2)))


@pytest.fixture(scope="module")
def table(lib):
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("ns,nc", [(3, 2), (4, 2), (5, 2), (6, 3), (12, 4)])
def test_rollout_wide_kernels_keep_every_register(table, ns, nc):
    r = table[f"k_rollout_wide<{ns}, {nc}>"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256


@pytest.mark.parametrize("name", ["k_graph_bits_wide", "k_dedup_wide", "k_bucket_sort_wide", "k_gather_bucket_wide", "k_stitch_wide"])
def test_wide_front_end_kernels_keep_every_register(table, name):
    r = table[f"dpilqr::{name}"] if f"dpilqr::{name}" in table else next(v for q, v in table.items() if q.split("(")[0].endswith(name))
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
