"""The large-cluster closed-loop rollout's host side, without a GPU: the cases are honest (from the CPU reference alone), the symbol
is declared, exported and bound, its limits answer before any launch (fake, aligned device pointers as in
tests/test_policy_host.py), ProblemBatch.policy_rollout_large validates on the host, and the three instantiations of
k_policy_rollout_large keep their registers where k_policy_rollout of the same family keeps them."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_large_cases as plc

ROOT = Path(__file__).resolve().parent.parent
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test
NAME = "dpilqr_policy_rollout_large"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


def _desc(lib, k, ns, nc, B=2, T=10):
    return lib.BatchDesc(B, k, ns, nc, T, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)


def _call(lib, d, X=P, U=P, K=P, S=4, x0s=P, W=None, u_lim=None, Xs=None, Us=None, J=P, sep=None, goal=None):
    return lib.load().dpilqr_policy_rollout_large(C.byref(d), X, U, K, S, x0s, W, u_lim, Xs, Us, J, sep, goal, None)


@pytest.mark.parametrize("case", plc.CASES, ids=[c.id for c in plc.CASES])
def test_case_conditions(case):
    """From the reference alone: the case exercises what it is meant to, and stays inside the unchecked cap."""
    from tests import linesearch_cases as lc
    before = dict(lc.U0_NOISE)
    ref = plc.case_ref(case)
    assert lc.U0_NOISE == before      # the noise supplied for model 8 is gone again
    f = ref.figures()
    print(case.id, f)
    assert case.S == plc.SPW[case.id] + 1 and case.k * case.ns > 60
    assert 0.10 <= f["clamped"] <= 0.90, f
    assert f["near"] >= 0.10, f
    assert f["moved"] >= 0.5, f
    assert all(u <= pc.MAX_UNCHECKED for u in f["unchecked"].values()), f


def test_symbol_is_declared_exported_and_bound(lib):
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    ext = strip((ROOT / "include" / "dpilqr_policy.h").read_text())
    m = re.search(r"\bint32_t\s+" + NAME + r"\s*\(([^)]*)\)\s*;", ext)
    assert m, "not declared in include/dpilqr_policy.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert NAME in lib.EXT_SIGNATURES and NAME not in lib.SIGNATURES
    assert len(lib.EXT_SIGNATURES[NAME][1]) == n_args == 14
    assert sorted(set(re.findall(r"\b(dpilqr_[a-z_0-9]+)\s*\(", ext))) == sorted(lib.EXT_SIGNATURES)
    fn = getattr(lib.load(), NAME)
    assert fn.argtypes == lib.EXT_SIGNATURES[NAME][1] and fn.restype is C.c_int32
    assert lib.EXT_SIGNATURES[NAME] == lib.EXT_SIGNATURES["dpilqr_policy_rollout"]      # the same arguments
    assert lib.load().dpilqr_abi_version() == 4      # additive: the ABI version stays


def test_the_header_compiles_as_c(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dpilqr_hip.h"\nint32_t (*p)(const dpilqr_batch_desc*, const double*, const double*, const double*, int32_t, const double*, '
                   'const double*, const double*, double*, double*, double*, double*, double*, void*) = ' + NAME + ';\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_small_clusters_are_the_other_entry_points(lib):
    for k, ns, nc in ((5, 4, 2), (10, 6, 3), (5, 12, 4)):
        assert _call(lib, _desc(lib, k, ns, nc)) == lib.EUNSUPPORTED
        msg = lib.load().dpilqr_last_error().decode()
        assert "policy_rollout_large" in msg and f"n_x={k * ns}" in msg, msg
        assert re.search(r"\bdpilqr_policy_rollout\b(?!_)", msg), msg


def test_beyond_the_served_sizes_is_unsupported_before_any_launch(lib):
    for k, ns, nc in ((21, 12, 4), (21, 4, 2)):
        assert _call(lib, _desc(lib, k, ns, nc)) == lib.EUNSUPPORTED
        msg = lib.load().dpilqr_last_error().decode()
        assert "policy_rollout_large" in msg and f"n_x={k * ns}" in msg, msg
    assert _call(lib, _desc(lib, 6, 12, 4, B=1 << 30), S=43 * 3) == lib.EUNSUPPORTED      # 3 * 2^30 workgroups
    assert b"workgroups" in lib.load().dpilqr_last_error()


def test_bad_arguments_are_einval(lib):
    d = _desc(lib, 16, 4, 2)
    L = lib.load()
    assert _call(lib, d, X=None) == lib.EINVAL and b"NULL" in L.dpilqr_last_error()
    assert _call(lib, d, x0s=None) == lib.EINVAL and b"NULL" in L.dpilqr_last_error()
    assert _call(lib, d, U=None) == lib.EINVAL and _call(lib, d, K=None) == lib.EINVAL and _call(lib, d, J=None) == lib.EINVAL
    assert _call(lib, d, S=0) == lib.EINVAL and b"n_samples=0" in L.dpilqr_last_error()
    assert _call(lib, d, S=-3) == lib.EINVAL
    for name in ("X", "U", "K", "x0s", "W", "u_lim", "Xs", "Us", "J", "sep", "goal"):      # check_desc's alignment rule
        assert _call(lib, d, **{name: P + 4}) == lib.EINVAL, name
        assert b"aligned" in L.dpilqr_last_error(), name
    assert L.dpilqr_policy_rollout_large(None, P, P, P, 1, P, None, None, None, None, P, None, None, None) == lib.EINVAL
    bad = lib.BatchDesc(2, 16, 4, 2, 10, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P + 4, 0, P, 0, P, 0, P, 0, P, 0)      # a misaligned xf
    assert _call(lib, bad) == lib.EINVAL


def test_an_empty_batch_is_ok(lib):
    for k, ns, nc in ((16, 4, 2), (11, 6, 3), (20, 12, 4)):
        assert _call(lib, _desc(lib, k, ns, nc, B=0)) == lib.OK


def test_policy_rollout_large_validates_on_the_host():
    """Every shape or size error is a ValueError naming policy_rollout_large, raised before the device is touched: the batch
    object here has no device state at all.  The shapes are tests/test_policy_host.py's, scaled to n_x = 64."""
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 2, 6, 16, 4, 2, 64, 32
    assert pb.is_large
    X, U, K = np.zeros((2, 7, 64)), np.zeros((2, 6, 32)), np.zeros((2, 6, 32, 64))
    x0s = np.zeros((2, 5, 64))
    assert pb._policy_large_shapes(X, U, K, x0s, None, None) == 5
    assert pb._policy_large_shapes(X, U, K, x0s, np.zeros((2, 5, 6, 64)), np.array([[-1.0] * 32, [1.0] * 32])) == 5
    bad = [dict(X=X[:, :6]), dict(U=U[:, :, :31]), dict(K=np.zeros((2, 6, 64, 32))), dict(x0s=np.zeros((2, 64))),
           dict(x0s=np.zeros((2, 0, 64))), dict(x0s=np.zeros((3, 5, 64))), dict(W=np.zeros((2, 5, 7, 64))),
           dict(W=np.zeros((2, 4, 6, 64))), dict(u_lim=np.zeros((32, 2))), dict(u_lim=np.array([[1.0] * 32, [-1.0] * 32]))]
    for kw in bad:
        a = dict(X=X, U=U, K=K, x0s=x0s, W=None, u_lim=None); a.update(kw)
        with pytest.raises(ValueError, match="policy_rollout_large"):
            pb.policy_rollout_large(a["X"], a["U"], a["K"], a["x0s"], W=a["W"], u_lim=a["u_lim"])
    pb.k, pb.n_x, pb.n_u = 15, 60, 30
    assert not pb.is_large
    with pytest.raises(ValueError, match="policy_rollout_large.*n_x = 60"):
        pb.policy_rollout_large(np.zeros((2, 7, 60)), np.zeros((2, 6, 30)), np.zeros((2, 6, 30, 60)), np.zeros((2, 5, 60)))
    pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 21, 12, 4, 252, 84
    with pytest.raises(ValueError, match="policy_rollout_large.*n_x = 252"):
        pb.policy_rollout_large(np.zeros((2, 7, 252)), np.zeros((2, 6, 84)), np.zeros((2, 6, 84, 252)), np.zeros((2, 5, 252)))


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("ns,nc", [(4, 2), (6, 3), (12, 4)])
def test_kernel_resources(table, ns, nc):
    """LDS is sized by the launcher; no more spilled registers and no more scratch than k_policy_rollout of the family, which
    carries the same per-agent model code."""
    r, yard = table[f"k_policy_rollout_large<{ns}, {nc}>"], table[f"k_policy_rollout<{ns}, {nc}>"]
    print({k_: (r[k_], yard[k_]) for k_ in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size")})
    assert r["max_flat_workgroup_size"] == 256 and r["group_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] <= yard["vgpr_spill_count"], (r, yard)
    assert r["private_segment_fixed_size"] <= yard["private_segment_fixed_size"], (r, yard)


def test_the_launcher_stays_inside_the_lds():
    """csrc/policy_large.hpp's layout, recomputed: every served (family, k) fits 160 KiB (the launcher refuses what does not)."""
    worst = 0
    for ns, nc in ((4, 2), (6, 3), (12, 4)):
        for k in range(60 // ns + 1, 21):
            n, m, spw = k * ns, k * nc, 256 // k
            ct, mt = (spw + 15) // 16, (m + 15) // 16 * 16
            ds = (n + 29) // 32 * 32 + 2
            assert ds >= n and ds % 32 == 2
            words = 2 * k * (ns | 1) + 2 * k * (nc | 1) + 16 * ct * ds + 16 * ct * (mt | 1) + 2 * 256 * 3 + 2 * spw * k \
                + 2 * spw * (k * (k - 1) // 2) + 256
            worst = max(worst, 8 * words)
    assert worst <= 160 * 1024, worst
