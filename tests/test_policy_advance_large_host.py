"""The large-cluster receding-horizon advance's host side, without a GPU: the symbol is declared, exported and bound with
dpilqr_policy_advance's arguments; its limits and argument checks answer before any launch (fake, aligned device pointers as
in tests/test_policy_advance_host.py); ProblemBatch.policy_advance_large and solve_rhc_closed_loop(large=True) validate on the
host; the three instantiations of k_policy_advance_large use no scratch; and the cases of tests/policy_large_cases.py are honest
on the prefixes the GPU tests execute (from the CPU reference alone)."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import policy_advance_large_cases as alc
from tests import policy_cases as pc

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test
NAME = "dpilqr_policy_advance_large"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


def _desc(lib, k, ns, nc, B=2, T=10):
    return lib.BatchDesc(B, k, ns, nc, T, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)


_DEFAULT = dict(X=P, U=P, K=P, h=1, scen=None, n_scen=4, L=5, n_d=2, W=None, u_lim=None, x_cur=P, n_done=P, X_exec=P, U_exec=P,
                J_exec=P, min_sep=P, dist_left=P, U_next=P, X_next=P)
_REQUIRED = ("X", "U", "x_cur", "n_done", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left", "U_next", "X_next")


def _call(lib, d, **kw):
    a = dict(_DEFAULT); a.update(kw)
    return getattr(lib.load(), NAME)(C.byref(d), a["X"], a["U"], a["K"], a["h"], a["scen"], a["n_scen"], a["L"], a["n_d"], a["W"],
                                     a["u_lim"], a["x_cur"], a["n_done"], a["X_exec"], a["U_exec"], a["J_exec"], a["min_sep"],
                                     a["dist_left"], a["U_next"], a["X_next"], None)


def test_symbol_is_declared_exported_and_bound(lib):
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    ext = strip((ROOT / "include" / "dpilqr_policy.h").read_text())
    m = re.search(r"\bint32_t\s+" + NAME + r"\s*\(([^)]*)\)\s*;", ext)
    assert m, "not declared in include/dpilqr_policy.h"
    small = re.search(r"\bint32_t\s+dpilqr_policy_advance\s*\(([^)]*)\)\s*;", ext)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(m.group(1)) == norm(small.group(1))      # the argument list of dpilqr_policy_advance
    assert NAME in lib.EXT_SIGNATURES and NAME not in lib.SIGNATURES
    assert lib.EXT_SIGNATURES[NAME] == lib.EXT_SIGNATURES["dpilqr_policy_advance"] and len(lib.EXT_SIGNATURES[NAME][1]) == 21
    assert sorted(set(re.findall(r"\b(dpilqr_[a-z_0-9]+)\s*\(", ext))) == sorted(lib.EXT_SIGNATURES)
    fn = getattr(lib.load(), NAME)
    assert fn.argtypes == lib.EXT_SIGNATURES[NAME][1] and fn.restype is C.c_int32
    assert lib.load().dpilqr_abi_version() == 4      # additive: the ABI version stays


def test_the_header_compiles_as_c(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    state = "double*, int32_t*, double*, double*, double*, double*, double*, double*, double*, void*"
    src = tmp_path / "t.c"
    src.write_text('#include "dpilqr_hip.h"\n'
                   'int32_t (*p)(const dpilqr_batch_desc*, const double*, const double*, const double*, int32_t, const int32_t*, int32_t, '
                   f'int32_t, int32_t, const double*, const double*, {state}) = {NAME};\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_small_clusters_are_the_other_entry_point(lib):
    for k, ns, nc in ((5, 4, 2), (10, 6, 3), (5, 12, 4), (15, 4, 2)):
        assert _call(lib, _desc(lib, k, ns, nc)) == lib.EUNSUPPORTED
        msg = lib.load().dpilqr_last_error().decode()
        assert "policy_advance_large:" in msg and f"n_x={k * ns}" in msg and "60" in msg, msg
        assert re.search(r"\bdpilqr_policy_advance\b(?!_)", msg), msg


def test_beyond_the_served_sizes_is_unsupported_before_any_launch(lib):
    for k, ns, nc in ((21, 12, 4), (21, 4, 2), (41, 6, 3)):      # n_x > 240 or k > 20
        assert _call(lib, _desc(lib, k, ns, nc)) == lib.EUNSUPPORTED
        msg = lib.load().dpilqr_last_error().decode()
        assert "policy_advance_large:" in msg and f"n_x={k * ns}" in msg and "240" in msg and "20" in msg, msg
    # a family that is not served: the five-state one is the only other that can exceed 60 states at k <= 20
    assert _call(lib, _desc(lib, 13, 5, 2)) == lib.EUNSUPPORTED
    msg = lib.load().dpilqr_last_error().decode()
    assert "policy_advance_large:" in msg and "(5, 2) family" in msg and "(4, 2), (6, 3) and (12, 4)" in msg and "240" in msg, msg
    assert _call(lib, _desc(lib, 20, 4, 3)) == lib.EINVAL      # not a model family at all: the descriptor's own check
    # the small entry point keeps its refusal of n_x > 60
    a = dict(_DEFAULT)
    tail = [a[f] for f in ("h", "scen", "n_scen", "L", "n_d", "W", "u_lim", "x_cur", "n_done", "X_exec", "U_exec", "J_exec", "min_sep",
                           "dist_left", "U_next", "X_next")]
    assert lib.load().dpilqr_policy_advance(C.byref(_desc(lib, 16, 4, 2)), P, P, P, *tail, None) == lib.EUNSUPPORTED


def test_bad_arguments_are_einval(lib):
    d = _desc(lib, 16, 4, 2)                # T = 10, B = 2
    L = lib.load()
    for name in _REQUIRED:
        assert _call(lib, d, **{name: None}) == lib.EINVAL, name
        assert b"policy_advance_large" in L.dpilqr_last_error() and b"NULL" in L.dpilqr_last_error(), name
    for kw in (dict(h=0), dict(h=11), dict(h=-1), dict(L=0), dict(n_d=0), dict(n_d=5), dict(n_scen=1)):
        assert _call(lib, d, **kw) == lib.EINVAL, kw
        key = next(iter(kw))
        assert (key + "=").encode() in L.dpilqr_last_error(), (kw, L.dpilqr_last_error())
    for name in tuple(f for f in _REQUIRED if f != "n_done") + ("K", "W", "u_lim"):
        assert _call(lib, d, **{name: P + 4}) == lib.EINVAL, name
        assert b"aligned" in L.dpilqr_last_error(), name
    assert _call(lib, d, scen=P + 2) == lib.EINVAL and _call(lib, d, n_done=P + 2) == lib.EINVAL      # int32 words
    # EINVAL comes first: bad arguments on a size that is not served either
    assert _call(lib, _desc(lib, 5, 4, 2), h=0) == lib.EINVAL
    bad = lib.BatchDesc(2, 16, 4, 2, 10, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P + 4, 0, P, 0, P, 0, P, 0, P, 0)      # a misaligned xf
    assert _call(lib, bad) == lib.EINVAL
    assert getattr(L, NAME)(None, P, P, P, 1, None, 4, 5, 2, None, None, P, P, P, P, P, P, P, P, P, None) == lib.EINVAL


def test_an_empty_batch_launches_nothing(lib):
    """B = 0 is DPILQR_OK: with the fake pointers of this file a launch would not return it."""
    for k, ns, nc in ((16, 4, 2), (11, 6, 3), (20, 12, 4)):
        assert _call(lib, _desc(lib, k, ns, nc, B=0), n_scen=0) == lib.OK
        assert _call(lib, _desc(lib, k, ns, nc, B=0), K=None) == lib.OK      # open loop


def _host_batch():
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 2, 6, 16, 4, 2, 64, 32
    return pb


def _host_state(S=4, L=5, T=6, k=16, n=64, m=32, **over):
    import torch
    f64 = torch.float64
    st = dict(x_cur=torch.zeros((S, n), dtype=f64), n_done=torch.zeros((S,), dtype=torch.int32), X_exec=torch.zeros((S, L + 1, n), dtype=f64),
              U_exec=torch.zeros((S, L, m), dtype=f64), J_exec=torch.zeros((S,), dtype=f64), min_sep=torch.zeros((S,), dtype=f64),
              dist_left=torch.zeros((S, k), dtype=f64), U_next=torch.zeros((S, T, m), dtype=f64), X_next=torch.zeros((S, T + 1, n), dtype=f64))
    st.update(over)
    return st


def test_policy_advance_large_validates_on_the_host():
    """Every error is a ValueError naming policy_advance_large, raised before the device is touched: the batch object has no
    device state, the state lives on the host.  The shapes are tests/test_policy_advance_host.py's, scaled to n_x = 64."""
    import torch
    pb = _host_batch()
    X, U, K = np.zeros((2, 7, 64)), np.zeros((2, 6, 32)), np.zeros((2, 6, 32, 64))
    ok = dict(X=X, U=U, K=K, h=2, state=_host_state(), scen=None, W=None, u_lim=None, n_d=2)

    def shapes(**kw):
        a = dict(ok); a.update(kw)
        return pb._advance_shapes("policy_advance_large", a["X"], a["h"], a["state"], a["scen"], a["W"], a["u_lim"], a["n_d"],
                                  (("U", a["U"], (2, 6, 32)), ("K", a["K"], (2, 6, 32, 64))), large=True)

    assert shapes() == (4, 5)
    assert shapes(K=None, scen=[3, 1], W=np.zeros((4, 5, 64)), u_lim=np.array([[-1.0] * 32, [1.0] * 32]), h=6, n_d=4) == (4, 5)
    assert shapes(scen=torch.tensor([3, 1], dtype=torch.int32)) == (4, 5)
    bad = [dict(X=X[:, :6]), dict(U=U[:, :, :31]), dict(K=np.zeros((2, 6, 64, 32))), dict(h=0), dict(h=7), dict(h=1.5), dict(n_d=0), dict(n_d=5),
           dict(scen=[0]), dict(scen=[0, 4]), dict(scen=[-1, 0]), dict(scen=[1, 1]), dict(scen=np.array([0.0, 1.0])),
           dict(W=np.zeros((4, 6, 64))), dict(W=np.zeros((2, 5, 64))), dict(u_lim=np.zeros((32, 2))),
           dict(u_lim=np.array([[1.0] * 32, [-1.0] * 32])), dict(state={}), dict(state=_host_state(S=1)),
           dict(state=_host_state(n_done=torch.zeros((4,), dtype=torch.int64))), dict(state=_host_state(X_exec=torch.zeros((4, 5, 64), dtype=torch.float64))),
           dict(state=_host_state(U_next=torch.zeros((4, 5, 32), dtype=torch.float64))), dict(state=_host_state(min_sep=torch.zeros((4,), dtype=torch.float32))),
           dict(state=_host_state(X_next=torch.zeros((4, 64, 7), dtype=torch.float64).transpose(1, 2)))]
    for kw in bad:
        with pytest.raises(ValueError, match="policy_advance_large"):
            shapes(**kw)
    # through the public method, still without a device
    with pytest.raises(ValueError, match="policy_advance_large: h = 9"):
        pb.policy_advance_large(X, U, K, 9, _host_state())
    with pytest.raises(ValueError, match="policy_advance_large: K has shape"):
        pb.policy_advance_large(X, U, np.zeros((2, 6, 64, 32)), 1, _host_state())
    pb.k, pb.n_x, pb.n_u = 15, 60, 30
    with pytest.raises(ValueError, match="policy_advance_large.*n_x = 60.*policy_advance"):
        pb.policy_advance_large(np.zeros((2, 7, 60)), np.zeros((2, 6, 30)), None, 1, _host_state(n=60, m=30, k=15))
    pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 21, 12, 4, 252, 84
    with pytest.raises(ValueError, match="policy_advance_large.*n_x = 252"):
        pb.policy_advance_large(np.zeros((2, 7, 252)), np.zeros((2, 6, 84)), None, 1, _host_state(n=252, m=84, k=21))
    pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 21, 4, 2, 84, 42
    with pytest.raises(ValueError, match="policy_advance_large.*k = 21"):
        pb.policy_advance_large(np.zeros((2, 7, 84)), np.zeros((2, 6, 42)), None, 1, _host_state(n=84, m=42, k=21))
    pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 20, 5, 2, 100, 40
    with pytest.raises(ValueError, match=r"policy_advance_large.*\(5, 2\)"):
        pb.policy_advance_large(np.zeros((2, 7, 100)), np.zeros((2, 6, 40)), None, 1, _host_state(n=100, m=40, k=20))
    # policy_advance keeps its own message for the same batch
    pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 16, 4, 2, 64, 32
    with pytest.raises(ValueError, match="policy_advance serves clusters up to n_x = 60"):
        pb.policy_advance(X, U, None, 1, _host_state())


def _problem(k):
    import dpilqr_amd as dp
    dp._reset_ids()
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(np.zeros(4), np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k)))


def test_the_loop_validates_on_the_host():
    import dpilqr_amd as dp
    big = _problem(16)
    x0 = np.zeros((2, 64))
    with pytest.raises(ValueError, match="n_x = 60.*large=True"):      # the default is unchanged, with a hint
        dp.solve_rhc_closed_loop(big, x0, 10, dist_converge=0.1, max_steps=4)
    with pytest.raises(ValueError, match="large=True.*distributed loop.*not built"):
        dp.solve_rhc_closed_loop(big, x0, 10, radius=1.0, dist_converge=0.1, max_steps=4, centralized=False, large=True)
    with pytest.raises(ValueError, match="large=True.*k <= 20.*k = 21"):
        dp.solve_rhc_closed_loop(_problem(21), np.zeros((2, 84)), 10, dist_converge=0.1, max_steps=4, large=True)
    with pytest.raises(ValueError, match="large=True.*n_x <= 240.*n_x = 244"):
        dp.solve_rhc_closed_loop(_problem(61), np.zeros((2, 244)), 10, dist_converge=0.1, max_steps=4, large=True)
    # the checks that follow are the loop's own, reached with large=True too
    with pytest.raises(ValueError, match="max_steps"):
        dp.solve_rhc_closed_loop(big, x0, 10, dist_converge=0.1, large=True)
    with pytest.raises(ValueError, match="step_size"):
        dp.solve_rhc_closed_loop(big, x0, 10, dist_converge=0.1, max_steps=4, step_size=11, large=True)
    # a small problem takes the existing route whatever `large` says: its distributed loop still asks for the radius
    with pytest.raises(ValueError, match="radius"):
        dp.solve_rhc_closed_loop(_problem(3), np.zeros((2, 12)), 10, dist_converge=0.1, max_steps=4, centralized=False, large=True)


# ---------------------------------------------------------------------------------------------- the built kernels
@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("ns,nc", [(4, 2), (6, 3), (12, 4)])
def test_advance_large_kernels_use_no_scratch(table, ns, nc):
    r = table[f"k_policy_advance_large<{ns}, {nc}>"]
    print({k_: r[k_] for k_ in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size")})
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256 and r["group_segment_fixed_size"] == 0, r      # LDS is sized by the launcher


def test_the_lds_fits_at_every_served_size():
    """AdvanceLargeLds of csrc/policy_advance_large.hpp, restated: every served (family, k) stays below the 64 KiB a kernel may
    use without asking, far below the 160 KiB of a workgroup."""
    worst = 0
    for ns, nc in ((4, 2), (6, 3), (12, 4)):
        for k in range(60 // ns + 1, 21):
            n, m = k * ns, k * nc
            mt, ds = (m + 15) // 16 * 16, (n + 29) // 32 * 32 + 2
            assert ds >= n and ds % 32 == 2
            words = 16 * ds + 16 * (mt | 1) + 2 * k * 3 + 2 * k + 2 * (k * (k - 1) // 2) + k
            worst = max(worst, 8 * ((words + 1) & ~1))
    assert worst <= 64 * 1024, worst


# ---------------------------------------------------------------------------------------------- the cases, on a prefix
@pytest.mark.parametrize("case", alc.CASES, ids=alc.IDS)
def test_case_conditions(case):
    """From the CPU reference alone, for every executed length the GPU tests use: the limits bind somewhere and not everywhere,
    a sample of the W variant is inside the radius within the prefix, the unchecked share stays inside policy_cases' cap."""
    ref = alc.case_ref(case)
    assert alc.T in alc.HS[case.id] and set(alc.HS[case.id]) <= {1, 3, alc.T}
    for h in alc.HS[case.id]:
        f = alc.prefix_figures(case, ref, h)
        print(f"{case.id} h={h}: clamped {f['clamped']:.4f} near {f['near']:.4f} unchecked " +
              " ".join(f"{v} {u:.4f}" for v, u in f["unchecked"].items()))
        assert 0.0 < f["clamped"] < 1.0, (h, f)
        assert f["near"] > 0.0, (h, f)
        assert all(u <= pc.MAX_UNCHECKED for u in f["unchecked"].values()), (h, f)
