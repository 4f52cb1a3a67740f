"""The closed-loop ensemble rollout's host side, without a GPU: the symbol is declared and exported, its argument checks answer
before any launch (fake, aligned device pointers in the style of tests/test_abi.py), perturbed_starts is the loop over
perturb_state it documents, and ProblemBatch.policy_rollout validates shapes on the host."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


def _desc(lib, k, ns, nc, B=2, T=10):
    return lib.BatchDesc(B, k, ns, nc, T, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)


def _call(lib, d, X=P, U=P, K=P, S=4, x0s=P, W=None, u_lim=None, Xs=None, Us=None, J=P, sep=None, goal=None):
    return lib.load().dpilqr_policy_rollout(C.byref(d), X, U, K, S, x0s, W, u_lim, Xs, Us, J, sep, goal, None)


def test_symbol_is_declared_and_exported(lib):
    """include/dpilqr_hip.h declares it for every includer through its extension header include/dpilqr_policy.h; the binding
    and the library agree with that header, as tests/test_abi.py holds the core symbols to dpilqr_hip.h."""
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    core, ext = strip((ROOT / "include" / "dpilqr_hip.h").read_text()), strip((ROOT / "include" / "dpilqr_policy.h").read_text())
    assert re.search(r'^\s*#\s*include\s+"dpilqr_policy.h"', core, re.M)
    assert re.search(r"\bint32_t\s+dpilqr_policy_rollout\s*\(", ext)
    assert sorted(set(re.findall(r"\b(dpilqr_[a-z_0-9]+)\s*\(", ext))) == sorted(lib.EXT_SIGNATURES)
    assert not set(lib.EXT_SIGNATURES) & set(lib.SIGNATURES)
    assert hasattr(lib.load(), "dpilqr_policy_rollout")
    assert lib.load().dpilqr_policy_rollout.argtypes == lib.EXT_SIGNATURES["dpilqr_policy_rollout"][1]
    assert lib.load().dpilqr_abi_version() == 4      # additive: the ABI version stays


def test_the_header_compiles_as_c(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "dpilqr_hip.h"\nint32_t (*p)(const dpilqr_batch_desc*, const double*, const double*, const double*, int32_t, const double*, '
                   'const double*, const double*, double*, double*, double*, double*, double*, void*) = dpilqr_policy_rollout;\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


def test_beyond_sixty_states_is_unsupported_before_any_launch(lib):
    for k, ns, nc in ((16, 4, 2), (11, 6, 3), (6, 12, 4), (21, 3, 2)):
        assert _call(lib, _desc(lib, k, ns, nc)) == lib.EUNSUPPORTED
        msg = lib.load().dpilqr_last_error().decode()
        assert "policy_rollout" in msg and f"n_x={k * ns}" in msg and "60" in msg, msg


def test_bad_arguments_are_einval(lib):
    d = _desc(lib, 5, 4, 2)
    L = lib.load()
    assert _call(lib, d, X=None) == lib.EINVAL and b"NULL" in L.dpilqr_last_error()
    assert _call(lib, d, x0s=None) == lib.EINVAL and b"NULL" in L.dpilqr_last_error()
    assert _call(lib, d, U=None) == lib.EINVAL and _call(lib, d, K=None) == lib.EINVAL and _call(lib, d, J=None) == lib.EINVAL
    assert _call(lib, d, S=0) == lib.EINVAL and b"n_samples=0" in L.dpilqr_last_error()
    assert _call(lib, d, S=-3) == lib.EINVAL
    for name in ("X", "U", "K", "x0s", "W", "u_lim", "Xs", "Us", "J", "sep", "goal"):      # check_desc's alignment rule
        assert _call(lib, d, **{name: P + 4}) == lib.EINVAL, name
        assert b"aligned" in L.dpilqr_last_error(), name
    assert L.dpilqr_policy_rollout(None, P, P, P, 1, P, None, None, None, None, P, None, None, None) == lib.EINVAL
    bad = lib.BatchDesc(2, 5, 4, 2, 10, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P + 4, 0, P, 0, P, 0, P, 0, P, 0)      # a misaligned xf
    assert _call(lib, bad) == lib.EINVAL


def test_perturbed_starts_is_the_loop_over_perturb_state():
    from dpilqr_amd.util import perturb_state, perturbed_starts
    x0 = np.arange(12, dtype=np.float64) * 0.25 - 1.0
    for dims, n_d, var, seed in (([4] * 3, 2, 0.5, 7), ([6] * 2, 3, 0.1, 0), ([12], 3, 2.0, 123)):
        got = perturbed_starts(x0, dims, 9, n_d=n_d, var=var, seed=seed)
        np.random.seed(seed)
        want = np.stack([perturb_state(x0, dims, n_d=n_d, var=var) for _ in range(9)])
        assert got.shape == (9, 12) and got.dtype == np.float64
        assert np.array_equal(got, want)
        assert not np.array_equal(got[0], got[1])
        moved = np.array([(i % dims[0]) < n_d for i in range(12)])      # positions only
        assert np.array_equal(got[:, ~moved], np.tile(x0[~moved], (9, 1))) and (got[:, moved] != x0[moved]).all()
    # a column vector start, as random_setup returns it; seed=None continues the stream
    np.random.seed(3)
    a = perturbed_starts(x0.reshape(-1, 1), [4] * 3, 2)
    b = perturbed_starts(x0, [4] * 3, 2)
    np.random.seed(3)
    assert np.array_equal(np.vstack([a, b]), perturbed_starts(x0, [4] * 3, 4))
    import dpilqr_amd
    assert dpilqr_amd.perturbed_starts is perturbed_starts


def test_policy_rollout_validates_shapes_on_the_host():
    """Every shape error is raised before the device is touched: the batch object here has no device state at all."""
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 2, 6, 3, 4, 2, 12, 6
    X, U, K = np.zeros((2, 7, 12)), np.zeros((2, 6, 6)), np.zeros((2, 6, 6, 12))
    x0s = np.zeros((2, 5, 12))
    assert pb._policy_shapes(X, U, K, x0s, None, None) == 5
    assert pb._policy_shapes(X, U, K, x0s, np.zeros((2, 5, 6, 12)), np.array([[-1.0] * 6, [1.0] * 6])) == 5
    bad = [dict(X=X[:, :6]), dict(U=U[:, :, :5]), dict(K=np.zeros((2, 6, 12, 6))), dict(x0s=np.zeros((2, 12))),
           dict(x0s=np.zeros((2, 0, 12))), dict(x0s=np.zeros((3, 5, 12))), dict(W=np.zeros((2, 5, 7, 12))),
           dict(W=np.zeros((2, 4, 6, 12))), dict(u_lim=np.zeros((6, 2))), dict(u_lim=np.array([[1.0] * 6, [-1.0] * 6]))]
    for kw in bad:
        a = dict(X=X, U=U, K=K, x0s=x0s, W=None, u_lim=None); a.update(kw)
        with pytest.raises(ValueError, match="policy_rollout"):
            pb.policy_rollout(a["X"], a["U"], a["K"], a["x0s"], W=a["W"], u_lim=a["u_lim"])
    pb.k, pb.n_x, pb.n_u = 16, 64, 32
    with pytest.raises(ValueError, match="n_x = 60"):
        pb.policy_rollout(np.zeros((2, 7, 64)), np.zeros((2, 6, 32)), np.zeros((2, 6, 32, 64)), np.zeros((2, 5, 64)))


def test_closed_loop_refuses_host_plugins():
    import dpilqr_amd as dp

    class HostModel(dp.DynamicalModel):
        def __init__(self):
            super().__init__(4, 2, 0.1)

        def f(self, x, u):
            return np.zeros(4)

        def linearize(self, x, u):
            return np.eye(4), np.zeros((4, 2))

    dp._reset_ids()
    cost = dp.GameCost([dp.ReferenceCost(np.zeros(4), np.eye(4), np.eye(2), np.eye(4), 0)], dp.ProximityCost([4], 0.5, [2]))
    sol = dp.ilqrSolver(dp.ilqrProblem(HostModel(), cost), 5)
    with pytest.raises(NotImplementedError, match="host plugins"):
        sol.closed_loop(np.zeros((6, 4)), np.zeros((5, 2)), np.zeros((3, 4)))
