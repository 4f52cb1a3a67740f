"""The receding-horizon advance's host side, without a GPU: both symbols are declared, bound and exported; their argument
checks answer before any launch (fake, aligned device pointers in the style of tests/test_policy_host.py);
ProblemBatch.policy_advance / policy_advance_dec and solve_rhc_closed_loop validate on the host; the built kernels keep their
registers out of scratch; and the cases of tests/policy_cases.py are honest on the prefixes the GPU tests execute."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import policy_advance_cases as ac
from tests import policy_cases as pc

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced by the checks under test
NAMES = ("dpilqr_policy_advance", "dpilqr_policy_advance_dec")


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


def _call(lib, d, dec=False, kc_max=1, bits=P, **kw):
    a = dict(_DEFAULT); a.update(kw)
    tail = (a["h"], a["scen"], a["n_scen"], a["L"], a["n_d"], a["W"], a["u_lim"], a["x_cur"], a["n_done"], a["X_exec"], a["U_exec"],
            a["J_exec"], a["min_sep"], a["dist_left"], a["U_next"], a["X_next"], None)
    if dec:
        return lib.load().dpilqr_policy_advance_dec(C.byref(d), a["X"], a["U"], a["K"], kc_max, bits, *tail)
    return lib.load().dpilqr_policy_advance(C.byref(d), a["X"], a["U"], a["K"], *tail)


def test_symbols_are_declared_bound_and_exported(lib):
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    ext = strip((ROOT / "include" / "dpilqr_policy.h").read_text())
    for name in NAMES:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", ext), name
        assert name in lib.EXT_SIGNATURES and name not in lib.SIGNATURES
        assert getattr(lib.load(), name).argtypes == lib.EXT_SIGNATURES[name][1]
    assert len(lib.EXT_SIGNATURES[NAMES[0]][1]) == 21 and len(lib.EXT_SIGNATURES[NAMES[1]][1]) == 23
    assert sorted(set(re.findall(r"\b(dpilqr_[a-z_0-9]+)\s*\(", ext))) == sorted(lib.EXT_SIGNATURES)
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
                   f'int32_t, int32_t, const double*, const double*, {state}) = dpilqr_policy_advance;\n'
                   'int32_t (*q)(const dpilqr_batch_desc*, const double*, const double*, const double*, int32_t, const uint64_t*, int32_t, '
                   f'const int32_t*, int32_t, int32_t, int32_t, const double*, const double*, {state}) = dpilqr_policy_advance_dec;\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)], check=True)


@pytest.mark.parametrize("dec", [False, True])
def test_beyond_the_range_is_unsupported_before_any_launch(lib, dec):
    who = "policy_advance_dec" if dec else "policy_advance"
    for k, ns, nc in ((16, 4, 2), (11, 6, 3), (6, 12, 4), (21, 3, 2)):
        assert _call(lib, _desc(lib, k, ns, nc), dec=dec) == lib.EUNSUPPORTED
        msg = lib.load().dpilqr_last_error().decode()
        assert who + ":" in msg and f"n_x={k * ns}" in msg and "60" in msg, msg
    if dec:
        for kc_max in (0, 6):
            assert _call(lib, _desc(lib, 5, 4, 2), dec=True, kc_max=kc_max) == lib.EUNSUPPORTED
            assert b"kc_max" in lib.load().dpilqr_last_error()


@pytest.mark.parametrize("dec", [False, True])
def test_bad_arguments_are_einval(lib, dec):
    d = _desc(lib, 5, 4, 2)                # T = 10, B = 2
    L = lib.load()
    for name in _REQUIRED:
        assert _call(lib, d, dec=dec, **{name: None}) == lib.EINVAL, name
        assert b"NULL" in L.dpilqr_last_error(), name
    for kw in (dict(h=0), dict(h=11), dict(h=-1), dict(L=0), dict(n_d=0), dict(n_d=5), dict(n_scen=1)):
        assert _call(lib, d, dec=dec, **kw) == lib.EINVAL, kw
        key = next(iter(kw))
        assert (key + "=").encode() in L.dpilqr_last_error(), (kw, L.dpilqr_last_error())
    for name in tuple(f for f in _REQUIRED if f != "n_done") + ("K", "W", "u_lim"):      # the alignment rule of the sibling entries
        assert _call(lib, d, dec=dec, **{name: P + 4}) == lib.EINVAL, name
        assert b"aligned" in L.dpilqr_last_error(), name
    assert _call(lib, d, dec=dec, scen=P + 2) == lib.EINVAL and _call(lib, d, dec=dec, n_done=P + 2) == lib.EINVAL      # int32 words
    if dec:
        assert _call(lib, d, dec=True, bits=None) == lib.EINVAL and _call(lib, d, dec=True, bits=P + 4) == lib.EINVAL
    bad = lib.BatchDesc(2, 5, 4, 2, 10, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P + 4, 0, P, 0, P, 0, P, 0, P, 0)      # a misaligned xf
    assert _call(lib, bad, dec=dec) == lib.EINVAL


@pytest.mark.parametrize("dec", [False, True])
def test_an_empty_batch_launches_nothing(lib, dec):
    """B = 0 is DPILQR_OK: with the fake pointers of this file a launch would not return it."""
    assert _call(lib, _desc(lib, 5, 4, 2, B=0), dec=dec, n_scen=0) == lib.OK
    assert _call(lib, _desc(lib, 5, 4, 2, B=0), dec=dec, K=None, bits=None) == lib.OK      # open loop: no gains, no masks


def _host_batch():
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = 2, 6, 3, 4, 2, 12, 6
    return pb


def _host_state(S=4, L=5, T=6, k=3, n=12, m=6, **over):
    import torch
    f64 = torch.float64
    st = dict(x_cur=torch.zeros((S, n), dtype=f64), n_done=torch.zeros((S,), dtype=torch.int32), X_exec=torch.zeros((S, L + 1, n), dtype=f64),
              U_exec=torch.zeros((S, L, m), dtype=f64), J_exec=torch.zeros((S,), dtype=f64), min_sep=torch.zeros((S,), dtype=f64),
              dist_left=torch.zeros((S, k), dtype=f64), U_next=torch.zeros((S, T, m), dtype=f64), X_next=torch.zeros((S, T + 1, n), dtype=f64))
    st.update(over)
    return st


def test_policy_advance_validates_on_the_host():
    """Every error is raised before the device is touched: the batch object has no device state, the state lives on the host."""
    import torch
    pb = _host_batch()
    X, U, K = np.zeros((2, 7, 12)), np.zeros((2, 6, 6)), np.zeros((2, 6, 6, 12))
    ok = dict(X=X, U=U, K=K, h=2, state=_host_state(), scen=None, W=None, u_lim=None, n_d=2)

    def shapes(**kw):
        a = dict(ok); a.update(kw)
        return pb._advance_shapes("policy_advance", a["X"], a["h"], a["state"], a["scen"], a["W"], a["u_lim"], a["n_d"],
                                  (("U", a["U"], (2, 6, 6)), ("K", a["K"], (2, 6, 6, 12))))

    assert shapes() == (4, 5)
    assert shapes(K=None, scen=[3, 1], W=np.zeros((4, 5, 12)), u_lim=np.array([[-1.0] * 6, [1.0] * 6]), h=6, n_d=4) == (4, 5)
    assert shapes(scen=torch.tensor([3, 1], dtype=torch.int32)) == (4, 5)
    bad = [dict(X=X[:, :6]), dict(U=U[:, :, :5]), dict(K=np.zeros((2, 6, 12, 6))), dict(h=0), dict(h=7), dict(h=1.5), dict(n_d=0), dict(n_d=5),
           dict(scen=[0]), dict(scen=[0, 4]), dict(scen=[-1, 0]), dict(scen=[1, 1]), dict(scen=np.array([0.0, 1.0])),
           dict(W=np.zeros((4, 6, 12))), dict(W=np.zeros((2, 5, 12))), dict(u_lim=np.zeros((6, 2))),
           dict(u_lim=np.array([[1.0] * 6, [-1.0] * 6])), dict(state={}), dict(state=_host_state(S=1)),
           dict(state=_host_state(n_done=torch.zeros((4,), dtype=torch.int64))), dict(state=_host_state(X_exec=torch.zeros((4, 5, 12), dtype=torch.float64))),
           dict(state=_host_state(U_next=torch.zeros((4, 5, 6), dtype=torch.float64))), dict(state=_host_state(min_sep=torch.zeros((4,), dtype=torch.float32))),
           dict(state=_host_state(X_next=torch.zeros((4, 12, 7), dtype=torch.float64).transpose(1, 2)))]
    for kw in bad:
        with pytest.raises(ValueError, match="policy_advance"):
            shapes(**kw)
    # through the public methods, still without a device
    with pytest.raises(ValueError, match="policy_advance: h = 9"):
        pb.policy_advance(X, U, K, 9, _host_state())
    with pytest.raises(ValueError, match="policy_advance_dec: Kc has shape"):
        pb.policy_advance_dec(X, U, np.zeros((2, 6, 3, 2, 5)), np.full((2, 3), 7), 1, _host_state())
    with pytest.raises(ValueError, match="policy_advance_dec: nbr_bits has shape"):
        pb.policy_advance_dec(X, U, np.zeros((2, 6, 3, 2, 8)), np.full((3, 3), 7), 1, _host_state())
    with pytest.raises(ValueError, match="policy_advance_dec: a neighbourhood mask lacks its agent's own bit"):
        pb.policy_advance_dec(X, U, np.zeros((2, 6, 3, 2, 8)), np.full((2, 3), 1), 1, _host_state())
    with pytest.raises(ValueError, match="policy_advance_dec: a neighbourhood mask has 3 members"):
        pb.policy_advance_dec(X, U, np.zeros((2, 6, 3, 2, 8)), np.full((2, 3), 7), 1, _host_state())
    pb.k, pb.n_x, pb.n_u = 16, 64, 32
    with pytest.raises(ValueError, match="n_x = 60"):
        pb.policy_advance(np.zeros((2, 7, 64)), np.zeros((2, 6, 32)), None, 1, _host_state(n=64, m=32, k=16))


def _problem(k=3, ns=4):
    import dpilqr_amd as dp
    dp._reset_ids()
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(np.zeros(4), np.eye(4), np.eye(2), 100.0 * np.eye(4), i) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([4] * k, 0.5, [2] * k)))


def test_the_loop_validates_on_the_host():
    import dpilqr_amd as dp
    assert dp.solve_rhc_closed_loop is dp.distributed.solve_rhc_closed_loop
    prob = _problem()
    x0 = np.zeros((2, 12))
    with pytest.raises(ValueError, match="convergence cost or distance"):
        dp.solve_rhc_closed_loop(prob, x0, 10, max_steps=4)
    with pytest.raises(ValueError, match="convergence cost or distance"):
        dp.solve_rhc_closed_loop(prob, x0, 10, max_steps=4, dist_converge=0.1, J_converge=1.0)
    with pytest.raises(ValueError, match="max_steps"):
        dp.solve_rhc_closed_loop(prob, x0, 10, dist_converge=0.1)
    with pytest.raises(ValueError, match="max_steps"):
        dp.solve_rhc_closed_loop(prob, x0, 10, dist_converge=0.1, max_steps=4, W=np.zeros((2, 5, 12)))
    with pytest.raises(ValueError, match="W has shape"):
        dp.solve_rhc_closed_loop(prob, x0, 10, dist_converge=0.1, W=np.zeros((3, 5, 12)))
    with pytest.raises(ValueError, match="step_size"):
        dp.solve_rhc_closed_loop(prob, x0, 10, dist_converge=0.1, max_steps=4, step_size=11)
    with pytest.raises(ValueError, match="radius"):
        dp.solve_rhc_closed_loop(prob, x0, 10, dist_converge=0.1, max_steps=4, centralized=False)
    big = _problem(k=16)
    with pytest.raises(ValueError, match="n_x = 60"):
        dp.solve_rhc_closed_loop(big, np.zeros((2, 64)), 10, dist_converge=0.1, max_steps=4)

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
        dp.solve_rhc_closed_loop(dp.ilqrProblem(HostModel(), cost), np.zeros((1, 4)), 5, dist_converge=0.1, max_steps=3)


# ---------------------------------------------------------------------------------------------- the built kernels
@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    return {r["demangled"]: r for r in kernel_resources.resources()}


@pytest.mark.parametrize("kern", ["k_policy_advance", "k_policy_advance_dec"])
@pytest.mark.parametrize("ns,nc", [(3, 2), (4, 2), (5, 2), (6, 3)])
def test_advance_kernels_do_not_spill(table, kern, ns, nc):
    r = table[f"{kern}<{ns}, {nc}>"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256 and r["group_segment_fixed_size"] == 0, r      # LDS is sized by the launcher


@pytest.mark.parametrize("kern", ["k_policy_advance", "k_policy_advance_dec"])
def test_twelve_state_advance_kernel_against_the_rollout(table, kern):
    r, yard = table[f"{kern}<12, 4>"], table["k_policy_rollout<12, 4>"]
    assert r["private_segment_fixed_size"] <= yard["private_segment_fixed_size"], (r, yard)
    assert r["vgpr_spill_count"] <= yard["vgpr_spill_count"], (r, yard)
    assert r["max_flat_workgroup_size"] == 256


def test_the_lds_fits_at_every_family_limit():
    """AdvanceLds of csrc/policy_advance.hpp, restated: the largest allocation of every family stays below 160 KiB."""
    def lds_bytes(ns, k):
        ipw, as_, np1 = 256 // k, ns | 1, max(k * (k - 1) // 2, 1)
        words = 4 * ipw * k * as_ + 2 * ipw * k + 2 * ipw * np1 + ipw * k + ipw
        return 8 * ((words + 1) & ~1)
    for ns in (3, 4, 5, 6, 12):
        worst = max(lds_bytes(ns, k) for k in range(1, min(20, 60 // ns) + 1))
        assert worst <= 160 * 1024, (ns, worst)


# ---------------------------------------------------------------------------------------------- the cases, on a prefix
@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_the_cases_are_honest_on_a_prefix(case):
    ref = pc.case_ref(case)
    f3, f1 = ac.prefix_figures(case, ref, 3), ac.prefix_figures(case, ref, 1)
    print(case.id, "h=3", f3, "h=1", f1)
    assert 0.10 <= f3["clamped"] <= 0.90, f3
    assert 0.0 < f1["clamped"] < 1.0, f1
    if case.k >= 2:
        assert f3["near"] >= 0.10, f3
    assert all(u == 0.0 for u in f3["unchecked"].values()), f3      # no sample is left without a bound
