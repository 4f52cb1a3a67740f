"""Separated random scenarios (csrc/separated_setup.hpp, include/dpilqr_separated_setup.h) without a GPU.

tests/separated_setup_check.cpp -- a stand-alone program with its own main -- is compiled against the header by the host compiler,
with AddressSanitizer and UBSan where the compiler has them, and run directly: it emulates the kernel's threads (per phase: all
read, then all write) and prints the digests / bit patterns and round counts of the records of tests/golden/g12_separated_setup.npz
(written by scripts/make_golden_separated.py from the real reference's util.random_setup(random=False)), which must match.  Then
util.separate_locs against the same fixture, the symbol, the entry's refusals (no device needed), the kernel's code object (no
scratch, no spills, the stated LDS) and the Python refusals."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "g12_separated_setup.npz"
N_ARGS = 11
CAP_RECORD = 66      # the record separated_setup_check.cpp also runs under max_iter = 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def g12():
    return np.load(GOLD)


def _digest(a):
    v = np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)
    w = np.arange(v.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over="ignore"):
        return np.array([v.sum(dtype=np.uint64), (v * w).sum(dtype=np.uint64)], dtype=np.uint64)


def _raw(g, rec):
    """The two raw point sets of a record, as randomize_locs draws them."""
    k, n_d = int(g["k"][rec]), int(g["n_d"][rec])
    np.random.seed(int(g["seed"][rec]))
    return [float(g["var"][rec]) * np.random.uniform(-1, 1, (k, n_d)) for _ in range(2)]


def _rows(g, rec, sets):
    k, n_s, n_d = int(g["k"][rec]), int(g["n_s"][rec]), int(g["n_d"][rec])
    return [np.c_[s, np.zeros((k, n_s - n_d))].reshape(-1, 1) for s in sets]


def _compile(cxx, out, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", str(ROOT / "dpilqr_amd" / "csrc"),
           "-o", str(out), str(ROOT / "tests" / "separated_setup_check.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_host_emulation_of_the_kernel_matches_the_fixture(tmp_path, g12):
    from dpilqr_amd.util import separate_locs
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "separated_setup_check"
    built = _compile(cxx, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0:      # a compiler without the sanitizer runtimes: the same program, plain
        built = _compile(cxx, exe, [])
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    n_rec = len(g12["k"])
    got, rounds = np.zeros_like(g12["digest"]), np.zeros_like(g12["rounds"])
    full = {(r, ai): np.zeros(g12[f"{name}_{r}"].shape, np.uint64) for r in range(n_rec) if int(g12["k"][r]) <= 8
            for ai, name in enumerate(("x0", "xf"))}
    n_full, cap = 0, {}
    for line in run.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        if f[0] == "full":
            full[int(f[1]), int(f[2])][int(f[3])] = np.uint64(int(f[4])); n_full += 1
        elif f[0] == "cap":
            cap[int(f[2])] = (int(f[1]), np.array([int(f[3]), int(f[4])], dtype=np.uint64), int(f[5]))
        else:
            got[int(f[0]), int(f[1])] = [np.uint64(int(f[2])), np.uint64(int(f[3]))]
            rounds[int(f[0]), int(f[1])] = int(f[4])
    assert np.array_equal(got, g12["digest"]), np.argwhere((got != g12["digest"]).any(axis=-1))[:8]
    assert np.array_equal(rounds, g12["rounds"])
    assert full and n_full == sum(v.size for v in full.values())
    for (r, ai), v in full.items():
        assert np.array_equal(v, g12[f"{('x0', 'xf')[ai]}_{r}"].view(np.uint64)), (r, ai)
    # the cap: one round of NumPy's statement, -1, no normalisation
    assert float(g12["energy"][CAP_RECORD]) == 0.0 and (g12["rounds"][CAP_RECORD] > 1).all()
    one = [separate_locs(s, float(g12["rel_dist"][CAP_RECORD]), max_iter=1) for s in _raw(g12, CAP_RECORD)]
    for ai, row in enumerate(_rows(g12, CAP_RECORD, [x for x, _ in one])):
        assert cap[ai][0] == CAP_RECORD and cap[ai][2] == one[ai][1] == -1 and np.array_equal(cap[ai][1], _digest(row))


def test_separate_locs_chained_like_random_setup_equals_the_fixture(g12):
    """util.separate_locs on the raw draws of either set, then normalize_energy: the reference's arrays bit for bit, with the
    fixture's round counts; and util.random_setup(random=False), the host mirror of the branch, gives the same arrays."""
    from dpilqr_amd.util import normalize_energy, random_setup, separate_locs
    seen_k = set()
    for rec in range(len(g12["k"])):
        k, n_s, n_d = int(g12["k"][rec]), int(g12["n_s"][rec]), int(g12["n_d"][rec])
        rel_dist, energy = float(g12["rel_dist"][rec]), float(g12["energy"][rec])
        done = [separate_locs(s, rel_dist) for s in _raw(g12, rec)]
        assert [r for _, r in done] == g12["rounds"][rec].tolist()
        rows = _rows(g12, rec, [x for x, _ in done])
        if energy:
            rows = [normalize_energy(x, [n_s] * k, energy, n_d) for x in rows]
        np.random.seed(int(g12["seed"][rec]))
        host = random_setup(k, n_s, is_rotation=False, rel_dist=rel_dist, var=float(g12["var"][rec]), n_d=n_d, random=False,
                            energy=energy or None)
        for ai, name in enumerate(("x0", "xf")):
            assert np.array_equal(_digest(rows[ai]), g12["digest"][rec, ai]), (rec, name)
            assert np.array_equal(_digest(host[ai]), g12["digest"][rec, ai]), (rec, name)
            if k <= 8:
                assert np.array_equal(rows[ai].ravel().view(np.uint64), g12[f"{name}_{rec}"].view(np.uint64)), (rec, name)
        seen_k.add((k, n_d))
    assert {(2, 2), (3, 3), (64, 2), (65, 2), (129, 2), (130, 3), (256, 2)} <= seen_k
    assert g12["rounds"].min() >= 1 and g12["rounds"].max() >= 3 and g12["rounds"].max() <= 64


def test_separate_locs_quirks():
    from dpilqr_amd.util import separate_locs
    far = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]])
    x, r = separate_locs(far, 3.0)
    assert r == 1 and np.array_equal(x, far) and x is not far      # at least one round, nothing moved, a copy
    # z is ignored: two points apart in z only are on top of one another, and the push, the same for both in x and y, never parts them
    stacked = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 50.0], [9.0, 9.0, 0.0]])
    x, r = separate_locs(stacked, 3.0, max_iter=5)
    assert r == -1 and np.array_equal(x[:2, :2], x[[1, 0], :2]) and x[0, 2] != x[1, 2]
    # a partial round moves the flagged points only, from the old centre
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [100.0, 100.0]])
    x, r = separate_locs(pts, 2.0, max_iter=1)
    c = pts.mean(axis=0)
    assert r == -1 and np.array_equal(x[2], pts[2]) and np.array_equal(x[:2], pts[:2] + 0.1 * 3 * (pts[:2] - c))
    with pytest.raises(ValueError, match="Can't compute pairwise distance for one agent."):
        separate_locs(np.zeros((1, 2)), 3.0)


def test_symbol_is_declared_bound_and_exported(lib):
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    core, ext = strip((ROOT / "include" / "dpilqr_hip.h").read_text()), strip((ROOT / "include" / "dpilqr_separated_setup.h").read_text())
    assert re.search(r'^\s*#\s*include\s+"dpilqr_separated_setup.h"', core, re.M)
    decl = dict(re.findall(r"\bint32_t\s+(dpilqr_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", ext))
    assert sorted(decl) == ["dpilqr_setup_separate"] == sorted(lib.SEPARATED_SIGNATURES)
    others = (set(lib.SIGNATURES) | set(lib.EXT_SIGNATURES) | set(lib.SWARM_SIGNATURES) | set(lib.SWARM_POLICY_SIGNATURES)
              | set(lib.SWARM_ADVANCE_SIGNATURES) | set(lib.ORDER_SIGNATURES) | set(lib.NEAREST_SIGNATURES) | set(lib.SWARM_STUDY_SIGNATURES))
    assert not set(lib.SEPARATED_SIGNATURES) & others
    params = [p.split()[-1].lstrip("*") for p in decl["dpilqr_setup_separate"].split(",")]
    assert params == ["S", "k", "n_s", "n_d", "rel_dist", "energy", "max_iter", "x0", "xf", "n_iter", "stream"]
    assert len(params) == N_ARGS == len(lib.SEPARATED_SIGNATURES["dpilqr_setup_separate"][1])
    fn = lib.load().dpilqr_setup_separate
    assert fn.argtypes == lib.SEPARATED_SIGNATURES["dpilqr_setup_separate"][1] and fn.restype is C.c_int32
    assert [t for t in fn.argtypes[:7]] == [C.c_int32] * 4 + [C.c_double] * 2 + [C.c_int32]
    assert int(re.search(r"#define\s+DPILQR_SETUP_SEPARATE_LDS\s+(\d+)", ext).group(1)) == lib.SETUP_SEPARATE_LDS
    assert int(re.search(r"#define\s+DPILQR_SETUP_SEPARATE_MAX_ITER\s+(\d+)", ext).group(1)) == lib.SETUP_SEPARATE_MAX_ITER == 4096
    # the study's header keeps its single declaration, and the ABI version stays: additive
    study = strip((ROOT / "include" / "dpilqr_swarm_study.h").read_text())
    assert re.findall(r"\bint32_t\s+(dpilqr_[a-z_0-9]+)\s*\(", study) == ["dpilqr_trial_inputs"]
    assert lib.load().dpilqr_abi_version() == 4 == lib.ABI_VERSION


def test_entry_refuses_bad_arguments_before_any_launch(lib):
    L = lib.load()
    P = 1 << 20      # never dereferenced: every call below is refused first
    ok = dict(S=2, k=65, n_s=4, n_d=2, rel_dist=65.0, energy=130.0, max_iter=256, x0=P, xf=P, n_iter=P, stream=None)
    bad = [dict(S=-1), dict(k=1), dict(k=0), dict(k=257), dict(n_d=0), dict(n_d=4, n_s=6), dict(n_d=3, n_s=2), dict(max_iter=0),
           dict(max_iter=-1), dict(max_iter=4097), dict(x0=None), dict(xf=None), dict(n_iter=None), dict(rel_dist=float("nan"))]
    for change in bad:
        args = {**ok, **change}
        assert L.dpilqr_setup_separate(*args.values()) == lib.EINVAL, change
        assert b"setup_separate" in L.dpilqr_last_error(), change
    # S = 0: nothing to launch, whatever the limits of the other arguments allow
    for change in (dict(), dict(k=2), dict(k=256), dict(max_iter=1), dict(max_iter=4096), dict(n_d=3, n_s=3), dict(rel_dist=-1.0),
                   dict(rel_dist=float("inf"))):
        assert L.dpilqr_setup_separate(*{**ok, "S": 0, **change}.values()) == 0, change


def test_code_object_has_no_scratch_no_spills_and_the_stated_lds(lib):
    import sys
    sys.path.insert(0, str(ROOT / "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    rows = [r for r in kernel_resources.resources() if r["demangled"] == "dpilqr::k_setup_separate"]
    assert len(rows) == 1, [r["demangled"] for r in rows]
    r = rows[0]
    assert r["private_segment_fixed_size"] == 0 and r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["group_segment_fixed_size"] == lib.SETUP_SEPARATE_LDS and r["max_flat_workgroup_size"] == 256, r


def test_python_layers_refuse_one_agent_and_name_the_sets_that_did_not_separate(lib, monkeypatch):
    """No device: one agent is refused with the reference's words before anything is drawn; a -1 among the counts read back is a
    ValueError naming seed and set (the counts come from a stand-in for the device call)."""
    import torch
    from dpilqr_amd import analysis, device, util
    words = "Can't compute pairwise distance for one agent."
    with pytest.raises(ValueError, match=words):
        util.random_setup_batch(range(3), 1, 4, 0.5, separated=True)
    with pytest.raises(ValueError, match=words):
        util.random_setup_batch(range(3), 1, 4, 0.5, separated=True, wide=True)
    with pytest.raises(ValueError, match=words):
        analysis.trial_inputs_batch(1, 4, 2, 3, 10.0, 2, [0, 1], separated=True)
    with pytest.raises(ValueError, match=words):
        analysis.trial_inputs(1, 4, 2, 3, 10.0, 2, 0, separated=True)
    with pytest.raises(ValueError, match="2 .. 256"):
        util.random_setup_batch(range(3), 257, 4, 128.5, separated=True)
    with pytest.raises(ValueError, match="return_rounds"):
        util.random_setup_batch(range(3), 5, 4, 2.5, return_rounds=True)

    class _Lib:
        @staticmethod
        def dpilqr_setup_separate(S, k, n_s, n_d, rel_dist, energy, max_iter, x0, xf, n_iter, stream):
            counts = (C.c_int32 * (2 * S)).from_address(n_iter)
            counts[:] = [3, 2, -1, 4, 1, -1][:2 * S]
            return 0

    monkeypatch.setattr(lib, "load", lambda: _Lib)
    monkeypatch.setattr(device, "empty", lambda shape, dtype=torch.float64: torch.empty(shape, dtype=dtype))
    monkeypatch.setattr(device, "stream_handle", lambda: None)
    x = torch.zeros((3, 20), dtype=torch.float64)
    with pytest.raises(ValueError) as e:
        util.separate_setups(x, x.clone(), [11, 12, 40], 5, 4, 2, 5.0, None, max_iter=7, who="random_setup_batch")
    text = str(e.value)
    assert "random_setup_batch" in text and "max_iter=7" in text and "seed 12 (starts)" in text and "seed 40 (goals)" in text
    assert "seed 11" not in text
    rounds = util.separate_setups(x[:1], x[:1].clone(), [11], 5, 4, 2, 5.0, None)
    assert rounds.tolist() == [[3, 2]]
