"""The study's input generator (csrc/trial_inputs.hpp, include/dpilqr_swarm_study.h) without a GPU.

tests/trial_inputs_check.cpp -- a stand-alone program with its own main -- is compiled against the header by the host compiler,
with AddressSanitizer and UBSan where the compiler has them, and run directly: it emulates the kernel's lanes (per twist phase: all
read, then all write) and prints the digests / bit patterns of the cases of tests/golden/g11_trial_inputs_wide.npz (written by
scripts/make_golden_wide.py from the real reference's util.random_setup), which must match: a wrong phase boundary, a pair
straddling a twist or a wrong split of NumPy's pairwise sum shows here.  Then the symbols, the entry's refusals (no device needed)
and the kernel's code object (no scratch, no spills, the stated LDS)."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "g11_trial_inputs_wide.npz"
N_ARGS = 17


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


def _compile(cxx, out, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", str(ROOT / "dpilqr_amd" / "csrc"),
           "-o", str(out), str(ROOT / "tests" / "trial_inputs_check.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_host_emulation_of_the_kernel_matches_the_fixture(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "trial_inputs_check"
    built = _compile(cxx, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0:      # a compiler without the sanitizer runtimes: the same program, plain
        built = _compile(cxx, exe, [])
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    g = np.load(GOLD)
    seeds = list(g["seeds"])
    got = np.zeros_like(g["digest"])
    small = {0: np.zeros(g["small_x0"].shape, np.uint64), 1: np.zeros(g["small_xf"].shape, np.uint64),
             2: np.zeros(g["small_Ua"].shape, np.uint64).reshape(len(g["small_seeds"]), -1),
             3: np.zeros(g["small_Ub"].shape, np.uint64).reshape(len(g["small_seeds"]), -1)}
    n_small = 0
    for line in run.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        if f[0] == "small":
            small[int(f[2])][int(f[1]), int(f[3])] = np.uint64(int(f[4])); n_small += 1
        else:
            got[int(f[0]), int(f[1]), seeds.index(int(f[2])), int(f[3])] = [np.uint64(int(f[4])), np.uint64(int(f[5]))]
    assert np.array_equal(got, g["digest"]), np.argwhere((got != g["digest"]).any(axis=-1))[:8]
    assert n_small == sum(v.size for v in small.values())
    for ai, name in enumerate(("small_x0", "small_xf", "small_Ua", "small_Ub")):
        want = np.ascontiguousarray(g[name]).reshape(len(g["small_seeds"]), -1).view(np.uint64)
        assert np.array_equal(small[ai], want), name


def test_symbol_is_declared_bound_and_exported(lib):
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    core, ext = strip((ROOT / "include" / "dpilqr_hip.h").read_text()), strip((ROOT / "include" / "dpilqr_swarm_study.h").read_text())
    assert re.search(r'^\s*#\s*include\s+"dpilqr_swarm_study.h"', core, re.M)
    decl = dict(re.findall(r"\bint32_t\s+(dpilqr_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", ext))
    assert sorted(decl) == ["dpilqr_trial_inputs"] == sorted(lib.SWARM_STUDY_SIGNATURES)
    others = (set(lib.SIGNATURES) | set(lib.EXT_SIGNATURES) | set(lib.SWARM_SIGNATURES) | set(lib.SWARM_POLICY_SIGNATURES)
              | set(lib.SWARM_ADVANCE_SIGNATURES) | set(lib.ORDER_SIGNATURES) | set(lib.NEAREST_SIGNATURES))
    assert not set(lib.SWARM_STUDY_SIGNATURES) & others
    assert len(decl["dpilqr_trial_inputs"].split(",")) == N_ARGS == len(lib.SWARM_STUDY_SIGNATURES["dpilqr_trial_inputs"][1])
    fn = lib.load().dpilqr_trial_inputs
    assert fn.argtypes == lib.SWARM_STUDY_SIGNATURES["dpilqr_trial_inputs"][1] and fn.restype is C.c_int32
    assert int(re.search(r"#define\s+DPILQR_TRIAL_INPUTS_LDS\s+(\d+)", ext).group(1)) == lib.TRIAL_INPUTS_LDS
    assert lib.load().dpilqr_abi_version() == 4 == lib.ABI_VERSION      # additive: the ABI version stays


def test_entry_refuses_bad_arguments_before_any_launch(lib):
    L = lib.load()
    P = 1 << 20      # never dereferenced: every call below is refused first
    ok = dict(S=2, seed0=0, seeds=None, k=65, n_s=4, n_d=2, var=32.5, energy=130.0, n_warm=2, N=3, n_u=130, warm_scale=0.01, x0=P, xf=P,
              U_a=P, U_b=P, stream=None)
    bad = [dict(k=0), dict(k=257), dict(n_d=0), dict(n_d=4, n_s=6), dict(n_d=3, n_s=2), dict(n_warm=-1), dict(n_warm=3),
           dict(x0=None), dict(xf=None), dict(U_a=None), dict(U_b=None), dict(U_a=None, n_warm=1), dict(seed0=-1),
           dict(seed0=(1 << 32) - 1), dict(seed0=1 << 32, S=1), dict(S=-1), dict(N=0)]
    for change in bad:
        args = {**ok, **change}
        assert L.dpilqr_trial_inputs(*args.values()) == lib.EINVAL, change
        assert b"trial_inputs" in L.dpilqr_last_error(), change
    # what n_warm does not require may be NULL: nothing to refuse, and with S = 0 nothing to launch
    assert L.dpilqr_trial_inputs(*{**ok, "S": 0, "n_warm": 1, "U_b": None}.values()) == 0
    assert L.dpilqr_trial_inputs(*{**ok, "S": 0, "n_warm": 0, "U_a": None, "U_b": None, "seed0": (1 << 32) - 1}.values()) == 0


def test_code_object_has_no_scratch_no_spills_and_the_stated_lds(lib):
    import sys
    sys.path.insert(0, str(ROOT / "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    rows = [r for r in kernel_resources.resources() if r["demangled"] == "dpilqr::k_trial_inputs"]
    assert len(rows) == 1, [r["demangled"] for r in rows]
    r = rows[0]
    assert r["private_segment_fixed_size"] == 0 and r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["group_segment_fixed_size"] == lib.TRIAL_INPUTS_LDS and r["max_flat_workgroup_size"] == 128, r
