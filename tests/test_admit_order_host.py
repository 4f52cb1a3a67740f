"""The host side of csrc/admit_order.hpp without a GPU: tests/admit_order_check.cpp (a stand-alone program with its own main) is
compiled against the header with the host compiler -- with AddressSanitizer and UBSan where the compiler has them -- and run
directly.  It checks, for n in {1, 2, 63, 64, 1024, 1025, 2048, 2049, 3071, 3072, 3073, 6144, 6145, 20480}, n_cus in {1, 8, 256} and
the 4 / 8 / 12-wavefront tiers, that the rank -> position map of both orders is a permutation of 0..n-1 and that the grouped order
gives each sweep workgroup's positions consecutive ranks.  The library's own dpilqr_order_position must answer the same."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"dpilqr_cost_keys": 6, "dpilqr_order_list": 9, "dpilqr_order_position": 5}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dpilqr_amd import _lib
    return _lib


def _compile(cxx, out, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", str(ROOT / "dpilqr_amd" / "csrc"), "-o", str(out),
           str(ROOT / "tests" / "admit_order_check.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_rank_to_position_map_stand_alone(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "admit_order_check"
    built = _compile(cxx, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0:      # a compiler without the sanitizer runtimes: the same program, plain
        built = _compile(cxx, exe, [])
    assert built.returncode == 0, built.stderr[-3000:]
    import os
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert run.stdout.strip() == f"ok {14 * 3 * 3}", run.stdout[-1000:]


def test_symbols_are_declared_bound_and_exported(lib):
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    core, ext = strip((ROOT / "include" / "dpilqr_hip.h").read_text()), strip((ROOT / "include" / "dpilqr_order.h").read_text())
    assert re.search(r'^\s*#\s*include\s+"dpilqr_order.h"', core, re.M)
    decl = dict(re.findall(r"\bint32_t\s+(dpilqr_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", ext))
    assert sorted(decl) == sorted(NAMES) == sorted(lib.ORDER_SIGNATURES)
    assert not set(lib.ORDER_SIGNATURES) & (set(lib.SIGNATURES) | set(lib.EXT_SIGNATURES) | set(lib.SWARM_SIGNATURES))
    for name, n_args in NAMES.items():
        assert len(decl[name].split(",")) == n_args == len(lib.ORDER_SIGNATURES[name][1]), name
        fn = getattr(lib.load(), name)
        assert fn.argtypes == lib.ORDER_SIGNATURES[name][1] and fn.restype is C.c_int32
    assert lib.load().dpilqr_abi_version() == 4      # additive: the ABI version stays


@pytest.mark.parametrize("n,n_cus,waves", [(1, 256, 4), (63, 8, 8), (1025, 256, 8), (2049, 256, 12), (3073, 8, 12), (6144, 256, 12), (6145, 256, 12)])
def test_library_map_is_the_headers(lib, n, n_cus, waves):
    """dpilqr_order_position (the library's copy of the header's map): permutations, spread = identity, grouped = consecutive ranks
    per workgroup in the sweep's own dealing (riccati_mfma.hpp: slot = layer 4 n_cus + simd n_cus + cu, rounds split evenly)."""
    L = lib.load()
    spread = [L.dpilqr_order_position(r, n, n_cus, waves, lib.ORDER_SPREAD) for r in range(n)]
    assert spread == list(range(n))
    pos = [L.dpilqr_order_position(r, n, n_cus, waves, lib.ORDER_GROUPED) for r in range(n)]
    assert sorted(pos) == list(range(n))
    rank_at = {p: r for r, p in enumerate(pos)}
    # the sweep's dealing, written out independently of the header
    per_layer = 4 * n_cus
    layers = -(-n // per_layer)
    rounds = -(-layers // (waves // 4))
    lo, extra = divmod(layers, rounds)
    nxt = 0
    for rnd in range(rounds):
        my_layers = lo + (1 if rnd < extra else 0)
        first = rnd * lo + min(rnd, extra)
        for cu in range(n_cus):
            for wave in range(4 * my_layers):
                slot = (first + (wave >> 2)) * per_layer + (wave & 3) * n_cus + cu
                if slot < n:
                    assert rank_at[slot] == nxt, (rnd, cu, wave)
                    nxt += 1
    assert nxt == n
    for bad in ((-1, n, n_cus, waves, 1), (n, n, n_cus, waves, 2), (0, n, 0, waves, 1), (0, n, n_cus, 6, 1), (0, n, n_cus, waves, 0)):
        assert L.dpilqr_order_position(*bad) == lib.EINVAL and b"order_position" in L.dpilqr_last_error()


def test_entries_refuse_bad_arguments_before_any_launch(lib):
    L = lib.load()
    P = 1 << 20
    d = lib.BatchDesc(4, 2, 6, 3, 5, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)
    assert L.dpilqr_cost_keys(C.byref(d), P, None, None, P, None) == lib.EUNSUPPORTED and b"four-state" in L.dpilqr_last_error()
    d4 = lib.BatchDesc(4, 2, 4, 2, 5, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)
    assert L.dpilqr_cost_keys(C.byref(d4), None, None, None, P, None) == lib.EINVAL
    assert L.dpilqr_cost_keys(C.byref(d4), P, P, None, P, None) == lib.EINVAL      # items and n_items go together
    assert L.dpilqr_order_list(None, P, P, 5, 256, 12, 1, P, None) == lib.EINVAL
    for T, n_cus, waves, order in ((0, 256, 12, 1), (5, 0, 12, 1), (5, 256, 16, 1), (5, 256, 12, 3)):
        assert L.dpilqr_order_list(P, P, P, T, n_cus, waves, order, P, None) == lib.EINVAL and b"order_list" in L.dpilqr_last_error()
