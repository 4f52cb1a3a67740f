"""The CPU side of tests/test_gpu_singular.py, without a GPU: every item tests/singular_cases.py labels singular draws the
oracle's zero-pivot verdict and no other item does; the solve cases reach every sweep class of the loop; the tile cases reach
every route of the record-fed launcher; and the ABI's convention for a listed launch -- flags by item id, gains by list position
-- holds on the CPU twin."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import loop_gains_cases as lg
from tests import singular_cases as sc
from tests.golden_util import relerr

ROOT = Path(__file__).resolve().parent.parent
TILE_CASES = sc.tile_cases()
SOLVE_CASES = sc.solve_cases() + [sc.window_edge_case(), sc.enqueue_case()]
CHECKED = 60      # items of a batch whose verdict is drawn here (the GPU test draws all of them)


def _labelled_singular(item):
    return item[0] not in ("healthy", "tiny")


@pytest.mark.parametrize("case", TILE_CASES, ids=[c.id for c in TILE_CASES])
def test_tile_items_draw_the_labelled_verdict(case):
    assert sc.tile_route(case) == case.route
    items = case.items()
    assert case.complete() or case.count == 9
    kinds = {it[0] for it in items}
    assert {"healthy", "tiny"} <= kinds and len(kinds) >= 4 and {it[2] for it in items} == set(sc.PLACEMENTS)
    arrays = sc.make_tiles(case)
    assert not arrays[1].any()      # B = 0: Q_uu = L_uu
    for i, (item, (flag, K, d)) in enumerate(zip(items, sc.tile_verdicts(arrays))):
        assert flag == _labelled_singular(item), (i, item)
        if not flag:
            assert np.isfinite(K).all() and np.isfinite(d).all(), (i, item)


def test_tile_routes_are_all_reached():
    assert {c.route for c in TILE_CASES} == {"wave-bd", "wave-dense", "wave-mfma", "padded", "workgroup", "generic"}
    assert {c.count for c in TILE_CASES if c.route == "wave-bd"} == {9, 1100, 2100}
    assert 9 <= lg.TEAM_MAX < 1100 and lg.TIER8_ABOVE < 1100 <= lg.TIER12_ABOVE < 2100      # the 4-, 8- and 12-wavefront tiers


@pytest.mark.parametrize("case", [c for c in TILE_CASES if c.count < 100][::3], ids=lambda c: c.id)
def test_the_oracle_holds_the_tolerance_on_the_tiny_pivot(case):
    """The 2^-60 pivot makes row 1 of K about 1e18, but nothing of it leaks: the column's other entries are exactly zero, so no
    multiplier and no back-substitution term carries it.  The oracle's gains of the `tiny` items agree with an np.longdouble
    replay far inside the GPU test's tolerance, so that test holds `tiny` to the tolerance like `healthy`."""
    arrays = sc.make_tiles(case)
    seen = 0
    for i, (item, (flag, K, d)) in enumerate(zip(case.items(), sc.tile_verdicts(arrays))):
        if item[0] != "tiny" or seen == 3:
            continue
        seen += 1
        Kl, dl = sc.longdouble_pass_tiles(*(a[i] for a in arrays), sc.TILE_MU)
        assert relerr(K, Kl.astype(np.float64)) < 1e-3 * case.tol and relerr(d, dl.astype(np.float64)) < 1e-3 * case.tol, i
    assert seen == min(3, sum(it[0] == "tiny" for it in case.items())) >= 2


@pytest.mark.parametrize("case", SOLVE_CASES, ids=[c.id for c in SOLVE_CASES])
def test_solve_items_draw_the_labelled_verdict(case):
    b = sc.make_solve_batch(case)
    mixed = case.how != "shared_R"
    assert b["singular"].any() and (not mixed or not b["singular"].all())
    idx = sorted(set(range(min(case.B, CHECKED))) | {case.B - 1})
    for i in idx:
        flag, K, d = sc.item_verdict(b, i)
        assert flag == bool(b["singular"][i]), i
        r = sc.item_problem(b, i).solve(b["x0"][i], b["U0"][i], n_lqr_iter=case.n_lqr_iter)
        if flag:
            assert r["status"] == -1 and r["n_bwd"] == 0, (i, r["status"])      # the oracle's zero-pivot code
        else:
            assert np.isfinite(K).all() and np.isfinite(d).all() and r["status"] in (1, 2, 3) and np.isfinite(r["J"]), (i, r["status"])
    if not mixed:
        h = sc.make_solve_batch(case, healthy_twin=True)
        assert not h["singular"].any() and not any(sc.item_verdict(h, i)[0] for i in idx)


def test_solve_cases_reach_every_sweep_class():
    routes = {c.id: lg.loop_route(c)[1] for c in sc.solve_cases()}
    assert routes == sc.SOLVE_ROUTES
    assert set(routes.values()) == set(lg.SWEEPS)
    assert lg.loop_route(sc.window_edge_case())[1] == "in-sweep production" and lg.loop_route(sc.enqueue_case())[1] == "record-fed padded"
    e = sc.window_edge_case()
    assert list(np.flatnonzero(e.mask)) == [0, e.window - 1, e.window, 22, e.B - 1]
    for c in sc.solve_cases():
        assert c.T <= 8 and c.n_lqr_iter <= 6


def test_sweep_cases_take_the_sweep_they_are_meant_for():
    cases = sc.sweep_cases()
    for case, route in cases:
        assert sc.sweep_route(case) == route, case.id
        assert (case.B <= lg.TEAM_MAX) == (case.B != 1100)
        b = sc.make_solve_batch(case)
        for i in sorted(set(range(CHECKED // 2)) | {case.B - 1}):
            assert sc.item_verdict(b, i)[0] == bool(b["singular"][i]), (case.id, i)
    assert {r for _, r in cases} == {"in-sweep production", "team", "fused wavefront", "fused general", "fused workgroup"}


@pytest.fixture(scope="module")
def twin():
    subprocess.run(["make", "-s", "-C", str(ROOT / "oracle"), str(ROOT / "oracle" / "libdpilqr_cpu_twin.so")], check=True)
    from dpilqr_amd import _lib
    L = C.CDLL(str(ROOT / "oracle" / "libdpilqr_cpu_twin.so"))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L, _lib


@pytest.mark.parametrize("case", [c for c in TILE_CASES if c.count < 100], ids=lambda c: c.id)
def test_listed_launch_on_the_cpu_twin(twin, case):
    """An item list through the ABI (include/dpilqr_hip.h): mu and singular[] are indexed by item id, the tile records, K and d
    by position in the list; items not listed are not touched."""
    L, _lib = twin
    arrays = sc.make_tiles(case)
    verdicts = sc.tile_verdicts(arrays)
    rec, stride = sc.pack_records(_lib, *arrays)
    Bn, T, n, m = case.count, case.T, case.n, case.m
    rng = np.random.default_rng(case.n)
    items = np.ascontiguousarray(rng.permutation(Bn)[:2 * Bn // 3], dtype=np.int32)
    listed = np.zeros(Bn, dtype=bool); listed[items] = True
    assert any(verdicts[i][0] for i in np.flatnonzero(~listed)) and any(verdicts[i][0] for i in items)
    cnt = np.array([len(items) - 2], dtype=np.int32)          # the live count is shorter than the list
    live = items[:cnt[0]]
    mu = np.full(Bn, sc.TILE_MU)
    rec = np.ascontiguousarray(rec[items])
    K = np.full((Bn, T, m, n), -7.0); d = np.full((Bn, T, m), -7.0); sing = np.zeros(Bn, dtype=np.int32)
    bns, bnc = case.blocks or (0, 0)
    hp = lambda a: a.ctypes.data
    assert L.dpilqr_backward_pass_tiles_blocks(Bn, T, n, m, bns, bnc, hp(rec), hp(mu), hp(K), hp(d), hp(sing), hp(items), hp(cnt), None) == 0
    want = np.zeros(Bn, dtype=np.int32)
    for i in live:
        want[i] = int(verdicts[i][0])
    assert np.array_equal(sing, want)
    for slot, i in enumerate(live):
        if not verdicts[i][0]:
            assert np.array_equal(K[slot], verdicts[i][1]) and np.array_equal(d[slot], verdicts[i][2]), (slot, i)
    assert (K[cnt[0]:] == -7.0).all() and (d[cnt[0]:] == -7.0).all()
