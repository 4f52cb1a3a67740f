"""The decoupled prologue of the fused DoubleInt4D wavefront sweep (csrc/riccati_mfma.hpp) on the device.

Behind an item's last near step (walking back from t = T) the sweep runs per-agent Riccati steps; at the first near pair, or at
the first doubt, it hands the step at hand to the dense loop.  Held here, at T = 12 and 1..5 agents, in launches of 1100 and 2100
items (the 8- and 12-wavefront tiers), on trajectories built by hand (tests/decoupled_sweep_cases.py): never near, near at every
step, near only at t = T, near at exactly one step (0, 1, 6, T-2, T-1), near over an interval and again later, one pair at distance
exactly r and at r (1 + 2e-12); shuffled, with per-item radius, mu in {0, 0.125, 1, 64}, goal and controls.
  * K and d equal the record-fed sweep's under ==, item for item;
  * K[t] is zero outside the agents' blocks on the steps behind the item's last near step -- exactly on the steps t >= last - 1, see
    the test -- so the cases are what they claim to be;
  * the CPU oracle agrees within TOL_PASS on one item per case (both device routes wrong together is excluded);
  * the same item at two list positions and in two launch sizes gives the same bits;
  * an Inf and a NaN in X behind the last near step: non-finite entries where the record-fed result has them, all else equal;
  * the key kernel's second output equals a NumPy statement of "last near step + 1";
  * DPILQR_NO_DECOUPLED (child process, behind DPILQR_DEBUG_ROUTES=1) gives the same bits, in the passes and in a windowed solve
    of cfg2's distribution (3000 items, window 2100, six iterations)."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import decoupled_sweep_cases as dc

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TOL_PASS = 1e-9
T = dc.T


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()
    return dpilqr_amd


@functools.lru_cache(maxsize=None)
def results(k):
    """the batch of k agents and both routes' gains for both launch sizes, computed once"""
    import dpilqr_amd
    return dc.build(k), dc.passes(dpilqr_amd, k)


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def off_block_mask(k):
    m = np.ones((2 * k, 4 * k), dtype=bool)
    for a in range(k):
        m[2 * a:2 * a + 2, 4 * a:4 * a + 4] = False
    return m


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_prologue_is_bit_identical_to_the_record_fed_sweep(dp, k):
    c, res = results(k)
    finite_items = np.array([i not in dc.NONFINITE for i in range(max(dc.SIZES))])
    for B in dc.SIZES:
        K1, d1 = res["fused", B]; K0, d0 = res["record", B]
        keep = finite_items[:B]
        assert np.isfinite(K0[keep]).all() and np.isfinite(d0[keep]).all()
        bad = np.flatnonzero((K1[keep] != K0[keep]).reshape(keep.sum(), -1).any(1) | (d1[keep] != d0[keep]).any((1, 2)))
        assert bad.size == 0, (B, bad[:10], [dc.NAMES[c["case"][:B][keep][i]] for i in bad[:10]])
    # the cases are what they claim to be: where the blocks of K decouple
    near = dc.near_steps(c["X"], k, c["radius"])
    last = dc.last_near(near)
    if k == 1:
        assert (last == -1).all()
    else:
        want = {"never": -1, "always": T, "terminal": T, "interval+later": 9, "exact@7": 7, "outside@7": -1}
        for i in range(max(dc.SIZES)):
            name = dc.NAMES[c["case"][i]]
            assert last[i] == (want[name] if name in want else int(name.split("@")[1])), (i, name, last[i])
        K1 = res["fused", max(dc.SIZES)][0]
        off = np.abs(K1[:, :, off_block_mask(k)]).max(2)            # [B][T]
        steps = np.arange(T)[None, :]
        # (K[t] = -Q_uu^-1 B^T P[t+1] A takes the velocity rows of P[t+1]; a near step t+1 couples the position entries of P[t+1] only,
        # which A spreads to the velocity rows one step later: K[t] is coupled from t = last - 2 down)
        assert (off[(steps >= last[:, None]) & finite_items[:, None]] == 0.0).all()             # behind the last near step
        assert (off[(steps >= last[:, None] - 1) & finite_items[:, None]] == 0.0).all()
        assert (off[(steps < last[:, None] - 1) & finite_items[:, None]] > 0.0).all()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_prologue_agrees_with_the_oracle(dp, k):
    from oracle import oracle as orc
    c, res = results(k)
    K1, d1 = res["fused", min(dc.SIZES)]
    for v in range(len(dc.NAMES)):
        i = int(np.flatnonzero((c["case"][:min(dc.SIZES)] == v) & np.array([j not in dc.NONFINITE for j in range(min(dc.SIZES))]))[0])
        proto = orc.Problem([0] * k, [2] * k, c["xf"][i], dc.Q, dc.R, dc.QF, float(c["radius"][i]), 0.1, T)
        Ko, do = proto.backward_pass(c["X"][i], c["U"][i], float(c["mu"][i]))
        assert relerr(K1[i], Ko) < TOL_PASS and relerr(d1[i], do) < TOL_PASS, (dc.NAMES[v], i, relerr(K1[i], Ko), relerr(d1[i], do))


@pytest.mark.parametrize("k", [2, 5])
def test_results_do_not_depend_on_the_position(dp, k):
    c, res = results(k)
    Kl, dl = res["fused", max(dc.SIZES)]; Ks, ds = res["fused", min(dc.SIZES)]
    keep = np.array([i not in dc.NONFINITE for i in range(min(dc.SIZES))])
    assert np.array_equal(Ks[keep], Kl[:min(dc.SIZES)][keep]) and np.array_equal(ds[keep], dl[:min(dc.SIZES)][keep])     # two launch sizes
    for src, dst in dc.DUPLICATES:
        assert np.array_equal(Kl[src], Kl[dst]) and np.array_equal(dl[src], dl[dst]), (src, dst)
        if dst < min(dc.SIZES):
            assert np.array_equal(Ks[src], Ks[dst]) and np.array_equal(ds[src], ds[dst]), (src, dst)


@pytest.mark.parametrize("k", [1, 3, 5])
def test_a_non_finite_iterate_is_handed_to_the_dense_step(dp, k):
    c, res = results(k)
    for B in dc.SIZES:
        K1, d1 = res["fused", B]; K0, d0 = res["record", B]
        for i in dc.NONFINITE:
            assert not np.isfinite(K0[i]).all() or not np.isfinite(d0[i]).all()          # the entry does reach the gains
            assert np.array_equal(np.isfinite(K1[i]), np.isfinite(K0[i])) and np.array_equal(np.isfinite(d1[i]), np.isfinite(d0[i])), (B, i)
            fk, fd = np.isfinite(K0[i]), np.isfinite(d0[i])
            assert np.array_equal(K1[i][fk], K0[i][fk]) and np.array_equal(d1[i][fd], d0[i][fd]), (B, i)
            assert np.array_equal(np.isnan(K1[i]), np.isnan(K0[i])) and np.array_equal(np.isnan(d1[i]), np.isnan(d0[i])), (B, i)
            # its neighbours in the launch are unaffected (they are among the items the bit-identity test holds to the record-fed sweep)
            for j in (min(dc.NONFINITE) - 1, max(dc.NONFINITE) + 1):
                assert j not in dc.NONFINITE and np.isfinite(K1[j]).all() and np.array_equal(K1[j], K0[j]) and np.array_equal(d1[j], d0[j])


@pytest.fixture(scope="module")
def switched_off(dp, tmp_path_factory):
    """the child process: the prologue switched off, and dpilqr_cost_keys giving the key kernel's second output"""
    out = tmp_path_factory.mktemp("decoupled") / "off.npz"
    e = {key: v for key, v in os.environ.items() if not key.startswith("DPILQR_")}
    e.update({"DPILQR_DEBUG_ROUTES": "1", "DPILQR_NO_DECOUPLED": "1", "DPILQR_KEYS_DENSE_STEPS": "1"})
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "decoupled_sweep_cases.py"), str(out)], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(out)


@pytest.mark.parametrize("k", [2, 5])
def test_the_route_switch_gives_the_same_bits(dp, switched_off, k):
    c, res = results(k)
    for B in dc.SIZES:
        K1, d1 = res["fused", B]
        assert np.array_equal(K1, switched_off[f"K/{k}/{B}"], equal_nan=True) and np.array_equal(d1, switched_off[f"d/{k}/{B}"], equal_nan=True)
        # (sign of zeros aside, that is; and the NaNs of the two non-finite items sit at the same places)


def test_a_windowed_solve_equals_the_switched_off_route(dp, switched_off):
    got = dc.windowed_solve(dp)
    assert (got["status"] != 0).all() and len(set(got["n_bwd"].tolist())) > 1
    for key in ("X", "U", "J", "status", "n_bwd", "n_fwd"):
        differ = np.flatnonzero((got[key] != switched_off[f"solve/{key}"]).reshape(3000, -1).any(1))
        assert differ.size == 0, (key, differ[:10])


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_the_second_key_is_the_last_near_step_plus_one(dp, switched_off, k):
    """k_cost_keys' second output (the sweep's dense steps) against a NumPy statement of it on the cases above; the exported
    dpilqr_cost_keys gives it only behind the test switch DPILQR_KEYS_DENSE_STEPS (the child process), and the near-step count here."""
    c = dc.build(k)
    near = dc.near_steps(c["X"], k, c["radius"])
    want = (dc.last_near(near) + 1).astype(np.int32)
    assert k == 1 or len(set(want.tolist())) >= 8                  # 0, 1, 2, 7, 8, 10, T-1, T, T+1
    np.testing.assert_array_equal(switched_off[f"keys/{k}"], want)
    listed = switched_off[f"keys_listed/{k}"]
    np.testing.assert_array_equal(listed[:len(dc.LISTED)], want[dc.LISTED])
    assert (listed[len(dc.LISTED):] == -7).all()
    count, _ = dc.device_keys(dp, k)
    np.testing.assert_array_equal(count, near.sum(1).astype(np.int32))
