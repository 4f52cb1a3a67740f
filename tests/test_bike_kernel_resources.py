"""The five-state family's kernels (BikeDynamics5D) in the BUILT library (scripts/kernel_resources.py): the in-sweep production
sweeps of tu_bike.hip, the per-model line search / rollout, the family-5 tile producer and the generic forward pass exist; the
hot ones keep every register out of scratch; and the large-cluster sweep is not instantiated for the family."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))

BIKE_INPROD = [f"k_riccati_bike_inprod<{n}, {m}, {w}>" for n, m in ((8, 4), (12, 6), (16, 8), (20, 10)) for w in (4, 8)]
BIKE_WAVE = [f"k_linesearch_wave<10, {k}>" for k in range(1, 7)] + [f"k_rollout_wave<10, {k}>" for k in range(1, 7)]
BIKE_TILES = ["k_make_tiles<5, 2, false>", "k_make_tiles<5, 2, true>"]


@pytest.fixture(scope="module")
def table():
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    rows = kernel_resources.resources()
    assert len(rows) > 200
    return {r["demangled"]: r for r in rows}


@pytest.mark.parametrize("name", BIKE_INPROD + BIKE_WAVE + BIKE_TILES)
def test_bike_kernels_do_not_spill(table, name):
    r = table[name]
    # (scratch: at most the 36 B stack object of the trigonometric argument reduction the other families' kernels may carry)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] <= 36, (name, r)


def test_bike_generic_kernels_exist(table):
    """The size-generic kernels the family reaches beyond the specialised ones: the forward pass / line search of clusters of
    7..12 bikes, the model FFI and the cost evaluation."""
    names = ["k_cost_eval<5, 2>"] + [f"k_model_op<5, 2, {op}>" for op in range(3)]
    for name in names:
        assert table[name]["vgpr_spill_count"] == 0, (name, table[name])
    fwd = [k for k in table if k.startswith("k_forward<double, 5, 2, false")]
    assert fwd, "k_forward<double, 5, 2, false, ...> missing"
    # the generic forward pass spills for every family (a 256-register cap at two workgroups per CU); the bike's instantiation
    # is held to what the six-state family's already costs
    six = [table[k] for k in table if k.startswith("k_forward<double, 6, 3, false")]
    for k in fwd:
        assert table[k]["vgpr_spill_count"] <= max(r["vgpr_spill_count"] for r in six), (k, table[k])


def test_no_large_cluster_sweep_for_the_family(table):
    assert not [k for k in table if k.startswith("k_riccati_big<") and k.endswith(", 5, 2>")]
    assert not [k for k in table if k.startswith("k_riccati_mfma_inprod<") and ", 5, " in k]
    assert not [k for k in table if k.startswith("k_linesearch_team<10,")]
