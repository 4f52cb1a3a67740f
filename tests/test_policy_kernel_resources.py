"""The closed-loop rollout's kernels in the BUILT library (scripts/kernel_resources.py): k_policy_rollout<NS, NC> exists for every
family; the three- to six-state instantiations keep every register out of scratch; the twelve-state one carries no more scratch
than the table shows for the generic forward pass of that family, k_forward<double, 12, 4, false, false>."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    import kernel_resources
    if not (kernel_resources.LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-readelf")
    rows = kernel_resources.resources()
    assert len(rows) > 200
    return {r["demangled"]: r for r in rows}


@pytest.mark.parametrize("ns,nc", [(3, 2), (4, 2), (5, 2), (6, 3)])
def test_policy_kernels_do_not_spill(table, ns, nc):
    r = table[f"k_policy_rollout<{ns}, {nc}>"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["max_flat_workgroup_size"] == 256 and r["group_segment_fixed_size"] == 0, r      # LDS is sized by the launcher


def test_twelve_state_policy_kernel_against_the_generic_forward_pass(table):
    r, yard = table["k_policy_rollout<12, 4>"], table["k_forward<double, 12, 4, false, false>"]
    assert r["private_segment_fixed_size"] <= yard["private_segment_fixed_size"], (r, yard)
    assert r["vgpr_spill_count"] <= yard["vgpr_spill_count"], (r, yard)
