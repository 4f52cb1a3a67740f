"""The launch rule of the wavefront sweeps (launch.hpp: sweep_waves, sweep_grid), checked without a GPU: a small host program
compiled from launch.hpp and riccati_mfma.hpp prints what the two functions decide at the real LDS sizes of a few
instantiations (tests/sweep_launch_rules.cpp), and the tables below say what every launcher's own copy of the rule decided
before there was one helper:

    wavefronts per workgroup   12  if the family has a 12-wavefront instantiation (the record-fed sweep: for block-diagonal
                                   tiles only), grid_items > 2048, DPILQR_MFMA_WAVES >= 12 and 12 wavefronts' LDS <= 160 KiB
                                8  if grid_items > 1024, DPILQR_MFMA_WAVES >= 8 (and, in-sweep production, 8 wavefronts' LDS fit)
                                4  otherwise
    workgroups                 grid_items <= cus ? grid_items : ceil(grid_items / (cus * wv)) * cus"""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ITEMS = [1, 256, 257, 1024, 1025, 2048, 2049, 6144]
ONE = [4, 4, 4, 4, 4, 4, 4, 4]          # wavefronts per workgroup over ITEMS: one per SIMD whatever the launch
TWO = [4, 4, 4, 4, 8, 8, 8, 8]          # two per SIMD above 1024 items
THREE = [4, 4, 4, 4, 8, 8, 12, 12]      # ... and three above 2048

# bytes of LDS per wavefront: MfmaCfg::total (+ InprodCfg::total for in-sweep production) doubles
LDS = {"record_20_10": 13504, "record_24_12": 19264, "fused_20_10": 13424, "general_20_10": 14224,
       "inprod6_20_10": 19712, "inprod6_24_12": 28032, "bike_16_8": 12992, "bike_20_10": 19840}
K_MAX_LDS = 160 * 1024
# which side of the two caps each size is on
FITS_12 = {"record_20_10", "fused_20_10", "bike_16_8"}
FITS_8 = set(LDS) - {"inprod6_24_12"}

# {(site, 12-wavefront tier, DPILQR_MFMA_WAVES): wavefronts per workgroup over ITEMS}.  Tier 1 is what the launchers pass for
# the record-fed sweep of block-diagonal tiles and the fused sweep; 0 for every other family.
WAVES = {
    # record-fed k_riccati_mfma, (20, 10): block-diagonal tiles, then dense tiles
    ("record_20_10", 1, 12): THREE, ("record_20_10", 1, 8): TWO, ("record_20_10", 1, 4): ONE,
    ("record_20_10", 0, 12): TWO, ("record_20_10", 0, 8): TWO, ("record_20_10", 0, 4): ONE,
    # (24, 12): 12 wavefronts would need 231 168 B, so the tier makes no difference
    ("record_24_12", 1, 12): TWO, ("record_24_12", 1, 8): TWO, ("record_24_12", 1, 4): ONE,
    ("record_24_12", 0, 12): TWO, ("record_24_12", 0, 8): TWO, ("record_24_12", 0, 4): ONE,
    # fused k_riccati_mfma<..., true>
    ("fused_20_10", 1, 12): THREE, ("fused_20_10", 1, 8): TWO, ("fused_20_10", 1, 4): ONE,
    ("fused_20_10", 0, 12): TWO, ("fused_20_10", 0, 8): TWO, ("fused_20_10", 0, 4): ONE,
    # the general form (FUSED == 2): the per-agent weights take the LDS a third wavefront per SIMD needs (170 688 B)
    ("general_20_10", 1, 12): TWO, ("general_20_10", 1, 8): TWO, ("general_20_10", 1, 4): ONE,
    ("general_20_10", 0, 12): TWO, ("general_20_10", 0, 8): TWO, ("general_20_10", 0, 4): ONE,
    # in-sweep production, six-state family: (20, 10) fits eight wavefronts (157 696 B), (24, 12) does not (224 256 B)
    ("inprod6_20_10", 1, 12): TWO, ("inprod6_20_10", 1, 8): TWO, ("inprod6_20_10", 1, 4): ONE,
    ("inprod6_20_10", 0, 12): TWO, ("inprod6_20_10", 0, 8): TWO, ("inprod6_20_10", 0, 4): ONE,
    ("inprod6_24_12", 1, 12): ONE, ("inprod6_24_12", 1, 8): ONE, ("inprod6_24_12", 1, 4): ONE,
    ("inprod6_24_12", 0, 12): ONE, ("inprod6_24_12", 0, 8): ONE, ("inprod6_24_12", 0, 4): ONE,
    # BikeDynamics5D: three bikes (16, 8), four (20, 10; 158 720 B for eight wavefronts)
    ("bike_16_8", 1, 12): THREE, ("bike_16_8", 1, 8): TWO, ("bike_16_8", 1, 4): ONE,
    ("bike_16_8", 0, 12): TWO, ("bike_16_8", 0, 8): TWO, ("bike_16_8", 0, 4): ONE,
    ("bike_20_10", 1, 12): TWO, ("bike_20_10", 1, 8): TWO, ("bike_20_10", 1, 4): ONE,
    ("bike_20_10", 0, 12): TWO, ("bike_20_10", 0, 8): TWO, ("bike_20_10", 0, 4): ONE,
}
# workgroups at 256 CUs over ITEMS, per wavefronts per workgroup: whole rounds of one workgroup per CU
GRID = {4: [1, 256, 256, 256, 512, 512, 768, 1536],
        8: [1, 256, 256, 256, 256, 256, 512, 768],
        12: [1, 256, 256, 256, 256, 256, 256, 512]}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sweep") / "rules"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O0", "-Iinclude", "-Idpilqr_amd/csrc", "-o", str(exe),
                    "tests/sweep_launch_rules.cpp"], cwd=ROOT, check=True)
    rows = [line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    return {kind: [r[1:] for r in rows if r[0] == kind] for kind in ("lds", "waves", "grid")}


def test_lds_per_wavefront_and_the_caps(printed):
    assert {name: int(b) for name, b in printed["lds"]} == LDS
    assert {s for s, b in LDS.items() if 12 * b <= K_MAX_LDS} == FITS_12
    assert {s for s, b in LDS.items() if 8 * b <= K_MAX_LDS} == FITS_8


def test_wavefronts_per_workgroup(printed):
    got = {}
    for site, tier12, max_wv, items, wv in printed["waves"]:
        got.setdefault((site, int(tier12), int(max_wv)), {})[int(items)] = int(wv)
    assert set(got) == set(WAVES)
    for key, want in WAVES.items():
        assert got[key] == dict(zip(ITEMS, want)), key


def test_grid_is_whole_rounds_of_one_workgroup_per_cu(printed):
    got = {}
    for items, cus, wv, grid in printed["grid"]:
        assert int(cus) == 256
        got.setdefault(int(wv), {})[int(items)] = int(grid)
    assert got == {wv: dict(zip(ITEMS, g)) for wv, g in GRID.items()}
