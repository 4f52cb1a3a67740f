"""The cases of the large-cluster closed-loop rollout check (dpilqr_policy_rollout_large, csrc/policy_large.hpp), shared by
tests/test_policy_large_host.py and tests/test_gpu_policy_large.py.  Nothing here touches the GPU.

Everything but the cases is tests/policy_cases.py's, unchanged: Case, CaseRef (nominal and gains of the oracle, the reference loop
per sample, its rounding sensitivity), difference, bound_of, B = 3, T = 12, the 5 % cap on unchecked samples.

The cases put every edge of the kernel's tiling at the smallest size that has it -- 16-row tiles of K[t] dealt to four
wavefronts, 16-sample column tiles, reduction steps of four columns, spw = floor(256 / k) samples per workgroup:
  dint4_uni4-k16-S17       n_x 64, n_u 32: two exact row tiles; spw 16: one exact column tile
  quad6-k11-S24            n_x 66: n_x % 4 = 2, the zeroed tail columns; n_u 33: a third row tile with one valid row; spw 23: two
                           column tiles
  quad12-k6-S43            n_x 72, n_u 24: the second row tile half used; spw 42: three column tiles, the last with 10 samples
  quad12_human12-k20-S13   n_x 240, n_u 80 (BASELINE config 5's own size): five row tiles on four wavefronts, the models mixed
                           inside a wavefront, n_dims not homogeneous (per-pair dimensions); spw 12
In every case S = spw + 1: a second workgroup carries a single sample.

Start perturbation and radius were set on the CPU reference alone (test_case_conditions asserts what they must achieve).  At
radius 3.0 the six-quadcopter case leaves 26 % of its samples without a bound, at radius 1.0 the twenty-agent case 41 %: the
closed loop itself is unstable there.

tests/linesearch_cases.U0_NOISE has no entry for model 8, the padded HumanDynamics6D: the twenty-agent case was calibrated with a
noise of 0.05 supplied for it while policy_cases.make_batch runs, and case_ref does the same -- the shared dict is as it was
afterwards."""
from contextlib import contextmanager

from tests import linesearch_cases as lc
from tests import policy_cases as pc

T, B = pc.T, pc.B
HUMAN12 = 8
HUMAN12_NOISE = 0.05

CASES = [
    pc.Case("dint4_uni4-k16-S17", [0, 3] * 8, 17, 0.3, 0.6, weights="per_item", seed=11),
    pc.Case("quad6-k11-S24", [4] * 11, 24, 0.6, 0.15, weights="shared", seed=12),
    pc.Case("quad12-k6-S43", [7] * 6, 43, 0.1, 1.0, weights="shared", seed=13),
    pc.Case("quad12_human12-k20-S13", [7] * 14 + [HUMAN12] * 6, 13, 0.3, 0.5, n_dims=[3] * 14 + [2] * 6, weights="per_agent", seed=14),
]
SPW = {c.id: 256 // c.k for c in CASES}


@contextmanager
def _human12_noise():
    had = HUMAN12 in lc.U0_NOISE
    old = lc.U0_NOISE.get(HUMAN12)
    lc.U0_NOISE[HUMAN12] = HUMAN12_NOISE
    try:
        yield
    finally:
        if had:
            lc.U0_NOISE[HUMAN12] = old
        else:
            del lc.U0_NOISE[HUMAN12]


_REFS = {}


def case_ref(case):
    """policy_cases.CaseRef of a case, computed once and shared (never modified) by the tests that need it."""
    if case.id not in _REFS:
        with _human12_noise():
            _REFS[case.id] = pc.CaseRef(case)
    return _REFS[case.id]
