"""Shared by tests/test_policy_advance_large_host.py and tests/test_gpu_policy_advance_large.py: the receding-horizon advance for
large clusters (dpilqr_policy_advance_large, csrc/policy_advance_large.hpp) on the cases of tests/policy_large_cases.py, which
are imported and not changed -- the four cases already put every edge of the product's tiling at its smallest size (n_x 64 / n_u
32: two exact row tiles; 66 / 33: n_x % 4 = 2 and a row tile with one valid row; 72 / 24: the second row tile half used; 240 / 80:
five row tiles on four wavefronts, mixed models, heterogeneous n_dims).  Nothing here touches the GPU.

Every (item i, sample s) of a case becomes ONE scenario q = i * S + s whose plan is item i's (X, U, K), repeated: the helpers
are tests/policy_advance_cases.py's (repeated, problem_batch, scen_of, shift, prefix, prefix_figures), T = 12, B = 3.

HS: the executed lengths the GPU tests use, per case.  The candidates are 1, 3 and T; a length is used where the case's prefix
is honest there (test_case_conditions of the host file asserts it from the CPU reference alone: the limits bind somewhere and
not everywhere, a sample of the W variant is inside the radius within the prefix, the unchecked share stays inside
policy_cases' cap).  h = T is among them for every case: policy_large_cases' own conditions hold there."""
from tests import policy_advance_cases as ac
from tests import policy_large_cases as plc

T, B = plc.T, plc.B
N_D, SPARE = ac.N_D, ac.SPARE
CASES, case_ref = plc.CASES, plc.case_ref
IDS = [c.id for c in CASES]
HS = {c.id: (1, 3, T) for c in CASES}
CASE_H = [(c, h) for c in CASES for h in HS[c.id]]
CASE_H_IDS = [f"{c.id}-h{h}" for c, h in CASE_H]

repeated, problem_batch, scen_of, shift, prefix, prefix_figures = (ac.repeated, ac.problem_batch, ac.scen_of, ac.shift, ac.prefix,
                                                                   ac.prefix_figures)
