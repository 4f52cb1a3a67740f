"""Shared by tests/test_policy_advance_dec_wide_host.py, tests/test_gpu_policy_advance_dec_wide.py and
scripts/policy_advance_dec_wide_checks.py: the receding-horizon advance of a team of up to 256 agents
(dpilqr_policy_advance_dec_wide, csrc/policy_advance_dec_team.hpp at four mask words) on the six cases of tests/policy_dec_wide_cases.py, which are
imported and not changed.  Every (item i, sample s) of a case becomes ONE scenario q = i * S + s whose plan is item i's (X, U_ff,
Kc, words), repeated, as tests/policy_advance_dec_team_cases.py does it for the team advance.  Nothing here touches the GPU.

The shapes are the smallest at which THIS kernel can go wrong (a thread per (item, agent), ipw = floor(256 / k) items per
workgroup, n_words = ceil(k / 64) mask words):
  wide-dint4-k65-S4        two words; ipw = 3; its LAST scenario is left out (DROP): 11 items, the last workgroup holds two
  wide-dint4_uni4-k86-S3   ipw = 2; 9 scenarios, the last workgroup holds one; mixed models; per-item weights
  wide-car3-k65-S3         the three-state family; 9 scenarios in three full workgroups
  wide-quad12-k65-S2       the register peak; n_dims = 3
  wide-dint4-k129-S2       three words, the last holding one agent; ipw = 1
  wide-dint4-k256-S2       four words; bit 255; all 256 lanes; the offset k / 2

The CPU side is the prefix of WideCaseRef's own reference: policy_advance_dec_team_cases.prefix / prefix_figures /
scenario_error serve it unchanged (they read ref.ref, ref.problems, ref.batch and use policy_dec_team_cases.separation).  The
bound of a scenario is policy_cases.bound_of of the sample's own sensitivity.

member_walk is the kernel's walk of a lane's words, in NumPy: word by word, lowest bit first, the lowest kc_max members among
the low k bits kept; block p of the lane's compact rows belongs to its p-th member.

The loop's problem is tests/swarm_cases.py's first case: 65 double integrators (one neighbourhood across bit 64), horizon 10,
two of its scenarios, two steps a round, four steps: two rounds, under a disturbance."""
import numpy as np

from tests import policy_advance_cases as ac
from tests import policy_advance_dec_team_cases as atc
from tests import policy_cases as pc
from tests import policy_dec_wide_cases as wc
from tests import swarm_cases as sw

T, B = pc.T, pc.B
N_D, SPARE, HS = ac.N_D, ac.SPARE, ac.HS
CASES, IDS = wc.CASES, wc.IDS
VARIANTS = atc.VARIANTS
DROP = {"wide-dint4-k65-S4": 1}      # scenarios left out at the end of a case: a partly filled last workgroup at ipw = 3
prefix, prefix_figures, scenario_error = atc.prefix, atc.prefix_figures, atc.scenario_error


def kept(case):
    """The scenarios q = i * S + s of a case that the tests run."""
    return np.arange(B * case.S - DROP.get(case.id, 0))


def repeated(case, ref, fill=np.nan):
    """Host arrays of the case's scenarios (kept(case)): plans, compact gains (`fill` past every neighbourhood), words, starts,
    and W as (scenarios, T, n_x); `item`, `sample`: where every scenario comes from."""
    b, S = ref.batch, case.S
    q = kept(case)
    rep = lambda a: np.repeat(np.asarray(a), S, axis=0)[q]
    Kc = ref.Kc if np.isnan(fill) else np.where(np.isnan(ref.Kc), fill, ref.Kc)
    return dict(X=rep(ref.X), U=rep(ref.U), Kc=rep(Kc), words=rep(ref.words), x0=b["x0s"].reshape(B * S, -1)[q].copy(),
                W=b["W"].reshape(B * S, T, -1)[q].copy(), n=len(q), item=q // S, sample=q % S)


def problem_batch(case, b, items):
    """The device batch whose item j is the case's item items[j] (per-item weights follow)."""
    import dpilqr_amd as dp
    if case.weights == "per_item":
        Q, R, Qf = b["Q"][items], b["R"][items], b["Qf"][items]
    else:
        Q, R, Qf = b["Q"], b["R"], b["Qf"]
    return dp.ProblemBatch(b["models"], b["n_dims"], b["xf"][items], Q, R, Qf, b["radius"], b["dt"], T)


def member_walk(words, k, kc_max):
    """The kernel's walk of one lane's words (n_words,) uint64: the members it keeps, in the order it meets them."""
    out = []
    for w in range(4):      # kPolicyWideWords; words at and past n_words are zero
        hi = k - 64 * w
        rem = int(words[w]) if w < len(words) and hi > 0 else 0
        if hi < 64:
            rem &= (1 << max(hi, 0)) - 1
        while rem and len(out) < kc_max:
            low = rem & -rem
            out.append(64 * w + low.bit_length() - 1)
            rem &= rem - 1
    return out


# ---- the loop's problem: the first swarm of tests/swarm_cases.py
LOOP_CASE = sw.CASES[0]
S_LOOP, H_LOOP, L_LOOP = 2, 2, 4      # two scenarios, two steps a round, four steps: two rounds
N_LOOP = LOOP_CASE.T


def loop_problem(xf):
    import dpilqr_amd as dp
    from tests.test_gpu_swarm import dp_problem
    return dp_problem(dp, LOOP_CASE, xf)


def loop_inputs():
    """Starts, the goal (one for all scenarios), warm starts and the plant's disturbance, drawn as tests/policy_cases.py draws it."""
    x0s, xf, U0 = sw.scenario(LOOP_CASE, sw.OFFSET_SOLVE)
    rng = np.random.default_rng(6565)
    W = pc.W_SCALE * rng.normal(size=(S_LOOP, L_LOOP, LOOP_CASE.k * LOOP_CASE.ns))
    return x0s[:S_LOOP].copy(), xf, np.tile(U0[None], (S_LOOP, 1, 1)), W
