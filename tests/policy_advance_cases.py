"""Shared by tests/test_policy_advance_host.py and tests/test_gpu_policy_advance.py: the receding-horizon advance
(dpilqr_policy_advance, csrc/policy_advance.hpp) on the cases of tests/policy_cases.py and tests/policy_dec_cases.py, which
are imported and not changed.  Every (item i, sample s) of a case becomes ONE scenario q = i * S + s whose plan is item i's
(X, U, K), repeated: the advance has one sample per item.  Nothing here touches the GPU.

The CPU side is the prefix of the cases' own reference (policy_cases.ref_sample): the executed cost, the smallest separation
over the states 0 .. h and the distance left after h steps are recomputed from its trajectories by a NumPy loop over
policy_cases._step_cost; the bound of a scenario is policy_cases.bound_of of the sample's own sensitivity."""
import numpy as np

from tests import policy_cases as pc

T, B = pc.T, pc.B
N_D = 2               # the coordinates of dist_left (solve_rhc's n_d)
SPARE = 3             # scenarios of a test's state that no item names
HS = (1, 3)


def repeated(case, ref):
    """Host arrays of the case's B * S scenarios: plans, batch parameters, starts, and W as (scenarios, T, n_x)."""
    b, S = ref.batch, case.S
    rep = lambda a: np.repeat(np.asarray(a), S, axis=0)
    return dict(X=rep(ref.X), U=rep(ref.U), K=rep(ref.K), xf=rep(b["xf"]), x0=b["x0s"].reshape(B * S, -1).copy(),
                W=b["W"].reshape(B * S, T, -1).copy(), n=B * S)


def problem_batch(case, b, repeat=1, T_=T):
    """The device batch of a case with every item repeated `repeat` times (per-item weights repeated with it)."""
    import dpilqr_amd as dp
    rep = lambda a: np.repeat(a, repeat, axis=0)
    if case.weights == "per_item":
        Q, R, Qf = rep(b["Q"]), rep(b["R"]), rep(b["Qf"])
    else:
        Q, R, Qf = b["Q"], b["R"], b["Qf"]
    return dp.ProblemBatch(b["models"], b["n_dims"], rep(b["xf"]), Q, R, Qf, b["radius"], b["dt"], T_)


def scen_of(case, n):
    """A non-identity map of the n items into a state of n + SPARE scenarios."""
    return np.random.default_rng(4200 + case.seed).permutation(n + SPARE)[:n].astype(np.int32)


def shift(X, U, x, he):
    """The definition of the warm start: U_next[t] = U[t + he] (0 beyond), X_next[0] = x, X_next[t] = X[min(t + he, T)]."""
    Tn = U.shape[0]
    Un = np.zeros_like(U); Un[:Tn - he] = U[he:]
    Xn = np.stack([x] + [X[min(t + he, Tn)] for t in range(1, Tn + 1)])
    return Un, Xn


def prefix(case, ref, variant, i, s, h):
    """From the CPU reference of (item i, sample s): J of the first h steps (one addition per step), the smallest separation
    over the states 0 .. h, the distance left at state h over N_D coordinates."""
    r, b = ref.ref[variant][i][s], ref.batch
    _, cost = pc._step_cost(ref.problems[i])
    J = 0.0
    for t in range(h):
        J = J + cost(r["X"][t], r["U"][t])
    sep = min(pc.separation(r["X"][t], case.k, case.ns, case.n_dims) for t in range(h + 1))
    e = (r["X"][h] - b["xf"][i]).reshape(case.k, case.ns)[:, :N_D]
    return J, sep, np.sqrt(np.sum(e * e, axis=1))


def prefix_figures(case, ref, h):
    """What keeps a case honest on a prefix of h steps, from the reference alone: the share of clamped control entries in the
    u_lim variant, the share of samples inside the radius within the prefix of the W variant, the samples without a bound."""
    S = case.S
    Us = np.stack([[ref.ref["u_lim"][i][s]["U"][:h] for s in range(S)] for i in range(B)])
    clamped = float(np.mean((Us == ref.u_lim[0]) | (Us == ref.u_lim[1])))
    near = float(np.mean([[min(pc.separation(ref.ref["W"][i][s]["X"][t], case.k, case.ns, case.n_dims) for t in range(h + 1))
                           < ref.batch["radius"] for s in range(S)] for i in range(B)]))
    unchecked = {v: ref.unchecked_fraction(v) for v in ("plain", "W", "u_lim")}
    return dict(clamped=clamped, near=near, unchecked=unchecked)
