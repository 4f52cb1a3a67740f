"""Shared by tests/test_gpu_policy.py and scripts/policy_rollout_sensitivity.py: the cases of the closed-loop rollout check,
their seeded batches, and the CPU side of the check -- the reference loop for one sample, its rounding sensitivity and the
per-sample bound drawn from it.  Nothing here touches the GPU.

The reference of every model the C oracle knows is a NumPy loop over oracle.Problem.step / .cost; BikeDynamics5D (a device
model only) uses the NumPy RK4 of tests/linesearch_cases.py.  Nominals and gains are the oracle's own: the nominal is its
rollout of (x0, U0), drawn per model as tests/linesearch_cases.py draws them, the gains its backward pass there."""
import itertools

import numpy as np

from tests import linesearch_cases as lc
from tests.golden_util import relerr

T, B = 12, 3
MU = 1.0                  # the regularisation of the backward pass that supplies the gains (a solve's first iteration)
W_SCALE = 1e-2
TOL_ROLLOUT = 1e-11       # the project's rollout tolerance
MAX_UNCHECKED = 0.05      # of a case's samples
QUANTILES = (0.3, 0.7)    # u_lim: these quantiles, per control, of the reference's own unclamped controls


class Case:
    """models (k,), S samples per item, the start perturbation (positions; the other states a tenth of it) and the radius."""

    def __init__(self, name, models, S, sigma, radius, n_dims=None, weights="shared", seed=0):
        self.name, self.models, self.S, self.sigma, self.radius, self.weights, self.seed = name, list(models), S, sigma, radius, weights, seed
        self.k = len(self.models)
        self.ns, self.nc = lc.MODEL_DIMS[self.models[0]]
        self.n_dims = list(n_dims) if n_dims is not None else [3 if self.ns >= 6 else 2] * self.k

    @property
    def id(self):
        return self.name


# k, S against the kernel's layout (csrc/policy.hpp: floor(256 / k) samples per workgroup):
#   mixed 4-state k = 5: 51 samples per workgroup, samples straddle wavefronts (lanes 60..64); S = 53 is two workgroups, the
#     second nearly empty.  Quadcopter6D k = 10: 25 per workgroup at the n_x = 60 limit; S = 26.
# radius: WIDE_RADIUS of tests/linesearch_cases.py where few agents would otherwise never come near one another.
# sigma and radius are set on the CPU reference alone (scripts/policy_rollout_sensitivity.py, test_case_conditions): gains
# taken at a random nominal amid near pairs (an indefinite proximity Hessian) can make the closed loop itself unstable --
# ten quadcopters inside radius 0.6, or the heterogeneous trio inside 3.0, leave a third and more of the samples without a
# bound at any start perturbation -- so those cases get a smaller radius, and the cars and the twelve-state quadcopters
# (held near hover) a smaller perturbation.
CASES = [
    Case("car3-k2-S1", [2, 2], 1, 0.03, lc.WIDE_RADIUS, seed=1),
    Case("dint4_uni4-k5-S53", [0, 3, 0, 3, 3], 53, 0.3, 0.6, weights="per_item", seed=2),
    Case("bike5-k3-S5", [lc.BIKE] * 3, 5, 0.3, lc.WIDE_RADIUS, seed=3),
    Case("quad6-k10-S26", [4] * 10, 26, 0.6, 0.15, seed=4),
    Case("quad6_human6-k3-S6", [4, 5, 4], 6, 0.3, 1.5, n_dims=[3, 2, 3], weights="per_agent", seed=5),
    Case("quad12-k5-S4", [7] * 5, 4, 0.02, lc.WIDE_RADIUS, seed=6),
    Case("dint4-k1-S9", [0], 9, 0.3, 0.6, seed=7),
]


def make_batch(case):
    """Host arrays of a case: x0, xf, U0 scaled per model as tests/linesearch_cases.py: make_batch scales them."""
    k, ns, nc, models = case.k, case.ns, case.nc, case.models
    nd = 3 if ns >= 6 else 2
    dt = 0.1
    rng = np.random.default_rng(91000 + case.seed)
    xf = rng.normal(size=(B, k * ns)) * 1.5; x0 = rng.normal(size=(B, k * ns)) * 1.5
    x0.reshape(B, k, ns)[:, :, nd:] *= 0.1; xf.reshape(B, k, ns)[:, :, nd:] = 0.0
    U0 = rng.normal(size=(B, T, k * nc)) * max(lc.U0_NOISE[m] for m in models)
    for a, m in enumerate(models):
        if m == 4:
            U0[:, :, a * nc] += 9.80665
    if models[0] == 7:      # near hover, short steps (tests/linesearch_cases.py)
        dt = 0.05
        U0 = U0 * 1e-4; U0[:, :, 3::4] += 9.80665 * 63.0 / 2000.0
        x0.reshape(B, k, ns)[:, :, 3:] *= 0.02
    if case.weights == "shared":          # one Q, R, Qf for the batch: batch stride 0
        Q = np.eye(ns) * rng.uniform(0.5, 2.0); R = np.eye(nc); Qf = 100.0 * np.eye(ns)
        Qi, Ri, Qfi = (np.broadcast_to(M, (B, k) + M.shape) for M in (Q, R, Qf))
    else:
        shape = (k,) if case.weights == "per_agent" else (B, k)     # per_agent: stride 0 too; per_item: non-zero batch strides
        draw = lambda n, s, off: (np.stack([np.diag(rng.uniform(0.5, 2.0, n)) * s + off * rng.normal(size=(n, n))
                                            for _ in range(int(np.prod(shape)))]).reshape(shape + (n, n)))
        Q, R, Qf = draw(ns, 1.0, 0.05), draw(nc, 1.0, 0.05), draw(ns, 100.0, 1.0)
        Qi, Ri, Qfi = (np.broadcast_to(M, (B, k, M.shape[-1], M.shape[-1])) for M in (Q, R, Qf))
    S = case.S
    scale = np.ones((k, ns)) * 0.1; scale[:, :nd] = 1.0
    if models[0] == 7:
        scale[:, 3:] = 0.02
    x0s = x0[:, None, :] + case.sigma * rng.normal(size=(B, S, k * ns)) * scale.reshape(-1)
    W = W_SCALE * rng.normal(size=(B, S, T, k * ns))
    return dict(models=models, n_dims=case.n_dims, xf=xf, x0=x0, U0=U0, Q=Q, R=R, Qf=Qf, Qi=Qi, Ri=Ri, Qfi=Qfi,
                radius=float(case.radius), dt=dt, T=T, x0s=x0s, W=W)


def item_problem(batch, i):
    b = batch
    if b["models"][0] == lc.BIKE:
        return lc._BikeProblem(len(b["models"]), b["n_dims"], b["xf"][i], b["Qi"][i], b["Ri"][i], b["Qfi"][i], b["radius"], b["dt"], b["T"])
    return lc.orc.Problem(b["models"], b["n_dims"], b["xf"][i], b["Qi"][i], b["Ri"][i], b["Qfi"][i], b["radius"], b["dt"], b["T"])


def _step_cost(p):
    if isinstance(p, lc._BikeProblem):
        return p.s.dynamics, (lambda x, u, terminal=False: float(p.s.cost(x, u, terminal)))
    return p.step, (lambda x, u, terminal=False: float(p.cost(x, u, terminal)))


def nominal_and_gains(batch):
    """Per item: the oracle's rollout of (x0, U0) and its backward pass there."""
    Xn, Kn = [], []
    for i in range(B):
        p = item_problem(batch, i)
        X, _ = p.rollout(batch["x0"][i], batch["U0"][i])
        K, _ = p.backward_pass(X, batch["U0"][i], MU)
        Xn.append(np.asarray(X)); Kn.append(np.asarray(K))
    return np.stack(Xn), np.stack(Kn)


def separation(x, k, ns, n_dims):
    """Smallest distance of two agents as ProximityCost measures it (planar when every agent has the same n_dims)."""
    if k == 1:
        return np.inf
    xs = x.reshape(k, ns)
    uniform = len(set(n_dims)) == 1
    best = np.inf
    for i, j in itertools.combinations(range(k), 2):
        nd = 2 if uniform else min(n_dims[i], n_dims[j])
        best = min(best, float(np.sqrt(np.sum((xs[i, :nd] - xs[j, :nd]) ** 2))))
    return best


def ref_sample(p, batch, i, X, U, K, x0, W=None, u_lim=None):
    """The closed loop of one sample: Xs, Us, J, min_sep, goal_dist."""
    step, cost = _step_cost(p)
    k, n_dims = len(batch["models"]), batch["n_dims"]
    ns = X.shape[1] // k
    Tn = U.shape[0]
    Xs = np.zeros((Tn + 1, X.shape[1])); Us = np.zeros_like(U)
    Xs[0] = x0
    J, sep = 0.0, separation(Xs[0], k, ns, n_dims)
    for t in range(Tn):
        u = U[t] + K[t] @ (Xs[t] - X[t])
        if u_lim is not None:
            u = np.where(u < u_lim[0], u_lim[0], np.where(u > u_lim[1], u_lim[1], u))
        Us[t] = u
        J += cost(Xs[t], u)
        Xs[t + 1] = step(Xs[t], u)
        if W is not None:
            Xs[t + 1] += W[t]
        sep = min(sep, separation(Xs[t + 1], k, ns, n_dims))
    J += cost(Xs[-1], np.zeros(U.shape[1]), terminal=True)
    e = (Xs[-1] - batch["xf"][i]).reshape(k, ns)
    goal = np.array([np.sqrt(np.sum(e[a, :n_dims[a]] ** 2)) for a in range(k)])
    return dict(X=Xs, U=Us, J=J, min_sep=sep, goal_dist=goal)


def difference(got, ref):
    """Largest relative difference of a sample's five results (trajectories: by the largest reference entry)."""
    if not all(np.isfinite(np.asarray(got[key])).all() for key in ("X", "U", "J", "goal_dist")):
        return np.inf
    d = max(relerr(got["X"], ref["X"]), relerr(got["U"], ref["U"]), abs(got["J"] - ref["J"]) / max(abs(ref["J"]), 1e-300),
            relerr(got["goal_dist"], ref["goal_dist"]))
    if np.isinf(ref["min_sep"]) or np.isinf(got["min_sep"]):
        return d if got["min_sep"] == ref["min_sep"] else np.inf
    return max(d, abs(got["min_sep"] - ref["min_sep"]) / max(abs(ref["min_sep"]), 1e-300))


def bound_of(spread):
    return None if not spread <= lc.SPREAD_CAP else max(lc.TOL_PASS, lc.SPREAD_FACTOR * spread)


class CaseRef:
    """The CPU side of one case: nominal, gains, the limits, and per variant ('plain', 'W', 'u_lim') every sample's reference
    with its sensitivity to +-PERTURB relative perturbations of x0s, K, X, U."""

    def __init__(self, case):
        self.case, self.batch = case, make_batch(case)
        b = self.batch
        self.X, self.K = nominal_and_gains(b)
        self.U = b["U0"]
        self.problems = [item_problem(b, i) for i in range(B)]
        self.ref, self.spread = {}, {}
        self._run("plain")
        allU = np.stack([[self.ref["plain"][i][s]["U"] for s in range(case.S)] for i in range(B)])      # (B, S, T, m)
        flat = allU.reshape(-1, allU.shape[-1])
        self.u_lim = np.stack([np.quantile(flat, QUANTILES[0], axis=0), np.quantile(flat, QUANTILES[1], axis=0)])
        self._run("W"); self._run("u_lim")
        # the nominal's own cost, per item: what the perturbed starts are measured against
        self.J_nom = np.array([ref_sample(self.problems[i], b, i, self.X[i], self.U[i], self.K[i], self.X[i][0])["J"] for i in range(B)])

    def args(self, variant):
        return (self.batch["W"] if variant == "W" else None), (self.u_lim if variant == "u_lim" else None)

    def _run(self, variant):
        b, S = self.batch, self.case.S
        W, lim = self.args(variant)
        self.ref[variant] = [[None] * S for _ in range(B)]
        self.spread[variant] = np.zeros((B, S))
        for i in range(B):
            p = self.problems[i]
            for s in range(S):
                Ws = None if W is None else W[i, s]
                r = ref_sample(p, b, i, self.X[i], self.U[i], self.K[i], b["x0s"][i, s], Ws, lim)
                self.ref[variant][i][s] = r
                sp = 0.0
                for sg in (1.0, -1.0):
                    e = sg * lc.PERTURB
                    q = ref_sample(p, b, i, self.X[i] * (1 + e), self.U[i] * (1 - e), self.K[i] * (1 - e), b["x0s"][i, s] * (1 + e), Ws, lim)
                    sp = max(sp, difference(q, r))
                self.spread[variant][i, s] = sp

    # ---- the conditions that keep a case honest, from the reference alone
    def unchecked_fraction(self, variant):
        return float(np.mean([bound_of(v) is None for v in self.spread[variant].reshape(-1)]))

    def clamped_fraction(self):
        Us = np.stack([[self.ref["u_lim"][i][s]["U"] for s in range(self.case.S)] for i in range(B)])
        return float(np.mean((Us == self.u_lim[0]) | (Us == self.u_lim[1])))

    def near_fraction(self):
        sep = np.array([[self.ref["plain"][i][s]["min_sep"] for s in range(self.case.S)] for i in range(B)])
        return float(np.mean(sep < self.batch["radius"]))

    def moved_fraction(self):
        J = np.array([[self.ref["plain"][i][s]["J"] for s in range(self.case.S)] for i in range(B)])
        return float(np.mean(np.abs(J - self.J_nom[:, None]) >= 0.01 * np.abs(self.J_nom[:, None])))

    def figures(self):
        return dict(unchecked={v: self.unchecked_fraction(v) for v in ("plain", "W", "u_lim")},
                    max_spread={v: float(np.max(self.spread[v][self.spread[v] <= lc.SPREAD_CAP], initial=0.0)) for v in ("plain", "W", "u_lim")},
                    clamped=self.clamped_fraction(), near=self.near_fraction(), moved=self.moved_fraction())


_REFS = {}


def case_ref(case):
    """Computed once per case and shared (never modified) by the tests that need it."""
    if case.id not in _REFS:
        _REFS[case.id] = CaseRef(case)
    return _REFS[case.id]
