"""Shared by tests/test_gpu_forward.py and tests/test_forward_cases.py: the cases of the rollout check (kModeRollout) and of the
stand-alone forward pass (kModeCandidates, ProblemBatch.forward_pass), a Python mirror of launch_forward / launch_forward_big_t
(tu_forward.hip, tu_bigfwd.hip) for both modes, and the CPU side of the check -- the oracle's pass for one item, its rounding
sensitivity and the per-item bound drawn from it.  Nothing here touches the GPU.

Routes.  `wave`: k_rollout_wave<MODEL, KA> (rollout only: one model, no item list, (model, k) in the table).  `staged-packed` /
`staged`: k_forward<double, NS, NC, false>, four items per workgroup where an item is one wavefront and four items' LDS fit.
`big-pipe` / `big-nopipe`: k_forward<double, NS, NC, true, PIPE>.  What each mode can reach, from the launchers' branches: a
rollout never takes the matrix pipe (it has no gains), so it reaches wave, staged-packed, staged (twenty CarDynamics3D: n_x = 60,
an item's LDS is 44 KB and four no longer fit) and big-nopipe; the candidates mode reaches staged-packed, staged, big-pipe and
big-nopipe.

Batches are scaled as tests/linesearch_cases.py: make_batch scales x0, xf and U0 (the same draws in the same order), with three
extensions -- weights per ITEM (batch strides), an explicit n_dims, and a radius of the case's own.  ONE twelve-state quadcopter
keeps the ordinary 0.05 noise: with make_batch's LONE_QUAD12_NOISE its open-loop rollout is chaotic (spread of order 1).

Radius: WIDE_RADIUS of tests/linesearch_cases.py for clusters of at most four agents (twice that for batches of ONE item),
where otherwise hardly an item would have a near pair, 0.6 beyond.  Candidates cases of models whose closed loop under gains
taken at a random nominal amid near pairs is itself unstable (Quadcopter6D above all: tests/policy_cases.py) have a short
horizon or a small radius of their own, chosen on the CPU reference alone so that at most 5 % of a case's (item, alpha)
pairs draw no bound.  tests/test_forward_cases.py holds every case to: at least 10 % of the items have a pair inside the
radius at some step of the reference's trajectory.

The reference of every model the C oracle knows is oracle.Problem; BikeDynamics5D uses linesearch_cases._BikeProblem.

Bound of a rollout item: spread = the largest relative change of X and J under (x0, U0) perturbed by +-1e-15 relative (both sign
patterns) and by four seeded random-sign ABSOLUTE perturbations of 2**-52 (one ulp at 1: what a last-bit difference of sin / cos
amounts to, and what a relative perturbation of a state near zero cannot mimic); bound = max(1e-11, 100 x spread).  Of a
candidates (item, alpha): linesearch_cases.ItemRef.spread_of's perturbation of (X0, K, d), bound = max(1e-9, 100 x spread).  A
spread above 1e-7 draws no bound (unchecked)."""
import numpy as np

from oracle import oracle as orc
from tests import linesearch_cases as lc
from tests import policy_cases as pc
from tests.golden_util import relerr

RO_TABLE = lc.instantiation_table("tu_forward.hip", "DPILQR_TRY_RO")        # k_rollout_wave<MODEL, KA>
ROUTES = ("wave", "staged-packed", "staged", "big-pipe", "big-nopipe")
REACHABLE = {"rollout": {"wave", "staged-packed", "staged", "big-nopipe"},
             "candidates": {"staged-packed", "staged", "big-pipe", "big-nopipe"}}
ABS_PERTURB = 2.0 ** -52
N_ABS = 4
MAX_UNCHECKED = 0.05
MIN_NEAR = 0.10
MU = pc.MU
BIKE_CHECKED = 24         # BikeDynamics5D's reference is NumPy: about this many items of a case are checked


# ------------------------------------------------------------------ the launchers' branches
def forward_threads(k, groups):
    return ((k * groups + 63) // 64) * 64


def forward_on_pipe(n, m, k, threads, ngrp):
    """forward.hpp's predicate with the launch's thread count as an argument, as the source takes it (ForwardLds derives its
    own chunk width from k * ngrp)."""
    nth = ((k * ngrp + 63) // 64) * 64
    cw = max(min(2048 // m, lc.K_MAX_STAGE * nth // m, n), 1)
    rs = ((m + 14) // 16) * 16 + 1
    ns, nc = n // k, m // k
    return (m + 15) // 16 <= 2 * (threads // 64) and ngrp <= 16 and 2 * (cw * rs + 2) >= k * (ns * ns + 1 + nc * nc + ns)


def expected_route(mode, models, n_alpha=1):
    """launch_forward (tu_forward.hip) and launch_forward_big_t (tu_bigfwd.hip), branch by branch in their order, with no route
    switch set and no item list (the stand-alone entry points pass none)."""
    models = list(models)
    k = len(models)
    ns, nc = lc.MODEL_DIMS[models[0]]
    n, m = k * ns, k * nc
    rollout = mode == "rollout"
    ngrp = 1 if rollout else n_alpha              # dpilqr_rollout passes ngrp = 1
    threads = forward_threads(k, ngrp)
    assert threads <= 256, "k * n_alpha exceeds the 256-thread workgroup of the forward pass"
    lds_item = (lc.forward_lds_bytes(n, m, k, ngrp, False) + 15) & ~15
    if n > 60 or lds_item > lc.K_MAX_LDS or (not rollout and (m * n + threads - 1) // threads > lc.K_MAX_STAGE):
        pipe = not rollout and forward_on_pipe(n, m, k, threads, ngrp)
        return "big-pipe" if pipe else "big-nopipe"
    if rollout and len(set(models)) == 1 and (models[0], k) in RO_TABLE:      # hint_model(D) >= 0
        return "wave"
    ipb = 4 if threads == 64 and 4 * lds_item <= lc.K_MAX_LDS else 1
    return "staged-packed" if ipb == 4 else "staged"


def staged_threads(models, n_alpha):
    return forward_threads(len(models), n_alpha)


# ------------------------------------------------------------------ cases
class Case:
    """One parametrised case.  mode: 'rollout' | 'candidates'; weights: 'shared' | 'per_agent' (per-agent Q, R, Qf, per-item
    radius, n_dims alternating 3, 2 for six-state agents) | 'per_item' (per-item, per-agent Q, R, Qf and per-item radius);
    alphas: P1, P3, P8, P10 or OFF as alpha_set reads them (candidates)."""

    def __init__(self, mode, route, models, B, T=16, weights="shared", alphas=None, n_dims=None, radius=None, noise=1.0, seed=0):
        self.mode, self.route, self.models, self.B, self.T, self.weights = mode, route, list(models), B, T, weights
        self.alphas, self.noise, self.seed = alphas, noise, seed
        self.k = len(self.models)
        self.uniform = len(set(self.models)) == 1
        self.ns, self.nc = lc.MODEL_DIMS[self.models[0]]
        self.n_dims = None if n_dims is None else list(n_dims)
        self.radius = radius if radius is not None else (2 * lc.WIDE_RADIUS if B == 1 else lc.WIDE_RADIUS if self.k <= 4 else 0.6)

    @property
    def id(self):
        mdl = f"m{self.models[0]}k{self.k}" if self.uniform else "mix" + "_".join(map(str, self.models[:6])) + (f"_k{self.k}" if self.k > 6 else "")
        tail = ("-" + self.weights.replace("_", "") if self.weights != "shared" else "") + (f"-{self.alphas}" if self.alphas else "")
        return f"{self.mode[:4]}-{self.route}-{mdl}-B{self.B}-T{self.T}{tail}"

    def alpha_values(self):
        return alpha_set(self.alphas)

    def expected_route(self):
        return expected_route(self.mode, self.models, len(self.alpha_values()) if self.mode == "candidates" else 1)

    def checked(self):
        """Every item; a stride of them for BikeDynamics5D (NumPy reference).  Items 0, B - 2 and B - 1 always."""
        B = self.B
        stride = max(1, B // BIKE_CHECKED) if self.models[0] == lc.BIKE else 1
        return sorted(set(range(0, B, stride)) | {0, max(B - 2, 0), B - 1})


def alpha_set(name):
    """Prefixes of the solver's table (P1, P3, P10; Pn: its first n), or OFF: two values off the table, the first alpha = 0."""
    if name == "OFF":
        return np.array([0.0, 0.37])
    return orc.alphas()[:int(name[1:])]


FAMILY_K = {0: 13, 3: 9, 4: 9, 1: 4, 2: 3, lc.BIKE: 3, 5: 4, 6: 5, 7: 3}      # one k per model for the per-family variants


def rollout_cases():
    cases = []
    seed = 0

    def add(route, models, B, **kw):
        nonlocal seed
        seed += 1
        cases.append(Case("rollout", route, models, B, seed=seed, **kw))
    for m, k in sorted(RO_TABLE):      # one full workgroup (four wavefronts of 64 // k items) plus one item
        add("wave", [m] * k, 4 * (64 // k) + 1)
    for m, k in FAMILY_K.items():
        add("wave", [m] * k, max(64 // k - 1, 1))      # a wavefront one item short
        add("wave", [m] * k, 1)
        add("wave", [m] * k, 64 // k + 1, T=1)
        add("wave", [m] * k, 64 // k + 1, T=2)         # the t + 1 < T prefetch
        add("wave", [m] * k, 4 * (64 // k) + 1, weights="per_agent")
    # the generic route: mixed models (no model hint), and one uniform batch outside the table
    for models in ([1, 5, 6], [4, 1], [0, 3, 0, 3, 3, 0], [5, 6, 4, 1], [7, 8]):
        add("staged-packed", models, 9)
        add("staged-packed", models, 5, weights="per_item")
    add("staged-packed", [1] * 7, 9)
    add("staged-packed", [1] * 7, 5, weights="per_item", T=2)
    add("staged-packed", [0, 3, 0], 1, T=1)
    add("staged", [2] * 20, 3)                         # four items' LDS no longer fit: one item per workgroup
    # large clusters (n_x > 60)
    add("big-nopipe", [3] * 16, 3)
    add("big-nopipe", [0] * 18, 3, T=12)
    add("big-nopipe", [4] * 11, 3, T=12)
    add("big-nopipe", [7] * 6, 3, radius=lc.WIDE_RADIUS)
    add("big-nopipe", [7] * 14 + [8] * 6, 3, T=4, n_dims=[3] * 14 + [2] * 6)      # config 5's cluster at a short horizon
    add("big-nopipe", [1] * 12, 3, T=2, weights="per_agent")
    return cases


def candidates_cases():
    cases = []
    seed = 500

    def add(route, models, B, alphas, **kw):
        nonlocal seed
        seed += 1
        cases.append(Case("candidates", route, models, B, alphas=alphas, seed=seed, **kw))
    # four items per workgroup, B = 1 mod 4
    add("staged-packed", [0] * 3, 9, "P10")
    add("staged-packed", [0] * 6, 5, "P10")                                   # 60 of a wavefront's 64 lanes
    add("staged-packed", [3] * 5, 13, "P10", weights="per_agent")
    add("staged-packed", [5] * 3, 5, "P3", weights="per_agent", T=8)             # n_dims 3, 2, 3: the pair (0, 2) is over three dimensions
    add("staged-packed", [1, 5, 6], 9, "P10")
    add("staged-packed", [0, 3, 0, 3, 3, 0], 9, "P1", weights="per_item")
    add("staged-packed", [2] * 4, 5, "OFF", T=4, radius=0.6)
    add("staged-packed", [lc.BIKE] * 2, 5, "P3", T=12, radius=0.6)
    add("staged-packed", [7] * 2, 5, "P1")
    add("staged-packed", [5, 6, 4, 1], 1, "P10", T=8, radius=0.6)
    add("staged-packed", [3] * 1, 17, "P3")
    # one item per workgroup of 128, 192, 256 threads
    add("staged", [0] * 7, 3, "P10")                                          # 70 lanes: 128 threads
    add("staged", [0, 3] * 4 + [0], 2, "P10", weights="per_item")             # 90: 128
    add("staged", [4] * 10, 3, "P10", T=4)                                    # 100: 128, n_x = 60
    add("staged", [3] * 13, 3, "P10")                                         # 130: 192
    add("staged", [0] * 15, 2, "P10", weights="per_agent", T=12)              # 150: 192
    add("staged", [2] * 20, 3, "P10", T=8)                                    # 200: 256
    # large clusters on the matrix pipe
    add("big-pipe", [3] * 16, 3, "P10")
    add("big-pipe", [7] * 5, 5, "P10", radius=1.5)                                     # n_x = 60: K[t] is beyond kMaxStage elements per thread
    add("big-pipe", [4] * 10, 5, "P1", T=4)                                   # the same clause with one alpha: 64 threads, two row tiles
    add("big-pipe", [7] * 6, 3, "P1")
    add("big-pipe", [4] * 11, 3, "P10", T=4, weights="per_agent")
    add("big-pipe", [7] * 14 + [8] * 6, 2, "P10", T=4, n_dims=[3] * 14 + [2] * 6)
    add("big-pipe", [2] * 30, 2, "P8", T=8)                                   # ten alphas would be 300 threads: the longest prefix that fits 256
    # ... and off it: more than two row tiles of sixteen controls per wavefront
    add("big-nopipe", [3] * 17, 3, "P1")
    add("big-nopipe", [4] * 11, 3, "P3", T=4)
    add("big-nopipe", [0] * 18, 3, "OFF", T=12)
    add("big-nopipe", [1] * 12, 3, "P1", T=10, weights="per_agent")
    add("big-nopipe", [7] * 14 + [8] * 6, 3, "P1", T=4, n_dims=[3] * 14 + [2] * 6)      # what ilqrSolver._forward_pass launches at config 5
    add("big-nopipe", [0, 3] * 9, 2, "P3", T=8, weights="per_item")
    return cases


ROLLOUT_CASES = rollout_cases()
CANDIDATES_CASES = candidates_cases()


# one case per route and mode for the checks that hold whatever the numbers are (position independence, guard rows); the cases an
# item is poisoned in (wave; packed in both modes); and the problems ilqrSolver._forward_pass is called on
ROUTE_SAMPLES = ["roll-wave-m3k9-B29-T16-peragent", "roll-staged-packed-mix0_3_0_3_3_0-B5-T16-peritem", "roll-staged-m2k20-B3-T16",
                 "roll-big-nopipe-m4k11-B3-T12", "cand-staged-packed-m3k5-B13-T16-peragent-P10", "cand-staged-m0k7-B3-T16-P10",
                 "cand-big-pipe-m3k16-B3-T16-P10", "cand-big-nopipe-m3k17-B3-T16-P1"]
POISON_SAMPLES = ["roll-wave-m3k9-B29-T16", "roll-staged-packed-mix5_6_4_1-B9-T16", "cand-staged-packed-m3k5-B13-T16-peragent-P10"]
PUBLIC_PATH_CASES = ["cand-big-nopipe-m3k17-B3-T16-P1", "cand-big-nopipe-mix7_7_7_7_7_7_k20-B3-T4-P1"]


def by_id(case_id):
    return next(c for c in ROLLOUT_CASES + CANDIDATES_CASES if c.id == case_id)


# ------------------------------------------------------------------ batches
def make_batch(case):
    """Host arrays of a case; x0, xf, U0 drawn and scaled as tests/linesearch_cases.py: make_batch."""
    B, models, k, ns, nc = case.B, case.models, case.k, case.ns, case.nc
    nd = 3 if ns >= 6 else 2
    m0 = models[0]
    T, dt = case.T, 0.1
    rng = np.random.default_rng(83000 + case.seed)
    xf = rng.normal(size=(B, k * ns)) * 1.5; x0 = rng.normal(size=(B, k * ns)) * 1.5
    x0.reshape(B, k, ns)[:, :, nd:] *= 0.1; xf.reshape(B, k, ns)[:, :, nd:] = 0.0
    U0 = rng.normal(size=(B, T, k * nc)) * max(lc.U0_NOISE[m] for m in models) * case.noise
    for a, m in enumerate(models):
        if m == 4:
            U0[:, :, a * nc] += 9.80665
    if m0 == 7:      # near hover, few and short steps (tests/linesearch_cases.py)
        T = min(T, 6); dt = 0.05
        U0 = U0[:, :T] * 1e-4; U0[:, :, 3::4] += 9.80665 * 63.0 / 2000.0
        x0.reshape(B, k, ns)[:, :, 3:] *= 0.02
    n_dims = [nd] * k if case.n_dims is None else case.n_dims
    if case.weights == "shared":
        Q = np.eye(ns) * rng.uniform(0.5, 2.0); R = np.eye(nc); Qf = 100.0 * np.eye(ns)
        radius = np.full(B, float(case.radius))
    else:
        lead = (k,) if case.weights == "per_agent" else (B, k)
        draw = lambda n, s, off: np.stack([np.diag(rng.uniform(0.5, 2.0, n)) * s + off * rng.normal(size=(n, n))
                                           for _ in range(int(np.prod(lead)))]).reshape(lead + (n, n))
        Q, R, Qf = draw(ns, 1.0, 0.05), draw(nc, 1.0, 0.05), draw(ns, 100.0, 1.0)
        radius = rng.uniform(0.4, 0.9, size=B) * (case.radius / 0.6)
        if ns == 6 and case.n_dims is None:
            n_dims = [3 if a % 2 == 0 else 2 for a in range(k)]
    return dict(models=models, n_dims=n_dims, xf=xf, x0=x0, U0=U0, Q=Q, R=R, Qf=Qf, radius=radius, dt=dt, T=T,
                per_item=case.weights == "per_item")


def item_problem(batch, i):
    b = batch
    Q, R, Qf = ((M[i] if b["per_item"] else M) for M in (b["Q"], b["R"], b["Qf"]))
    if b["models"][0] == lc.BIKE:
        return lc._BikeProblem(len(b["models"]), b["n_dims"], b["xf"][i], Q, R, Qf, float(b["radius"][i]), b["dt"], b["T"])
    return orc.Problem(b["models"], b["n_dims"], b["xf"][i], Q, R, Qf, float(b["radius"][i]), b["dt"], b["T"])


def has_near_pair(X, k, ns, n_dims, radius):
    """Some pair of agents is inside the radius at some step, as ProximityCost measures distance (planar when every agent has
    the same n_dims, over min(n_dims) of the pair otherwise)."""
    if k < 2:
        return False
    P = np.asarray(X).reshape(-1, k, ns)[:, :, :3]
    i, j = np.triu_indices(k, 1)
    nd = np.asarray(n_dims)
    pair_nd = np.full(i.size, 2) if len(set(n_dims)) == 1 else np.minimum(nd[i], nd[j])
    mask = (np.arange(3)[None, :] < pair_nd[:, None])
    d2 = (((P[:, i, :] - P[:, j, :]) ** 2) * mask[None]).sum(-1)
    return bool((np.sqrt(d2) < radius).any())


def bound_rollout(spread):
    return None if not spread <= lc.SPREAD_CAP else max(pc.TOL_ROLLOUT, lc.SPREAD_FACTOR * spread)


def bound_pass(spread):
    return None if not spread <= lc.SPREAD_CAP else max(lc.TOL_PASS, lc.SPREAD_FACTOR * spread)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


class RolloutRef:
    """The CPU side of a rollout case: per checked item the oracle's X, J, the spread and the bound."""

    def __init__(self, case):
        self.case, self.batch = case, make_batch(case)
        b = self.batch
        self.idx = case.checked()
        self.X, self.J, self.spread, self.bound, self.near = {}, {}, {}, {}, {}
        for i in self.idx:
            p = item_problem(b, i)
            x0, U0 = b["x0"][i], b["U0"][i]
            X, J = p.rollout(x0, U0)
            self.X[i], self.J[i] = np.array(X), float(J)
            self.spread[i] = self._spread(p, x0, U0, X, J, i)
            self.bound[i] = bound_rollout(self.spread[i])
            self.near[i] = has_near_pair(X, case.k, case.ns, b["n_dims"], float(b["radius"][i]))

    def _spread(self, p, x0, U0, X, J, i):
        if not (np.isfinite(J) and np.isfinite(X).all()):
            return np.inf
        rng = np.random.default_rng(5000 * self.case.seed + i)
        pert = [(x0 * (1 + e), U0 * (1 - e)) for e in (lc.PERTURB, -lc.PERTURB)]
        for _ in range(N_ABS):
            pert.append((x0 + ABS_PERTURB * rng.choice([-1.0, 1.0], size=x0.shape), U0 + ABS_PERTURB * rng.choice([-1.0, 1.0], size=U0.shape)))
        s = 0.0
        for xp, Up in pert:
            Xp, Jp = p.rollout(xp, Up)
            if not (np.isfinite(Jp) and np.isfinite(Xp).all()):
                return np.inf
            s = max(s, relerr(Xp, X), rel(float(Jp), J))
        return s

    def unchecked_fraction(self):
        return float(np.mean([self.bound[i] is None for i in self.idx]))

    def near_fraction(self):
        return float(np.mean([self.near[i] for i in self.idx]))

    def max_spread(self):
        return max([self.spread[i] for i in self.idx if self.bound[i] is not None], default=0.0)


class PassRef(lc.ItemRef):
    """linesearch_cases.ItemRef without the search: the nominal (X0, J0) is the oracle's rollout, every alpha is evaluated by
    candidate(i), spread_of(i) is ItemRef's perturbation of (X0, K, d)."""

    def __init__(self, p, x0, U0, K, d, alphas):
        self.p, self.U0, self.K, self.d, self.alphas = p, np.asarray(U0, dtype=np.float64), np.asarray(K), np.asarray(d), alphas
        self.X0, self.J0 = p.rollout(x0, U0)
        self.cand = {}


class CandidatesRef:
    """The CPU side of a candidates case.  Nominal and gains of EVERY item are the oracle's (its rollout of (x0, U0) and its
    backward pass there at mu = 1, as tests/policy_cases.py: nominal_and_gains); per checked (item, alpha) the oracle's Xn, Un,
    Jn, the spread and the bound."""

    def __init__(self, case):
        self.case, self.batch = case, make_batch(case)
        b = self.batch
        self.alphas = case.alpha_values()
        self.idx = case.checked()
        Xs, Ks, ds = [], [], []
        self.item = {}
        for i in range(case.B):
            p = item_problem(b, i)
            X, _ = p.rollout(b["x0"][i], b["U0"][i])
            K, d = p.backward_pass(X, b["U0"][i], MU)
            Xs.append(np.array(X)); Ks.append(np.array(K)); ds.append(np.array(d))
            if i in self.idx:
                self.item[i] = PassRef(p, b["x0"][i], b["U0"][i], K, d, self.alphas)
        self.X, self.K, self.d = np.stack(Xs), np.stack(Ks), np.stack(ds)
        self.U = b["U0"]
        self.spread = {(i, g): self.item[i].spread_of(g) for i in self.idx for g in range(len(self.alphas))}
        self.bound = {key: bound_pass(s) for key, s in self.spread.items()}
        self.near = {i: has_near_pair(self.X[i], case.k, case.ns, b["n_dims"], float(b["radius"][i])) for i in self.idx}

    def ref(self, i, g):
        return self.item[i].candidate(g)

    def unchecked_fraction(self):
        return float(np.mean([v is None for v in self.bound.values()]))

    def near_fraction(self):
        return float(np.mean([self.near[i] for i in self.idx]))

    def max_spread(self):
        return max([s for key, s in self.spread.items() if self.bound[key] is not None], default=0.0)

    def costs_differ(self, i):
        """The reference's J differs between two of the case's alphas; with ONE alpha, between it and the nominal's own cost
        (the pass at alpha = 0)."""
        Js = [self.item[i].J(g) for g in range(len(self.alphas))]
        if len(Js) == 1:
            Js.append(self.item[i].J0)
        return len({repr(float(v)) for v in Js}) >= 2


_REFS = {}


def case_ref(case):
    """Computed once per case and shared (never modified) by the tests that need it."""
    if case.id not in _REFS:
        _REFS[case.id] = RolloutRef(case) if case.mode == "rollout" else CandidatesRef(case)
    return _REFS[case.id]
