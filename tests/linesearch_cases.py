"""Shared by tests/test_gpu_linesearch.py and scripts/linesearch_oracle_sensitivity.py: the parametrised cases of the
line-search check, their seeded batches, and the CPU side of the check -- the oracle's own line search for one item, its
rounding sensitivity, and the per-item bound drawn from it.  Nothing here touches the GPU.

The reference of every model the C oracle knows is oracle.Problem.  BikeDynamics5D is a device model only (the C oracle
has no five-state family), so its reference is written out here in NumPy from the model's equations -- one classical RK4
step of dt per horizon step, forward-Euler Jacobians -- under oracle/numpy_port.py's cost and passes."""
import re
from pathlib import Path

import numpy as np

from oracle import numpy_port
from oracle import oracle as orc
from tests.golden_util import relerr

CSRC = Path(__file__).resolve().parent.parent / "dpilqr_amd" / "csrc"

TOL_PASS = 1e-9           # the project's per-pass tolerance
SPREAD_FACTOR = 100.0     # the ratio TOL_PASS has to the 1e-11 rollout tolerance
SPREAD_CAP = 1e-7         # an item whose own sensitivity exceeds this draws no bound
PERTURB = 1e-15
TOL_SOLVE = 1e-3          # ProblemBatch.solve's default tol: linesearch_decide's convergence test
TEAM_MAX = 1024           # launches of at most this many items take the team kernel where one is instantiated (tu_lsteam.hip)

BIKE = 10
MODEL_DIMS = dict(orc.MODEL_DIMS); MODEL_DIMS[BIKE] = (5, 2)
K_MAX_LDS, K_MAX_STAGE = 160 * 1024, 16      # launch.hpp: kMaxLds; forward.hpp: kMaxStage (tests/test_linesearch_cases.py holds them to the sources)


def instantiation_table(unit, try_macro):
    """The (model, k) pairs a launcher tries, read from its source: every use of `try_macro`(kModel, KA) outside a #define, with
    the unit's own helper macros (DPILQR_WAVE_10(MODEL) ...) expanded; model names resolved by models.hpp's enum."""
    enum = re.search(r"enum Model : int \{(.*?)\};", (CSRC / "models.hpp").read_text(), re.S).group(1)
    ids = {name: int(v) for name, v in re.findall(r"(k\w+)\s*=\s*(\d+)", re.sub(r"//.*", "", enum))}
    text = re.sub(r"\\\n", " ", re.sub(r"//.*", "", (CSRC / unit).read_text()))
    defines = dict(re.findall(r"^\s*#define\s+(DPILQR_\w+)\(MODEL\)\s+(.*)$", text, re.M))
    body = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    for _ in range(4):      # helper macros nest (DPILQR_WAVE_15 uses DPILQR_WAVE_10)
        for name, exp in defines.items():
            body = re.sub(name + r"\((k\w+)\)", lambda mo, exp=exp: exp.replace("MODEL", mo.group(1)), body)
    return {(ids[name], int(ka)) for name, ka in re.findall(try_macro + r"\((k\w+),\s*(\d+)\)", body)}


WAVE_TABLE = instantiation_table("tu_forward.hip", "DPILQR_TRY_WAVE")        # k_linesearch_wave<MODEL, KA>
TEAM_TABLE = instantiation_table("tu_lsteam.hip", "DPILQR_TRY_LSTEAM")       # k_linesearch_team<MODEL, KA>
# U0 noise per model: 0.05 is test_fuzz_shapes_against_oracle's.  Raised for CarDynamics3D and BikeDynamics5D, where the oracle
# alone then rejects the first candidate on 10 % of the items and more (profiles/linesearch_oracle_sensitivity.txt).
U0_NOISE = {0: 0.05, 3: 0.05, 4: 0.05, 2: 0.5, 5: 0.05, 1: 0.05, 6: 0.05, 7: 0.05, 8: 0.05, BIKE: 2.0}
# The double integrators and the linearised human are LINEAR, the twelve-state quadcopter is held near hover: with radius 0.6
# their line search from mu = 1 all but always accepts the first candidate, at any U0 noise -- only the proximity cost bends the
# problem.  Clusters of these models (the double integrator up to seven agents: beyond, 0.6 is enough) get WIDE_RADIUS, so that
# many pairs are near and the oracle alone rejects the first candidate on 10 % of the items and more.
WIDE_RADIUS_MODELS = {0: 7, 1: 99, 6: 99, 7: 99}
WIDE_RADIUS = 3.0
# ONE agent of a linear model is an exactly linear-quadratic problem: the full step lowers the cost by construction, so the floor
# "10 % of the items accept a later candidate" cannot be asked of these cases.  It is asked of every other one.
LINEAR_MODELS = (0, 1, 6)
# ONE twelve-state quadcopter has no pair at all: only its own dynamics bend the problem, and they do once the controls leave
# hover far enough -- U0 noise 40 (x 1e-4 on controls with gains of 5e4) has the oracle alone reject the first candidate on 29 % of
# the items with no item unchecked; 30 gives 6 %, 50 leaves 4.5 % of the items without a bound.
LONE_QUAD12_NOISE = 40.0


# ------------------------------------------------------------------ cases
class Case:
    """One parametrised case: `models` (k,), B items, which items are checked, and the route the sizes select."""

    def __init__(self, route, models, B, stride, per_agent=False, T=16, seed=0):
        self.route, self.models, self.B, self.stride, self.per_agent, self.T, self.seed = route, list(models), B, stride, per_agent, T, seed
        self.k = len(self.models)
        self.uniform = len(set(self.models)) == 1

    @property
    def id(self):
        m = f"m{self.models[0]}k{self.k}" if self.uniform else "mix" + "_".join(map(str, self.models))
        return f"{self.route}-{m}-B{self.B}" + ("-peragent" if self.per_agent else "")

    def checked(self):
        idx = list(range(0, self.B, self.stride))
        return idx if idx[-1] == self.B - 1 else idx + [self.B - 1]

    def later_candidates_expected(self):
        return not (self.k == 1 and self.models[0] in LINEAR_MODELS)

    def wide_radius(self):
        return self.k >= 2 and all(self.k <= WIDE_RADIUS_MODELS.get(m, 0) for m in self.models)

    def leaves_staged_forward(self):
        """launch_forward's first branch (tu_forward.hip), taken before either table is tried: the large-cluster k_forward serves
        the launch when n_x > 60, when an item's LDS exceeds kMaxLds, or when K[t] is more than kMaxStage elements per thread."""
        ns, nc = MODEL_DIMS[self.models[0]]
        n, m, k = self.k * ns, self.k * nc, self.k
        threads = ((k * 10 + 63) // 64) * 64
        lds_item = (forward_lds_bytes(n, m, k, 10, False) + 15) & ~15
        return n > 60 or lds_item > K_MAX_LDS or (m * n + threads - 1) // threads > K_MAX_STAGE

    def expected_route(self):
        """What launch_forward (tu_forward.hip) selects for this batch in line-search mode, from the sizes alone."""
        if self.leaves_staged_forward():
            return "big"
        if not self.uniform:
            return "generic"
        key = (self.models[0], self.k)
        if self.B <= TEAM_MAX and key in TEAM_TABLE:
            return "team"
        return "wave" if key in WAVE_TABLE else "generic"


def all_cases():
    cases = []
    seed = 0
    def add(*a, **kw):
        nonlocal seed
        seed += 1
        cases.append(Case(*a, seed=seed, **kw))
    for m, kmax in {0: 15, 3: 15, 4: 10, 1: 6, 2: 6, BIKE: 6, 5: 6, 6: 6, 7: 5}.items():
        for k in range(1, kmax + 1):
            if (m, k) in TEAM_TABLE:
                add("wave", [m] * k, 1100, 11)          # more than 1024 items: the team is not taken
            else:       # (five twelve-state quadcopters: K[t] is 19 elements per thread, the large-cluster k_forward serves them)
                add("wave" if (m, k) in WAVE_TABLE else "big", [m] * k, 260, 4)
    for m, k in [(0, 7), (0, 13), (3, 11), (3, 15), (4, 7), (4, 10)]:      # two / three wavefronts per item, a ragged batch
        add("wave", [m] * k, 37, 1)
    for m in (0, 3, 4, 1, 2):
        for k in range(1, 7):
            add("team", [m] * k, 700, 7)
    for models in ([1, 5, 6], [4, 1], [0, 3, 0, 3, 3, 0], [5, 6, 4, 1]):
        add("generic", models, 260, 4)
    add("big", [3] * 16, 260, 4)      # beyond the wave tables; n_x = 64 is beyond the LDS-staged k_forward too
    for m, k, T in [(3, 16, 20), (0, 18, 12), (4, 11, 15), (7, 6, 8), (1, 12, 10)]:
        add("big", [m] * k, 3, 1, T=T)
    seed = 122      # the per-agent cases draw their seeds from a range of their own
    for m, k, B in [(0, 5, 1100), (3, 4, 1100), (4, 3, 1100), (2, 6, 1100), (4, 8, 260), (0, 12, 260), (7, 2, 260), (5, 4, 260),
                    (BIKE, 3, 260)]:
        add("wave", [m] * k, B, 11 if B > 1024 else 4, per_agent=True)
    for m, k in [(0, 5), (3, 6), (4, 4), (1, 3), (2, 5)]:
        add("team", [m] * k, 700, 7, per_agent=True)
    return cases


def forward_on_pipe(n, m, k, ngrp=10):
    """forward.hpp's predicate of the same name with tu_bigfwd.hip's thread count, from its inputs."""
    nth = ((k * ngrp + 63) // 64) * 64
    c = min(2048 // m, K_MAX_STAGE * nth // m, n)
    cw = max(c, 1)
    rs = ((m + 14) // 16) * 16 + 1
    ns, nc = n // k, m // k
    return (m + 15) // 16 <= 2 * (nth // 64) and ngrp <= 16 and 2 * (cw * rs + 2) >= k * (ns * ns + 1 + nc * nc + ns)


def forward_lds_bytes(n, m, k, ngrp=10, kdirect=False):
    """forward.hpp's function of the same name (ForwardLds::total in fp64)."""
    ev = lambda x: (x + 1) & ~1
    npairs = k * (k - 1) // 2
    nth = ((k * ngrp + 63) // 64) * 64
    cw = max(min(2048 // m, K_MAX_STAGE * nth // m, n), 1); rs = ((m + 14) // 16) * 16 + 1; mk = ((m + 15) // 16) * 16
    kt = 2 * (cw * rs + 2) if kdirect else 2 * m * n
    o = ev(kt + 2 * m + 4 * ngrp * n + 2 * ngrp * k + 2 * ngrp * max(npairs, 1) + ngrp + 2) + (ngrp * mk if kdirect else 0)
    return 8 * ev(o)


def big_sweep_lds_bytes(k, ns, nc):
    """riccati_big.hpp: BigLds::total in fp64 -- what the large-cluster sweep asks of allow_lds (launch.hpp)."""
    ev = lambda x: (x + 1) & ~1
    n, m, npairs = k * ns, k * nc, k * (k - 1) // 2
    mk = ((m + 15) // 16) * 16
    o = (ev(k * ns * (ns + nc)) + ev(k * ns * ns) + ev(k * nc * nc) + 2 * ev(n) + ev(m) + ev(npairs * 3) + ev(npairs * 9) + ev(k * 9)
         + ev(k * 3) + ev(max(mk * (mk + 2), k * ns * (ns + nc), 16 * 544)) + 3 * mk + 4)
    return 8 * ev(o)


# ------------------------------------------------------------------ batches
def make_batch(case, B=None):
    """The seeded batch of a case, scaled as test_fuzz_shapes_against_oracle scales x0, xf, U0: returns a dict of host arrays."""
    B = case.B if B is None else B
    models, k = case.models, case.k
    ns, nc = MODEL_DIMS[models[0]]
    nd = 3 if ns >= 6 else 2
    m0 = models[0]
    T, dt = case.T, 0.1
    rng = np.random.default_rng(77000 + case.seed)
    xf = rng.normal(size=(B, k * ns)) * 1.5; x0 = rng.normal(size=(B, k * ns)) * 1.5
    x0.reshape(B, k, ns)[:, :, nd:] *= 0.1; xf.reshape(B, k, ns)[:, :, nd:] = 0.0
    noise = LONE_QUAD12_NOISE if (m0, k) == (7, 1) else max(U0_NOISE[m] for m in models)
    U0 = rng.normal(size=(B, T, k * nc)) * noise
    for a, m in enumerate(models):
        if m == 4:
            U0[:, :, a * nc] += 9.80665
    if m0 == 7:   # the free rigid body tumbles chaotically in an open-loop rollout: stay near hover, few steps, short steps
        T = min(T, 6); dt = 0.05
        U0 = U0[:, :T] * 1e-4; U0[:, :, 3::4] += 9.80665 * 63.0 / 2000.0
        x0.reshape(B, k, ns)[:, :, 3:] *= 0.02
    n_dims = [nd] * k
    if case.per_agent:
        Q = np.stack([np.diag(rng.uniform(0.5, 2.0, ns)) + 0.05 * rng.normal(size=(ns, ns)) for _ in range(k)])
        R = np.stack([np.diag(rng.uniform(0.5, 2.0, nc)) + 0.05 * rng.normal(size=(nc, nc)) for _ in range(k)])
        Qf = np.stack([100.0 * np.eye(ns) + rng.normal(size=(ns, ns)) for _ in range(k)])
        radius = rng.uniform(0.4, 0.9, size=B) * (WIDE_RADIUS / 0.6 if case.wide_radius() else 1.0)
        if ns == 6:
            n_dims = [3 if a % 2 == 0 else 2 for a in range(k)]
    else:
        Q = np.eye(ns) * rng.uniform(0.5, 2.0); R = np.eye(nc); Qf = 100.0 * np.eye(ns)
        radius = np.full(B, WIDE_RADIUS if case.wide_radius() else 0.6)
    return dict(models=models, n_dims=n_dims, xf=xf, x0=x0, U0=U0, Q=Q, R=R, Qf=Qf, radius=radius, dt=dt, T=T)


# ------------------------------------------------------------------ the CPU reference of one item
class _BikeJoint:
    """k BikeDynamics5D agents, x = [p_x, p_y, v, theta, phi], u = [a, rho]: p_x' = v cos theta, p_y' = v sin theta, v' = a,
    theta' = v tan phi, phi' = rho."""

    def __init__(self, k, dt):
        self.k, self.dt, self.n_s, self.n_c = k, float(dt), 5, 2
        self.n_x, self.n_u = 5 * k, 2 * k

    @staticmethod
    def _f(x, u):
        return np.stack([x[:, 2] * np.cos(x[:, 3]), x[:, 2] * np.sin(x[:, 3]), u[:, 0], x[:, 2] * np.tan(x[:, 4]), u[:, 1]], axis=1)

    def __call__(self, x, u):
        x, u, dt = x.reshape(self.k, 5), u.reshape(self.k, 2), self.dt
        k0 = self._f(x, u); k1 = self._f(x + 0.5 * k0 * dt, u); k2 = self._f(x + 0.5 * k1 * dt, u); k3 = self._f(x + k2 * dt, u)
        return (x + dt * (k0 + 2.0 * k1 + 2.0 * k2 + k3) / 6.0).reshape(-1)

    def linearize(self, x, u):
        A = np.eye(self.n_x); B = np.zeros((self.n_x, self.n_u))
        for i in range(self.k):
            _, _, v, th, ph = x[5 * i:5 * i + 5]
            Ac = np.zeros((5, 5))
            Ac[0, 2], Ac[0, 3] = np.cos(th), -v * np.sin(th)
            Ac[1, 2], Ac[1, 3] = np.sin(th), v * np.cos(th)
            Ac[3, 2], Ac[3, 4] = np.tan(ph), v * (np.tan(ph) ** 2 + 1.0)
            A[5 * i:5 * i + 5, 5 * i:5 * i + 5] += self.dt * Ac
            B[5 * i + 2, 2 * i] = self.dt; B[5 * i + 4, 2 * i + 1] = self.dt
        return A, B


class _BikeProblem:
    """oracle.Problem's pass interface for BikeDynamics5D clusters, on oracle/numpy_port.py."""

    def __init__(self, k, n_dims, xf, Q, R, Qf, radius, dt, T):
        dyn = _BikeJoint(k, dt)
        self.s = numpy_port.Solver(dyn, numpy_port.GameCost(xf, Q, R, Qf, radius, n_dims, 5, 2), T)

    def rollout(self, x0, U):
        X, J = self.s.rollout(np.asarray(x0, dtype=np.float64).reshape(-1), np.asarray(U, dtype=np.float64))
        return X, float(J)

    def backward_pass(self, X, U, mu):
        self.s.mu = float(mu)
        return self.s.backward_pass(np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64))

    def forward_pass(self, X, U, K, d, alpha):
        Xn, Un, J = self.s.forward_pass(np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64), np.asarray(K), np.asarray(d),
                                        float(alpha))
        return Xn, Un, float(J)


def item_problem(batch, i):
    b = batch
    if b["models"][0] == BIKE:
        return _BikeProblem(len(b["models"]), b["n_dims"], b["xf"][i], b["Q"], b["R"], b["Qf"], float(b["radius"][i]), b["dt"], b["T"])
    return orc.Problem(b["models"], b["n_dims"], b["xf"][i], b["Q"], b["R"], b["Qf"], float(b["radius"][i]), b["dt"], b["T"])


class ItemRef:
    """The oracle's own line search of one item with the given gains: X0, J0, the costs J_i of the candidates it evaluates (up
    to its first accepted one, all ten on a failed search), the trajectories of the last evaluated candidate, that pass's
    rounding sensitivity `spread`, and the item's bound (None: unchecked)."""

    def __init__(self, p, x0, U0, K, d, alphas):
        self.p, self.U0, self.K, self.d, self.alphas = p, np.asarray(U0, dtype=np.float64), np.asarray(K), np.asarray(d), alphas
        self.X0, self.J0 = p.rollout(x0, U0)
        self.cand = {}
        self.acc = -1
        for i in range(len(alphas)):
            if self.J(i) < self.J0:      # strict <, NaN rejects (control.py:183)
                self.acc = i
                break
        self.n_eval = self.acc + 1 if self.acc >= 0 else len(alphas)
        self.Js = [self.J(i) for i in range(self.n_eval)]
        self.spread = self.spread_of(self.n_eval - 1)
        self.bound = self.bound_of(self.spread)

    def candidate(self, i):
        if i not in self.cand:
            self.cand[i] = self.p.forward_pass(self.X0, self.U0, self.K, self.d, self.alphas[i])
        return self.cand[i]

    def J(self, i):
        return self.candidate(i)[2]

    def spread_of(self, i):
        """Largest relative change of X, U, J of candidate i's pass under +-1e-15 relative perturbations of X0, K, d."""
        X, U, J = self.candidate(i)
        if not (np.isfinite(J) and np.isfinite(X).all() and np.isfinite(U).all()):
            return np.inf
        s = 0.0
        for sg in (1.0, -1.0):
            e = sg * PERTURB
            Xp, Up, Jp = self.p.forward_pass(self.X0 * (1 + e), self.U0, self.K * (1 - e), self.d * (1 + e), self.alphas[i])
            if not (np.isfinite(Jp) and np.isfinite(Xp).all() and np.isfinite(Up).all()):
                return np.inf
            s = max(s, relerr(Xp, X), relerr(Up, U), abs(Jp - J) / max(abs(J), 1e-300))
        return s

    @staticmethod
    def bound_of(spread):
        return None if not spread <= SPREAD_CAP else max(TOL_PASS, SPREAD_FACTOR * spread)

    def margin(self, i):
        """|J_i - J0| / |J0|: how far candidate i is from the accept threshold."""
        return abs(self.J(i) - self.J0) / abs(self.J0)

    def near_tie(self, bound, upto=None):
        """A candidate the oracle evaluated (or any up to `upto`) lies within `bound` of J0, or the accepted one within
        `bound` of the convergence threshold: decisions are not required to match."""
        n = self.n_eval if upto is None else max(self.n_eval, upto + 1)
        if any(self.margin(i) < bound for i in range(n)):
            return True
        return self.acc >= 0 and abs(self.margin(self.acc) - TOL_SOLVE) < bound

    def status(self, acc):
        """linesearch_decide's status after the one iteration of an n_lqr_iter = 1 solve (include/dpilqr_hip.h)."""
        if acc < 0:
            return 2      # DPILQR_STATUS_LINESEARCH_FAILED
        return 1 if self.margin(acc) < TOL_SOLVE else 3      # DPILQR_STATUS_CONVERGED / DPILQR_STATUS_MAX_ITER
