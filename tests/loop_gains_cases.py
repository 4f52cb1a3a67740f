"""Shared by tests/test_gpu_loop_gains.py and tests/test_loop_gains_cases.py: the cases of the solve loop's backward-pass check,
a Python mirror of the loop's route selection (launch.hpp's predicates, shape_of and the launchers' tables), and the CPU side of
the check -- the oracle's gains at one item's linearisation point, their rounding sensitivity, and the per-item bounds drawn
from it.  Nothing here touches the GPU.

Two ends of a solve are observable through the public API (tests/test_gpu_loop_gains.py):
  first: solve(n_lqr_iter=1, gains=True) returns each item's gains of the pass at (rollout(x0, U0), U0, mu = 1);
  last:  an item that ends by line-search failure keeps its iterate, so the returned (X, U) are the point of its LAST backward
         pass, trace[n_bwd - 1, 0] the mu it used and (K, d) that pass's gains.  With tol = 0 no item converges: each runs
         until its search fails or n_lqr_iter is reached.

Two things the route mirror shows about the loop itself.  The producer class `static+sparse` -- the static part followed by
k_make_tiles<NS, NC, true> with dyn_only = 1 -- serves no shape unless a route switch is set (tests/test_loop_gains_cases.py):
it has no case.  And the one-wavefront-per-item fused sweeps (k_riccati_mfma<..., FUSED>, k_riccati_mfma_general) run only at
launch widths beyond the team form's 1024, so each has a `last` case of its own with a window of 1100.

Batches, the per-item reference (the C oracle; NumPy for BikeDynamics5D) and the project's tolerance constants are
tests/linesearch_cases.py's."""
import re

import numpy as np

from tests import linesearch_cases as lc
from tests.golden_util import relerr
from tests.linesearch_cases import BIKE, CSRC, MODEL_DIMS, PERTURB, SPREAD_CAP, SPREAD_FACTOR, TOL_PASS, item_problem, make_batch  # noqa: F401

N_LQR_ITER_LAST = 30

PRODUCERS = ("none", "sparse", "static+wave", "static+sparse", "big")
SWEEPS = ("fused wavefront", "fused general", "team", "in-sweep production", "fused workgroup", "record-fed wavefront",
          "record-fed padded", "record-fed workgroup", "record-fed generic", "big")
WAVE_SWEEPS = ("fused wavefront", "fused general", "team", "in-sweep production", "record-fed wavefront", "record-fed padded")


def mu_schedule():
    """The values mu takes in a solve (control.py:227-237: delta = min(1, delta) / 2, mu *= delta, mu <= 1e-6 -> 0)."""
    mu, delta, out = 1.0, 2.0, [1.0]
    while mu > 0.0:
        delta = min(1.0, delta) / 2.0
        mu *= delta
        if mu <= 1e-6:
            mu = 0.0
        out.append(mu)
    return out


MU_SCHEDULE = mu_schedule()      # 1, 0.5, 0.125, 1.5625e-2, 9.765625e-4, 3.0517578125e-5, 0


# ------------------------------------------------------------------ constants of the launchers, read from their sources
def _src(unit):
    return re.sub(r"\\\n", " ", re.sub(r"//.*", "", (CSRC / unit).read_text()))


def _size_macro(unit, name):
    """The tuples of `#define NAME(X) X(a, b[, c]) ...`."""
    body = re.search(r"#define\s+" + name + r"\(X\)(.*)$", _src(unit), re.M).group(1)
    return {tuple(int(v) for v in t.split(",")) for t in re.findall(r"X\(([\d,\s]+)\)", body)}


WAVE_SIZES = _size_macro("tu_riccati.hip", "DPILQR_WAVE_SIZES")             # (n, m) of the wavefront sweeps
TEAM_SIZES = _size_macro("tu_team.hip", "DPILQR_TEAM_SIZES")
WG_SIZES = _size_macro("tu_riccati.hip", "DPILQR_WG_SIZES")                 # (k, n_s, n_c): fused and record-fed
WG_RECORD_SIZES = _size_macro("tu_riccati.hip", "DPILQR_WG_RECORD_SIZES")   # record-fed only
_model_ids = dict(re.findall(r"(k\w+)\s*=\s*(\d+)", re.search(r"enum Model : int \{(.*?)\};", _src("models.hpp"), re.S).group(1)))


def _tiles_wave_table():
    """k_make_tiles_wave<MODEL, KA, true>: the agent counts of tu_tiles.hip's DPILQR_TW_6 for every model it is used with."""
    text = _src("tu_tiles.hip")
    ks = re.findall(r"DPILQR_TRY_TW\(MODEL,\s*(\d+),", re.search(r"#define\s+DPILQR_TW_6\(MODEL, LINEAR\)(.*)$", text, re.M).group(1))
    uses = [l for l in text.splitlines() if not l.lstrip().startswith("#")]
    return {(int(_model_ids[name]), int(k)) for name in re.findall(r"DPILQR_TW_6\((k\w+),", "\n".join(uses)) for k in ks}


TILES_WAVE_TABLE = _tiles_wave_table()
_launch = _src("launch.hpp")
BIG_ABOVE = int(re.search(r"uses_big_path\(int n_x\).*?n_x > (\d+)", _launch, re.S).group(1))
TIER12_ABOVE, TIER8_ABOVE = (int(v) for v in re.search(r"constexpr int sweep_waves\(.*?grid_items > (\d+).*?grid_items > (\d+)", _launch,
                                                       re.S).groups())
TEAM_MAX = int(re.search(r"grid_items <= (\d+) && sweep_max_waves\(\)", _src("tu_riccati.hip")).group(1))
# every A/B route switch and tuning knob the library reads (honoured only behind DPILQR_DEBUG_ROUTES)
ROUTE_SWITCHES = sorted({name for f in sorted(CSRC.glob("*.h*")) for name in re.findall(r'route_(?:flag|env|int)\("(DPILQR_\w+)"', f.read_text())})
STATIC_MODELS = tuple(int(_model_ids[name]) for name in re.findall(r"um == (k\w+)", _src("dpilqr_hip.hip")))      # static_part


# ------------------------------------------------------------------ cases
class Case(lc.Case):
    """One case: `models` (k,), B items, `window` items in flight, mode 'first' or 'last', the stride of the checked items."""

    def __init__(self, models, B, window, mode, stride, per_agent=False, seed=0):
        super().__init__("loop", models, B, stride, per_agent=per_agent, T=16, seed=seed)
        self.window, self.mode = window, mode

    @property
    def id(self):
        m = f"m{self.models[0]}k{self.k}" if self.uniform else "mix" + "_".join(map(str, self.models))
        return f"{self.mode}-{m}-B{self.B}-w{self.window}" + ("-peragent" if self.per_agent else "")

    def hints(self):
        """What ProblemBatch derives for the descriptor's uniform_model word from make_batch's arrays: (model or -1, n_dims or
        -1, one Q / R / Q_f for all agents, planar four-state models only).  No weight of make_batch is per item: the Q, R, Q_f
        batch strides are 0."""
        ns = MODEL_DIMS[self.models[0]][0]
        nd = [3 if ns >= 6 else 2] * self.k
        if self.per_agent and ns == 6:
            nd = [3 if a % 2 == 0 else 2 for a in range(self.k)]
        um = self.models[0] if self.uniform else -1
        return um, (nd[0] if len(set(nd)) == 1 else -1), not self.per_agent, all(m in (0, 3) for m in self.models)


def loop_route(case, width=None):
    """(producer class, sweep class) of the solve loop for this case, at a launch of `width` items (default: the window, the
    width of every launch until all items are admitted).  Mirrors shape_of and static_part (dpilqr_hip.hip), the predicates of
    launch.hpp, launch_make_tiles (tu_tiles.hip), launch_riccati and launch_riccati_fused (tu_riccati.hip), with every route
    switch unset."""
    width = case.window if width is None else width
    ns, nc = MODEL_DIMS[case.models[0]]
    k = case.k
    n, m = k * ns, k * nc
    um, und, shared, planar4 = case.hints()
    if n > BIG_ABOVE:
        return "big", "big"
    f_wave = um == 0 and und == 2 and shared and (ns, nc) == (4, 2) and k <= 5
    f_general = (planar4 or um in (0, 3)) and und == 2 and (ns, nc) == (4, 2) and k <= 5
    f_wg = ((ns, nc) == (4, 2) and 6 <= k <= 15) or ((ns, nc) == (6, 3) and 2 <= k <= 10)
    if (ns, nc) == (4, 2) and k <= 5:
        f_inprod = not f_wave and not f_general
    else:
        f_inprod = ((ns, nc) == (6, 3) and k <= 4) or ((ns, nc) == (3, 2) and k <= 6) or ((ns, nc) == (5, 2) and k <= 4)
    if f_inprod:
        records = ns == 5 and k <= 2
    else:
        records = ((ns, nc) == (6, 3) and k in (2, 3, 4)) or ((ns, nc) == (4, 2) and k == 6)
    if (f_wave or f_general or f_wg or f_inprod) and not records:
        if f_inprod:
            return "none", "in-sweep production"
        if width <= TEAM_MAX and (n, m) in TEAM_SIZES and (f_wave or f_general):
            return "none", "team"
        if f_wave and (n, m) in WAVE_SIZES:
            return "none", "fused wavefront"
        if f_general and (n, m) in WAVE_SIZES:
            return "none", "fused general"
        assert f_wg and (k, ns, nc) in WG_SIZES, case.id
        return "none", "fused workgroup"
    if um in STATIC_MODELS:      # one linear model and (make_batch: always) one R for the batch
        producer = "static+wave" if (um, k) in TILES_WAVE_TABLE else "static+sparse"
    else:
        producer = "sparse"
    if (n, m) in WAVE_SIZES or (n, m) == (24, 12):
        return producer, "record-fed wavefront"
    if n <= 24 and m <= 12 and not (ns == 12 and n == 24):
        return producer, "record-fed padded"
    if (k, ns, nc) in WG_SIZES | WG_RECORD_SIZES:
        return producer, "record-fed workgroup"
    return producer, "record-fed generic"


def sweep_tier(case, width=None):
    """Wavefronts per workgroup of a wavefront sweep's launch of `width` items (launch.hpp: sweep_waves; the team form: 4), or 0
    for the other sweeps.  The 12-wavefront tier exists for the fused wavefront sweep and the record-fed one on block-diagonal
    four-state tiles of an exact size; the LDS clauses of sweep_waves do not bind at the sizes of all_cases()."""
    width = case.window if width is None else width
    ns, nc = MODEL_DIMS[case.models[0]]
    _, sweep = loop_route(case, width)
    if sweep not in WAVE_SWEEPS:
        return 0
    if sweep == "team":
        return 4
    tier12 = sweep == "fused wavefront" or (sweep == "record-fed wavefront" and (ns, nc) == (4, 2) and (case.k * ns, case.k * nc) in WAVE_SIZES)
    return 12 if tier12 and width > TIER12_ABOVE else (8 if width > TIER8_ABOVE else 4)


RECORD_FED_SHAPES = [([0] * 6, False), ([0] * 6, True), ([3] * 6, False), ([7] * 1, False), ([7] * 2, False), ([7] * 5, False),
                     ([7, 8, 7], False), ([2] * 7, False), ([2] * 8, False), ([2] * 14, False), ([BIKE] * 1, False), ([BIKE] * 2, False),
                     ([BIKE] * 5, False), ([BIKE] * 8, False)]
FUSED_SHAPES = [([0] * 5, False), ([3] * 4, False), ([0, 3, 0], False), ([0] * 5, True), ([4] * 3, False), ([1, 5, 6], True),
                ([2] * 4, False), ([BIKE] * 3, False), ([3] * 8, False), ([4] * 8, True)]
BIG_SHAPE = [3] * 16


def _stride(models, B):
    """About 40 checked items; about 12 for three and more BikeDynamics5D agents, whose NumPy reference takes tenths of a second
    per pass (one or two bikes: hundredths)."""
    return max(1, B // (12 if models[0] == BIKE and len(models) > 2 else 40))


# `last` cases whose first seed did not meet LastStats.check on the oracle alone (the share of items that end by a failed search,
# of items whose d draws a bound, or of items that end at mu = 0): the seed that does, found by scanning seeds 201..235 on the oracle
LAST_SEEDS = {(BIKE,): 204, (BIKE, BIKE): 201, (4, 4, 4): 224, (1, 5, 6): 205, (7,) * 5: 202}


def all_cases():
    cases = []
    seed = 0

    def add(models, B, window, mode, per_agent=False):
        nonlocal seed
        seed += 1
        own = LAST_SEEDS.get(tuple(models)) if mode == "last" else None
        cases.append(Case(models, B, window, mode, _stride(models, B), per_agent=per_agent, seed=own or seed))

    for models, per_agent in RECORD_FED_SHAPES + FUSED_SHAPES:
        add(models, 260, 260, "first", per_agent)
    add(BIG_SHAPE, 12, 12, "first")
    # launch widths: the team form (<= 1024), the 8- and the 12-wavefront tiers
    for width in (700, 1100, 2100):
        add([0] * 5, width, width, "first")
        add([0] * 6, width, width, "first")
    add([3] * 4, 1100, 1100, "first")      # beyond the team form, the fused general sweep itself
    seed = 100
    for models, per_agent in RECORD_FED_SHAPES + FUSED_SHAPES:
        add(models, 200, 50, "last", per_agent)
    add(BIG_SHAPE, 24, 6, "last")
    add([0] * 6, 200, 7, "last")
    add([7] * 2, 200, 7, "last")
    # windows beyond the team form: the one-wavefront-per-item fused sweeps serve the launches until the list drains below 1025
    add([0] * 5, 2200, 1100, "last")
    add([3] * 4, 2200, 1100, "last")
    return cases


# ------------------------------------------------------------------ the CPU side of one item's check
def _finite_pass(p, X, U, mu):
    try:
        K, d = p.backward_pass(X, U, mu)
    except (AssertionError, np.linalg.LinAlgError):      # an exactly zero pivot (oracle.Problem) / a singular Q_uu (NumPy)
        return None
    return (K, d) if np.isfinite(K).all() and np.isfinite(d).all() else None


class GainsRef:
    """The oracle's gains of one item's backward pass at (X, U, mu), their rounding sensitivity -- spread_K, spread_d: the
    largest relerr of each under X (1 +- 1e-15), U (1 -+ 1e-15), mu unperturbed -- and the item's bounds
    max(TOL_PASS, SPREAD_FACTOR * spread), drawn separately for K and d; None (unchecked) where the spread exceeds SPREAD_CAP or a
    perturbed pass is not finite."""

    def __init__(self, p, X, U, mu):
        X, U = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64)
        self.mu = float(mu)
        self.K, self.d = p.backward_pass(X, U, self.mu)
        self.spread_K = self.spread_d = 0.0
        for sg in (1.0, -1.0):
            e = sg * PERTURB
            pert = _finite_pass(p, X * (1 + e), U * (1 - e), self.mu)
            if pert is None:
                self.spread_K = self.spread_d = np.inf
                break
            self.spread_K = max(self.spread_K, relerr(pert[0], self.K))
            self.spread_d = max(self.spread_d, relerr(pert[1], self.d))
        self.bound_K, self.bound_d = self.bound_of(self.spread_K), self.bound_of(self.spread_d)

    @staticmethod
    def bound_of(spread):
        return None if not spread <= SPREAD_CAP else max(TOL_PASS, SPREAD_FACTOR * spread)


def oracle_last(p, x0, U0):
    """The oracle's own solve of one item as the `last` mode runs it (tol = 0): status, n_bwd, the mu of its last backward pass
    and the iterate it ended at."""
    if isinstance(p, lc._BikeProblem):
        r = p.s.solve(x0, U0, n_lqr_iter=N_LQR_ITER_LAST, tol=0.0)
        n_bwd = len(r["trace"])
    else:
        r = p.solve(x0, U0, n_lqr_iter=N_LQR_ITER_LAST, tol=0.0)
        n_bwd = r["n_bwd"]
    return dict(status=int(r["status"]), n_bwd=int(n_bwd), mu=float(r["trace"][n_bwd - 1][0]), X=r["X"], U=r["U"])


class LastStats:
    """The conditions that keep a `last` case from passing on nothing, over its checked items."""

    def __init__(self):
        self.n = self.failed = self.no_K = self.no_d = 0
        self.mus = []

    def add(self, status, mu=None, ref=None):
        self.n += 1
        if status != 2:
            return
        self.failed += 1
        self.mus.append(mu)
        self.no_K += ref.bound_K is None
        self.no_d += ref.bound_d is None

    def histogram(self):
        return {mu: self.mus.count(mu) for mu in MU_SCHEDULE if mu in self.mus}

    def check(self):
        f = self.failed
        assert f >= 0.60 * self.n, (f, self.n)
        assert self.mus.count(0.0) >= 0.20 * f and len(set(self.mus)) >= 3, self.histogram()
        assert self.no_K <= 0.05 * f and self.no_d <= 0.10 * f, (self.no_K, self.no_d, f)
