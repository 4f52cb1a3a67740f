"""Shared by tests/test_gpu_singular.py and tests/test_singular_cases.py: inputs whose Q_uu has an EXACTLY zero pivot, built so
that the zero survives any order of exact row operations, the case tables that place them on every sweep and line search, and the
CPU verdict per item -- the oracle's zero-pivot return, which oracle.py raises as an AssertionError.  Nothing here touches the GPU.

Three constructions:
  (a) tiles with B = 0, so that Q_uu = L_uu exactly at every step and any mu.  Singular kinds: a zero column j (it stays zero under
      any row operations, so no pivot order can hide it), the zero matrix, and 4 I with the trailing 2 x 2 block all ones (its
      pivots are powers of two: exact under partial and under threshold pivoting).  The control `tiny` has column 1 zero except
      L_uu[1, 1] = 2^-60: that pivot is not zero, LAPACK does not raise and the item must not be flagged.  Each singular kind is
      placed at every step, at step T - 1 only (the first step a sweep processes) and at step 0 only.
  (b) an idle control with zero weight: the third control of Human6D (5) and HumanLin6D (6), the third and fourth of HumanPad12D (8)
      do not enter the dynamics, so that column of B is exactly zero and under R = diag(1, 1, 0) (diag(1, 1, 1, 0)) the column of
      Q_uu = R + B^T (P + mu I) B is exactly zero at every step, mu and iteration.  Healthy and singular items share a batch either
      through per-item R on a uniform model or through one shared R and a per-item model array: an item of quadcopters only is
      healthy, one with a human in the first or last agent slot is singular.
  (c) dt = 0: the discrete B of every built-in model is then exactly zero and Q_uu = R; R = diag(1, 0) on one agent is singular.
      No kernel divides by dt."""
import numpy as np

from oracle import oracle as orc
from tests import loop_gains_cases as lg

MODEL_DIMS = lg.MODEL_DIMS
STATUS_SINGULAR = 4
TILE_T = 3
TILE_MU = 0.5
PLACEMENTS = ("every", "last", "first")      # every step; step T - 1 only; step 0 only


# ------------------------------------------------------------------ (a) tiles
class TileCase:
    """One launch of the tiles API: records of n x m at T = 3, `count` items, with or without the block promise."""

    def __init__(self, route, n, m, blocks, count, tol=1e-9):
        self.route, self.n, self.m, self.blocks, self.count, self.tol = route, n, m, blocks, count, tol
        self.T = TILE_T

    @property
    def id(self):
        b = "dense" if self.blocks is None else "b%dx%d" % self.blocks
        return f"{self.route}-{self.n}x{self.m}-{b}-B{self.count}"

    def columns(self):
        """The zeroed columns: first, middle, last; where gj_blocked serves the size (n_u >= 24), also one that is no multiple of
        4 and one of 16 or more."""
        js = [0, self.m // 2, self.m - 1]
        if self.m >= 24:
            js += [5, 18]
        return js

    def singular_table(self):
        kinds = [("zero_col", j) for j in self.columns()] + [("all_zero", None), ("ones_block", None)]
        return [(kind, j, where) for kind, j in kinds for where in PLACEMENTS]

    def items(self):
        """(kind, column, placement) per item.  Even items are the controls -- healthy, every other one tiny --, odd items go
        through the singular table (a launch too small for the whole table takes evenly spaced rows of it)."""
        table = self.singular_table()
        n_sing = self.count // 2
        stride = max(1, len(table) // max(n_sing, 1))
        if stride > 1 and stride % len(PLACEMENTS) == 0:
            stride += 1      # the table lists each kind's placements together: walk across them as well
        out = []
        for i in range(self.count):
            if i % 2 == 0:
                out.append(("tiny" if i % 4 == 2 else "healthy", None, "every"))
            else:
                out.append(table[((i // 2) * stride) % len(table)])
        return out

    def complete(self):
        return {it for it in self.items() if it[0] not in ("healthy", "tiny")} == set(self.singular_table())


def _default_count(n, m, blocks):
    return 2 * len(TileCase("", n, m, blocks, 0).singular_table()) + 1


def tile_cases():
    """The routes of launch_riccati (tu_riccati.hip) a record-fed launch can take."""
    cases = []

    def add(route, n, m, blocks, count=None, tol=1e-9):
        cases.append(TileCase(route, n, m, blocks, _default_count(n, m, blocks) if count is None else count, tol))

    for n, m in ((8, 4), (20, 10)):
        for count in (9, 1100, 2100):                       # 4-, 8- and 12-wavefront tiers
            add("wave-bd", n, m, (4, 2), count)
        for count in (9, 1100):                             # dense tiles have no 12-wavefront tier; 1e-8: dense plugin tiles
            add("wave-dense", n, m, None, count, tol=1e-8)
    add("wave-mfma", 24, 12, None, tol=1e-8)
    add("wave-mfma", 24, 12, (4, 2))
    add("padded", 7, 3, None, tol=1e-8)
    add("padded", 6, 3, (6, 3))
    add("padded", 18, 9, None, tol=1e-8)
    add("padded", 18, 9, (6, 3))
    for k in (7, 12):            # register LU; gj_blocked declines, then lu_fallback_wg
        add("workgroup", 4 * k, 2 * k, (4, 2))
    for k in (8, 10):
        add("workgroup", 6 * k, 3 * k, (6, 3))
    for k in (2, 5):
        add("workgroup", 12 * k, 4 * k, (12, 4))
    add("generic", 28, 14, None, tol=1e-8)
    add("generic", 30, 7, None, tol=1e-8)
    return cases


def tile_route(case):
    """launch_riccati's selection (tu_riccati.hip) with every route switch unset."""
    n, m, bl = case.n, case.m, case.blocks
    bns, bnc = bl if bl else (0, 0)
    if (n, m) in lg.WAVE_SIZES:
        return "wave-bd" if (bns, bnc) == (4, 2) and n == 4 * (m // 2) and m % 2 == 0 else "wave-dense"
    if (n, m) == (24, 12):
        return "wave-mfma"
    if n <= 24 and m <= 12 and not (bns == 12 and n == 24):
        return "padded"
    if bns > 0 and n % bns == 0 and (n // bns, bns, bnc) in lg.WG_SIZES | lg.WG_RECORD_SIZES and m == (n // bns) * bnc:
        return "workgroup"
    return "generic"


def make_tiles(case, seed=0):
    """Host arrays A, B, Lx, Lu, Lxx, Luu, Lux of the launch (dp.pack_tiles' arguments) around the healthy base
    L_uu = off + off^T + 3 m I, off uniform in (0.2, 1)."""
    n, m, T, Bn = case.n, case.m, case.T, case.count
    rng = np.random.default_rng(9100 + 31 * n + m + seed)
    A = np.zeros((Bn, T, n, n)); Bm = np.zeros((Bn, T, n, m))
    if case.blocks:
        ns = case.blocks[0]
        for a in range(n // ns):
            A[:, :, ns * a:ns * a + ns, ns * a:ns * a + ns] = np.eye(ns) + 0.1 * rng.normal(size=(Bn, T, ns, ns))
    else:
        A[:] = np.eye(n) + 0.1 * rng.normal(size=(Bn, T, n, n)) / np.sqrt(n)
    S = rng.normal(size=(Bn, T + 1, n, n)); Lxx = S @ S.transpose(0, 1, 3, 2) / n + np.eye(n)
    off = rng.uniform(0.2, 1.0, size=(Bn, T + 1, m, m))
    Luu = off + off.transpose(0, 1, 3, 2) + 3.0 * m * np.eye(m)
    for b, (kind, j, where) in enumerate(case.items()):
        steps = {"every": range(T + 1), "last": [T - 1], "first": [0]}[where]
        for t in steps:
            M = Luu[b, t]
            if kind == "zero_col":
                M[:, j] = 0.0
            elif kind == "all_zero":
                M[:] = 0.0
            elif kind == "ones_block":
                M[:] = 4.0 * np.eye(m); M[-2:, -2:] = 1.0
            elif kind == "tiny":
                M[:, 1] = 0.0; M[1, 1] = 2.0 ** -60
    Lux = 0.2 * rng.normal(size=(Bn, T + 1, m, n))
    Lx = rng.normal(size=(Bn, T + 1, n)); Lu = rng.normal(size=(Bn, T + 1, m))
    return A, Bm, Lx, Lu, Lxx, Luu, Lux


def tile_verdicts(arrays, mu=TILE_MU):
    """Per item: (zero pivot?, K, d) from the oracle; K, d None for a flagged item."""
    out = []
    for parts in zip(*arrays):
        try:
            K, d = orc.backward_pass_tiles(*parts, mu)
            out.append((False, K, d))
        except AssertionError:
            out.append((True, None, None))
    return out


def tiles_subset(arrays, keep):
    return tuple(a[keep] for a in arrays)


def longdouble_pass_tiles(A, Bm, Lx, Lu, Lxx, Luu, Lux, mu):
    """The oracle's recursion on tiles (ilqr_oracle.c: riccati_step, lu_solve) in np.longdouble: the yardstick for the oracle's
    own error on the `tiny` kind."""
    ld = np.longdouble
    A, Bm, Lx, Lu, Lxx, Luu, Lux = (np.asarray(a, dtype=ld) for a in (A, Bm, Lx, Lu, Lxx, Luu, Lux))
    T, n, m = Bm.shape
    p, P = Lx[T].copy(), Lxx[T].copy()
    K = np.zeros((T, m, n), dtype=ld); d = np.zeros((T, m), dtype=ld)
    for t in range(T - 1, -1, -1):
        Qx = Lx[t] + A[t].T @ p; Qu = Lu[t] + Bm[t].T @ p
        Qxx = Lxx[t] + A[t].T @ P @ A[t]
        Preg = P + ld(mu) * np.eye(n, dtype=ld)
        Quu = Luu[t] + Bm[t].T @ Preg @ Bm[t]; Qux = Lux[t] + Bm[t].T @ Preg @ A[t]
        M = Quu.copy(); R = np.concatenate([Qux, Qu[:, None]], axis=1)
        for c in range(m):
            piv = c + int(np.argmax(np.abs(M[c:, c])))
            assert M[piv, c] != 0
            if piv != c:
                M[[c, piv]] = M[[piv, c]]; R[[c, piv]] = R[[piv, c]]
            l = M[c + 1:, c] / M[c, c]
            M[c + 1:] -= l[:, None] * M[c]; R[c + 1:] -= l[:, None] * R[c]
        for r in range(m - 1, -1, -1):
            R[r] = (R[r] - M[r, r + 1:] @ R[r + 1:]) / M[r, r]
        K[t], d[t] = -R[:, :n], -R[:, n]
        p = Qx + K[t].T @ Quu @ d[t] + K[t].T @ Qu + Qux.T @ d[t]
        Pn = Qxx + K[t].T @ Quu @ K[t] + K[t].T @ Qux + Qux.T @ K[t]
        P = (Pn + Pn.T) / 2
    return K, d


def pack_records(_lib, A, Bm, Lx, Lu, Lxx, Luu, Lux):
    """Host tile records in the library's layout (dpilqr_amd._lib.tile_layout), without a device: what dp.pack_tiles uploads."""
    Bn, T, n, m = Bm.shape
    lay, stride = _lib.tile_layout(n, m)
    rec = np.zeros((Bn, T + 1, stride))

    def put(key, arr, rows, cols, steps):
        o, l = lay[key]
        idx = o + (np.arange(rows) * l)[:, None] + np.arange(cols)[None, :]
        rec[:, :steps, idx] = np.asarray(arr, dtype=np.float64).reshape(Bn, steps, rows, cols)

    put("A", A, n, n, T); put("B", Bm, n, m, T)
    put("Lxx", Lxx, n, n, T + 1); put("Lux", Lux, m, n, T + 1); put("Luu", Luu, m, m, T + 1)
    put("Lx", Lx, 1, n, T + 1); put("Lu", Lu, 1, m, T + 1)
    return rec, stride


# ------------------------------------------------------------------ (b), (c) descriptor batches
HOVER_6, HOVER_12 = 9.80665, 9.80665 * 63.0 / 2000.0
IDLE = {4: 5, 7: 8}      # healthy model -> the model of its family with an idle control


class SolveCase(lg.Case):
    """One batch of construction (b) or (c).  how: 'per_item_R' (uniform model `models`, R of shape (B, k, n_c, n_c)), 'models'
    (one shared zero-weight R, a per-item model array: `models` names the healthy item) or 'shared_R' (every item singular: the
    fused flagship sweep wants one R for the batch).  `mask`: which items are singular (default: every third, from item 1)."""

    def __init__(self, name, models, B, how, dt, T, window=None, n_lqr_iter=6, f32=False, mask=None, seed=0):
        lg.lc.Case.__init__(self, "singular", models, B, 1, T=T, seed=seed)
        self.name, self.how, self.dt, self.n_lqr_iter, self.f32 = name, how, float(dt), n_lqr_iter, f32
        self.window = B if window is None else window
        self.mode = "first"
        m = np.zeros(B, dtype=bool)
        if how == "shared_R":
            m[:] = True
        elif mask is None:
            m[1::3] = True
        else:
            m[list(mask)] = True
        self.mask = m

    @property
    def id(self):
        return self.name

    def hints(self):
        ns = MODEL_DIMS[self.models[0]][0]
        um = self.models[0] if (self.uniform and self.how != "models") else -1
        planar4 = all(m in (0, 3) for m in self.models)
        return um, 3 if ns >= 6 else 2, self.how != "per_item_R", planar4

    def zero_weight(self):
        nc = MODEL_DIMS[self.models[0]][1]
        R = np.eye(nc); R[-1, -1] = 0.0
        return R


def make_solve_batch(case, healthy_twin=False):
    """Host arrays of the batch (ProblemBatch's arguments), and `singular`: the label per item.  healthy_twin: the batch of the
    same shape and iterates with R = I (the 'shared_R' cases' second batch)."""
    models, k, Bn, T = case.models, case.k, case.B, case.T
    ns, nc = MODEL_DIMS[models[0]]
    rng = np.random.default_rng(88000 + case.seed)
    if ns == 12:        # the gentle iterates of test_sweep_twelve_state_family: near the goal, near hover
        xf = rng.normal(size=(Bn, k * ns)) * 0.3; x0 = xf + rng.normal(size=(Bn, k * ns)) * 0.05
        U0 = rng.normal(size=(Bn, T, k * nc)) * 1e-3
    else:
        xf = rng.normal(size=(Bn, k * ns)) * 1.5; x0 = rng.normal(size=(Bn, k * ns)) * 1.5
        nd = 3 if ns >= 6 else 2
        x0.reshape(Bn, k, ns)[:, :, nd:] *= 0.1; xf.reshape(Bn, k, ns)[:, :, nd:] = 0.0
        U0 = rng.normal(size=(Bn, T, k * nc)) * 0.1
    mask = case.mask.copy()
    model = np.tile(np.asarray(models, dtype=np.int32), (Bn, 1))
    R = np.eye(nc)
    if case.how == "models":
        R = case.zero_weight()
        for i in np.flatnonzero(mask):
            model[i, 0 if (i // 3) % 2 == 0 else k - 1] = IDLE[models[0]]      # a human in the first or in the last agent slot
    elif case.how == "per_item_R":
        R = np.tile(np.eye(nc), (Bn, k, 1, 1))
        for i in np.flatnonzero(mask):
            R[i, 0 if (i // 3) % 2 == 0 else k - 1] = case.zero_weight()
    elif not healthy_twin:
        R = case.zero_weight()
    if healthy_twin:
        mask[:] = False
    Uv = U0.reshape(Bn, T, k, nc)
    for hover_model, ctrl, thrust in ((4, 0, HOVER_6), (7, 3, HOVER_12)):
        if MODEL_DIMS[hover_model] == (ns, nc):
            Uv[:, :, :, ctrl] += thrust * (model == hover_model)[:, None, :]
    Q = np.diag([1.0, 1, 0, 0]) if ns == 4 else np.eye(ns)
    Qf = (1000.0 if ns == 4 else 100.0) * np.eye(ns)
    return dict(models=model if case.how == "models" else list(models), n_dims=[3 if ns >= 6 else 2] * k, xf=xf, x0=x0, U0=U0, Q=Q, R=R,
                Qf=Qf, radius=0.5, dt=case.dt, T=T, singular=mask)


def batch_subset(b, keep):
    """The batch of the items `keep` alone."""
    out = dict(b)
    for key in ("xf", "x0", "U0", "singular"):
        out[key] = b[key][keep]
    if np.ndim(b["models"]) == 2:
        out["models"] = b["models"][keep]
    if np.ndim(b["R"]) == 4:
        out["R"] = b["R"][keep]
    return out


def item_problem(b, i):
    models = b["models"][i] if np.ndim(b["models"]) == 2 else b["models"]
    R = b["R"][i] if np.ndim(b["R"]) == 4 else b["R"]
    return orc.Problem(models, b["n_dims"], b["xf"][i], b["Q"], R, b["Qf"], b["radius"], b["dt"], b["T"])


def item_verdict(b, i, mu=1.0):
    """(zero pivot?, K, d) of the oracle's backward pass at (rollout(x0, U0), U0, mu) -- the first pass of a solve."""
    p = item_problem(b, i)
    X, _ = p.rollout(b["x0"][i], b["U0"][i])
    assert np.isfinite(X).all(), i      # an overflowing rollout gives NaN pivots, not zero ones: not the path under test
    try:
        K, d = p.backward_pass(X, b["U0"][i], mu)
        return False, K, d
    except AssertionError:
        return True, None, None


def solve_cases():
    """The solve-loop cases: every sweep class of loop_gains_cases.loop_route, the line searches of both launch widths."""
    c, s = [], iter(range(1, 99))
    add = lambda *a, **kw: c.append(SolveCase(*a, seed=next(s), **kw))
    add("six-mix-k2-B24", [4, 4], 24, "models", 0.1, 6)                                  # in-sweep production, team line search
    add("six-mix-k2-B1100", [4, 4], 1100, "models", 0.1, 6, window=1100)                 # ... one-wavefront sweep and line search
    add("six-mix-k6", [4] * 6, 30, "models", 0.1, 6)                                     # fused workgroup
    add("six-perR-k11", [5] * 11, 3, "per_item_R", 0.1, 6)                               # big, a team of workgroups
    add("six-perR-k11-f32", [5] * 11, 3, "per_item_R", 0.1, 6, f32=True)
    add("twelve-mix-k1", [7], 30, "models", 0.05, 8)                                     # record-fed padded
    add("twelve-mix-k2", [7, 7], 30, "models", 0.05, 8)                                  # record-fed workgroup
    add("twelve-mix-k6", [7] * 6, 6, "models", 0.05, 6)                                  # big
    add("dt0-m0-k5-shared-B64", [0] * 5, 64, "shared_R", 0.0, 8)                         # team
    add("dt0-m0-k5-shared-B1100", [0] * 5, 1100, "shared_R", 0.0, 8, window=1100)        # fused wavefront
    add("dt0-m3-k5-perR", [3] * 5, 1100, "per_item_R", 0.0, 8, window=1100)              # fused general
    add("dt0-m3-k8-perR", [3] * 8, 30, "per_item_R", 0.0, 8)                             # fused workgroup
    add("dt0-m3-k6-perR", [3] * 6, 30, "per_item_R", 0.0, 8)                             # record-fed wavefront
    add("dt0-m2-k7-perR", [2] * 7, 30, "per_item_R", 0.0, 8)                             # record-fed generic
    add("dt0-m0-k16-perR", [0] * 16, 6, "per_item_R", 0.0, 6)                            # big
    return c


# the class each solve case is meant for (tests/test_singular_cases.py holds loop_route to it)
SOLVE_ROUTES = {"six-mix-k2-B24": "in-sweep production", "six-mix-k2-B1100": "in-sweep production", "six-mix-k6": "fused workgroup",
                "six-perR-k11": "big", "six-perR-k11-f32": "big", "twelve-mix-k1": "record-fed padded",
                "twelve-mix-k2": "record-fed workgroup", "twelve-mix-k6": "big", "dt0-m0-k5-shared-B64": "team",
                "dt0-m0-k5-shared-B1100": "fused wavefront", "dt0-m3-k5-perR": "fused general", "dt0-m3-k8-perR": "fused workgroup",
                "dt0-m3-k6-perR": "record-fed wavefront", "dt0-m2-k7-perR": "record-fed generic", "dt0-m0-k16-perR": "big"}


def window_edge_case():
    """B = 40 through a window of 8: singular items at index 0, on both sides of the window's edge and at the last index."""
    return SolveCase("six-mix-k2-window8", [4, 4], 40, "models", 0.1, 6, window=8, mask=(0, 7, 8, 22, 39), seed=50)


def enqueue_case():
    return SolveCase("twelve-mix-k1-enqueue", [7], 30, "models", 0.05, 8, seed=51)


def sweep_cases():
    """Batches of the descriptor-sweep group (dpilqr_backward_pass_fused): (case, the sweep it takes).  Team forms at <= 1024
    items, the one-wavefront sweeps at 1100."""
    c, s = [], iter(range(60, 99))
    add = lambda route, *a, **kw: c.append((SolveCase(*a, seed=next(s), **kw), route))
    add("in-sweep production", "sweep-six-mix-k2", [4, 4], 90, "models", 0.1, 6)
    add("in-sweep production", "sweep-six-mix-k3-B1100", [4] * 3, 1100, "models", 0.1, 6)
    add("in-sweep production", "sweep-six-perR-k4", [6] * 4, 90, "per_item_R", 0.1, 6)
    add("fused workgroup", "sweep-six-mix-k5", [4] * 5, 60, "models", 0.1, 6)
    add("fused workgroup", "sweep-six-perR-k10", [5] * 10, 30, "per_item_R", 0.1, 6)
    add("team", "sweep-dt0-m0-k5-perR", [0] * 5, 90, "per_item_R", 0.0, 8)
    add("fused general", "sweep-dt0-m0-k5-perR-B1100", [0] * 5, 1100, "per_item_R", 0.0, 8)
    add("team", "sweep-dt0-m3-k2-perR", [3] * 2, 90, "per_item_R", 0.0, 8)
    add("fused general", "sweep-dt0-m3-k4-perR-B1100", [3] * 4, 1100, "per_item_R", 0.0, 8)
    add("fused workgroup", "sweep-dt0-m3-k15-perR", [3] * 15, 30, "per_item_R", 0.0, 8)
    add("team", "sweep-dt0-m0-k5-shared", [0] * 5, 90, "shared_R", 0.0, 8)
    add("fused wavefront", "sweep-dt0-m0-k5-shared-B1100", [0] * 5, 1100, "shared_R", 0.0, 8)
    return c


def sweep_route(case):
    """The sweep dpilqr_backward_pass_fused takes for the batch (launch_riccati_fused, tu_riccati.hip): loop_route's, except that
    the stand-alone entry never prefers records."""
    ns, nc = MODEL_DIMS[case.models[0]]
    k = case.k
    um, und, shared, planar4 = case.hints()
    f_wave = um == 0 and und == 2 and shared and (ns, nc) == (4, 2) and k <= 5
    f_general = (planar4 or um in (0, 3)) and und == 2 and (ns, nc) == (4, 2) and k <= 5
    if (ns, nc) == (4, 2) and k <= 5:
        if not f_wave and not f_general:
            return "in-sweep production"
    elif ((ns, nc) == (6, 3) and k <= 4) or ((ns, nc) == (3, 2) and k <= 6):
        return "in-sweep production"
    if case.B <= lg.TEAM_MAX and (k * ns, k * nc) in lg.TEAM_SIZES and (f_wave or f_general):
        return "team"
    if f_wave:
        return "fused wavefront"
    if f_general:
        return "fused general"
    assert (k, ns, nc) in lg.WG_SIZES, case.id
    return "fused workgroup"
