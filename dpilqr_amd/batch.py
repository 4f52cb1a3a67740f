"""Batched device solver: the lowering target of ilqrProblem and the one-launch-per-pass API.

A `ProblemBatch` is B sub-problems of one shape (k agents x (n_s, n_c), horizon T) held as device
tensors behind a `dpilqr_batch_desc` (include/dpilqr_hip.h).  It replaces the reference's per-problem
Python objects on the hot path:

    ilqrSolver._rollout        control.py:80-93    -> ProblemBatch.rollout
    ilqrSolver._backward_pass  control.py:116-148  -> ProblemBatch.make_tiles + backward_pass_tiles
    ilqrSolver._forward_pass   control.py:95-114   -> ProblemBatch.forward_pass
    ilqrSolver.solve           control.py:150-225  -> ProblemBatch.solve
    (no reference counterpart: the feedback policy closed loop)  -> ProblemBatch.policy_rollout, .policy_rollout_large, .policy_rollout_dec,
                                                                    .policy_rollout_dec_team, .policy_rollout_dec_wide
    (the step between two solves of a receding-horizon loop on a real plant)  -> ProblemBatch.policy_advance, .policy_advance_large, .policy_advance_dec,
                                                                                 .policy_advance_dec_team, .policy_advance_dec_wide
    (GameCost.__call__ at a few points, teams of up to 64 / 256 agents)  -> ProblemBatch.cost, .cost_wide
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .device import device, empty, ptr, stream_handle, to_dev, zeros

MODEL_DIMS = {0: (4, 2), 1: (6, 3), 2: (3, 2), 3: (4, 2), 4: (6, 3), 5: (6, 3), 6: (6, 3), 7: (12, 4), 8: (12, 4), 10: (5, 2)}

# The closed-loop routes: which (k, n_s, n_c) the closed-loop entry points serve, and the words they refuse the rest with.  This
# is the ONE place the limits are written on the Python side -- the validators below, DistributedPolicy (dispatch.py) and
# solve_rhc_closed_loop (distributed.py) ask route_refusal / route_serves -- as the closed-loop section of csrc/launch.hpp is on
# the C side; tests/test_closed_loop_routes_host.py holds the two to each other.  A route serves above_nx < n_x <= max_nx with
# k <= max_k agents (k <= max_k_of_ns[n_s] for the state sizes named there) of `families` (None: every family).
_SMALL = dict(above_nx=0, max_nx=60, max_k=20, families=None, max_k_of_ns={}, text=dict(
    beyond="{who} serves clusters up to n_x = {max_nx} and k = {max_k}, this batch has n_x = {n}, k = {k}"))
ROUTES = {
    "small": _SMALL,      # policy_rollout, policy_rollout_dec, policy_advance, policy_advance_dec
    "large": dict(above_nx=_SMALL["max_nx"], max_nx=240, max_k=_SMALL["max_k"], families=((4, 2), (6, 3), (12, 4)), max_k_of_ns={}, text=dict(
        below="{who} serves clusters of {above_nx} < n_x <= {max_nx}, this batch has n_x = {n}: use {use}",
        beyond="{who} serves clusters of {above_nx} < n_x <= {max_nx} and k <= {max_k} of the four-, six- and twelve-state families, "
               "this batch has n_x = {n}, k = {k}, (n_s, n_c) = ({n_s}, {n_c})")),      # policy_rollout_large, policy_advance_large
    "team": dict(above_nx=0, max_nx=float("inf"), max_k=_lib.MAX_AGENTS, families=None, max_k_of_ns={5: 12}, text=dict(
        beyond="{who} serves teams of up to {max_k} agents (a mask is one 64-bit word), this batch has k = {k}",
        family="{who} serves the five-state family up to {max_k_of_ns[5]} agents, this batch has k = {k}")),      # the two _dec_team
}
# an entry whose words differ from its route's
ROUTE_TEXT_OF = {"policy_rollout": dict(beyond="{who} serves clusters up to n_x = {max_nx}, this batch has n_x = {n}")}


def route_refusal(route, k, n_s, n_c):
    """None where `route` serves k agents of the (n_s, n_c) family, else the limit it misses: a key of ROUTES[route]['text']."""
    r, n = ROUTES[route], k * n_s
    if n <= r["above_nx"]:
        return "below"
    if n > r["max_nx"] or k > r["max_k"] or (r["families"] is not None and (n_s, n_c) not in r["families"]):
        return "beyond"
    return "family" if k > r["max_k_of_ns"].get(n_s, k) else None


def route_serves(route, k, n_s, n_c):
    return route_refusal(route, k, n_s, n_c) is None


def _shape(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


def _masks_trusted(masks_checked, nbr_bits):
    """masks_checked is the very int64 device tensor given as nbr_bits: an earlier call has read it back and checked it."""
    return masks_checked is not None and masks_checked is nbr_bits and isinstance(nbr_bits, torch.Tensor) and nbr_bits.dtype == torch.int64


def _shared_or_batched(a, B, per_item_shape, dtype):
    """Returns (device tensor, batch stride in elements): stride 0 when one copy serves the batch."""
    if isinstance(a, torch.Tensor):           # already on the device (the dispatch front end builds batches there)
        per = int(np.prod(per_item_shape))
        t = a.to(device=device(), dtype=dtype).contiguous()
        if t.numel() == per:
            return t, 0
        if t.numel() == B * per:
            return t, per
        raise ValueError(f"expected {per_item_shape} or {(B,) + tuple(per_item_shape)}, got {tuple(t.shape)}")
    a = np.asarray(a)
    per = int(np.prod(per_item_shape))
    if a.size == per:
        return to_dev(a.reshape(per_item_shape), dtype), 0
    if a.size == B * per:
        return to_dev(a.reshape((B,) + tuple(per_item_shape)), dtype), per
    raise ValueError(f"expected {per_item_shape} or {(B,) + tuple(per_item_shape)}, got {a.shape}")


class _WorkspacePool:
    """Solve workspaces (GBs each: tile records, gains, line-search candidates of a window of items), shared by all
    ProblemBatch objects and host threads of the process.  The dispatch front end solves one bucket per cluster size,
    concurrently, with a different workspace size each and different sizes again on the next call; handing every one
    to the caching allocator as a fresh odd-sized block made it hoard > 200 GB and then stall for seconds while it
    gave them back.  Buffers are rounded up to 256 MiB, the smallest free one that fits is reused, a solve returns its
    buffer when dpilqr_solve_batch has synchronised.  The pool is bounded by COUNT and by BYTES (a quarter of the
    device's memory): the buffers are live tensors, which the allocator's own out-of-memory recovery cannot reclaim."""
    GRANULE = 1 << 28
    MAX_FREE = 24
    MAX_FRACTION = 0.25

    def __init__(self):
        import threading
        self._lock = threading.Lock()
        self._free = []

    def _budget(self, dev):
        return int(torch.cuda.get_device_properties(dev).total_memory * self.MAX_FRACTION)

    def acquire(self, nbytes):
        dev = device()
        with self._lock:
            self._free = [t for t in self._free if t.device == dev]      # buffers of another device are dropped
            fit = [i for i, t in enumerate(self._free) if t.device == dev and t.numel() >= nbytes]
            if fit:
                return self._free.pop(min(fit, key=lambda i: self._free[i].numel()))
        size = max(1, -(-int(nbytes) // self.GRANULE)) * self.GRANULE
        try:
            return torch.empty(size, dtype=torch.uint8, device=dev)
        except getattr(torch, "OutOfMemoryError", torch.cuda.OutOfMemoryError):
            self.clear()                       # the pooled buffers are the likeliest reason: give them back and retry once
            torch.cuda.empty_cache()
            return torch.empty(size, dtype=torch.uint8, device=dev)

    def release(self, buf):
        with self._lock:
            self._free.append(buf)
            budget = self._budget(buf.device)
            # keep the large ones (they serve every request) within the count and byte bounds
            while len(self._free) > self.MAX_FREE or (len(self._free) > 1 and sum(t.numel() for t in self._free) > budget):
                self._free.pop(min(range(len(self._free)), key=lambda i: self._free[i].numel()))

    def clear(self):
        with self._lock:
            self._free.clear()


_workspace_pool = _WorkspacePool()


def release_workspaces():
    """Hand the pooled solve workspaces back to the allocator (they are kept between solves otherwise)."""
    _workspace_pool.clear()


class ProblemBatch:
    """B independent sub-problems with identical (k, n_s, n_c, T), resident in HBM.

    model, n_dims : (k,) shared or (B,k) per item     xf : (B, k*n_s)
    Q, Qf : (n_s,n_s) | (k,n_s,n_s) | (B,k,n_s,n_s)   R likewise with n_c     radius : scalar | (B,)
    """

    def __init__(self, model, n_dims, xf, Q, R, Qf, radius, dt, T, w_ref=1.0, w_prox=200.0, B=None, hints=None):
        """hints: (k, n_s, n_c, uniform_model word) for batches whose model / n_dims / weight arrays are device tensors
        (the dispatch front end): the constructor then neither reads them back nor derives the kernel hints from them."""
        lib = _lib.load()
        if hints is not None:
            self._init_from_device(lib, model, n_dims, xf, Q, R, Qf, radius, dt, T, w_ref, w_prox, B, hints)
            return
        xf = np.asarray(xf, dtype=np.float64) if not isinstance(xf, torch.Tensor) else xf
        model = np.asarray(model, dtype=np.int32)
        self.k = int(model.shape[-1])
        m0 = int(model.reshape(-1)[0])
        self.n_s, self.n_c = MODEL_DIMS[m0]
        if any(MODEL_DIMS[int(v)] != (self.n_s, self.n_c) for v in np.unique(model)):
            raise ValueError("all agents of a batch must share (n_s, n_c) -- the reference assumes it too "
                             "(dynamics.py:165-166)")
        self.n_x, self.n_u = self.k * self.n_s, self.k * self.n_c
        xf = xf.reshape(-1, self.n_x)
        self.B = int(B if B is not None else xf.shape[0])
        self.T, self.dt = int(T), float(dt)
        self.w_ref, self.w_prox = float(w_ref), float(w_prox)
        B_, k, ns, nc = self.B, self.k, self.n_s, self.n_c

        def expand(M, n):  # (n,n) -> (k,n,n)
            M = np.asarray(M, dtype=np.float64)
            return np.broadcast_to(M, (k, n, n)) if M.ndim == 2 else M

        self._model, ms = _shared_or_batched(model, B_, (k,), torch.int32)
        self._n_dims, ds = _shared_or_batched(np.asarray(n_dims, dtype=np.int32), B_, (k,), torch.int32)
        self._xf, xs = _shared_or_batched(xf, B_, (self.n_x,), torch.float64)
        if xf.shape[0] == 1 and B_ > 1:
            xs = 0
        self._Q, qs = _shared_or_batched(expand(Q, ns), B_, (k, ns, ns), torch.float64)
        self._R, rs = _shared_or_batched(expand(R, nc), B_, (k, nc, nc), torch.float64)
        self._Qf, fs = _shared_or_batched(expand(Qf, ns), B_, (k, ns, ns), torch.float64)
        self._radius, ras = _shared_or_batched(np.asarray(radius, dtype=np.float64), B_, (1,), torch.float64)
        uniform = 1 + m0 if bool((model == m0).all()) else 0      # hints for model-specialised kernels (dpilqr_hip.h)
        nd_all = np.asarray(n_dims, dtype=np.int32)
        if nd_all.size and bool((nd_all == nd_all.reshape(-1)[0]).all()):
            uniform |= (1 + int(nd_all.reshape(-1)[0])) << 8
        Qk, Rk, Qfk = (np.asarray(expand(M_, n_)) for M_, n_ in ((Q, ns), (R, nc), (Qf, ns)))
        if qs == 0 and rs == 0 and fs == 0 and all(M_.ndim == 3 and bool((M_ == M_[0]).all()) for M_ in (Qk, Rk, Qfk)):
            uniform |= 1 << 16                                       # one Q, R, Q_f for every agent of every item
        if bool(np.isin(np.asarray(model), (0, 3)).all()):
            uniform |= 1 << 17                                       # DoubleIntDynamics4D / UnicycleDynamics4D agents only
        self.desc = _lib.BatchDesc(B_, k, ns, nc, self.T, uniform, self.dt, self.w_ref, self.w_prox,
                                   ptr(self._model), ms, ptr(self._n_dims), ds, ptr(self._xf), xs,
                                   ptr(self._Q), qs, ptr(self._R), rs, ptr(self._Qf), fs, ptr(self._radius), ras)
        self._lib = lib
        self.tile_offsets, self.tile_stride = _lib.tile_layout(self.n_x, self.n_u)

    def _init_from_device(self, lib, model, n_dims, xf, Q, R, Qf, radius, dt, T, w_ref, w_prox, B, hints):
        self.k, self.n_s, self.n_c, uniform = (int(v) for v in hints)
        k, ns, nc = self.k, self.n_s, self.n_c
        self.n_x, self.n_u = k * ns, k * nc
        self.B = B_ = int(B)
        self.T, self.dt = int(T), float(dt)
        self.w_ref, self.w_prox = float(w_ref), float(w_prox)
        self._model, ms = _shared_or_batched(model, B_, (k,), torch.int32)
        self._n_dims, ds = _shared_or_batched(n_dims, B_, (k,), torch.int32)
        self._xf, xs = _shared_or_batched(xf, B_, (self.n_x,), torch.float64)
        self._Q, qs = _shared_or_batched(Q, B_, (k, ns, ns), torch.float64)
        self._R, rs = _shared_or_batched(R, B_, (k, nc, nc), torch.float64)
        self._Qf, fs = _shared_or_batched(Qf, B_, (k, ns, ns), torch.float64)
        rad = radius if isinstance(radius, torch.Tensor) else np.asarray(radius, dtype=np.float64)
        self._radius, ras = _shared_or_batched(rad, B_, (1,), torch.float64)
        if qs or rs or fs:
            uniform &= ~(1 << 16)
        self.desc = _lib.BatchDesc(B_, k, ns, nc, self.T, uniform, self.dt, self.w_ref, self.w_prox,
                                   ptr(self._model), ms, ptr(self._n_dims), ds, ptr(self._xf), xs,
                                   ptr(self._Q), qs, ptr(self._R), rs, ptr(self._Qf), fs, ptr(self._radius), ras)
        self._lib = lib
        self.tile_offsets, self.tile_stride = _lib.tile_layout(self.n_x, self.n_u)

    @staticmethod
    def hint_word(model, n_dims, Q, R, Qf):
        """The uniform_model hints (include/dpilqr_hip.h) of a k-agent problem whose host arrays are given."""
        model = np.asarray(model, dtype=np.int32); nd = np.asarray(n_dims, dtype=np.int32)
        w = (1 + int(model.reshape(-1)[0])) if bool((model == model.reshape(-1)[0]).all()) else 0
        if nd.size and bool((nd == nd.reshape(-1)[0]).all()):
            w |= (1 + int(nd.reshape(-1)[0])) << 8
        if all(np.asarray(M).ndim == 3 and bool((np.asarray(M) == np.asarray(M)[0]).all()) for M in (Q, R, Qf)):
            w |= 1 << 16
        if model.size and bool(np.isin(model, (0, 3)).all()):
            w |= 1 << 17                                             # DoubleIntDynamics4D / UnicycleDynamics4D agents only
        return w

    # ------------------------------------------------------------------ helpers
    @property
    def _d(self):
        return C.byref(self.desc)

    def tiles_buffer(self):
        return empty((self.B, self.T + 1, self.tile_stride))

    # ------------------------------------------------------------------ passes
    # dtype=torch.float32 selects the fp32 arm of BASELINE config 5's tolerance study (the *_f32 entry points): the
    # same passes with trajectories, gains and every intermediate in float; costs and the solver state stay double.
    @property
    def fused_sweep(self):
        """Clusters with n_x > 60 take the large-cluster path: linearize / quadraticize are evaluated inside the sweep,
        no tile records exist (one would be 1.28 MB at n_x = 240)."""
        return self.n_x > 60

    @property
    def is_large(self):
        """n_x > 60: the large-cluster kernels serve this batch (the fused sweep above, policy_rollout_large below)."""
        return self.n_x > ROUTES["small"]["max_nx"]

    def _in(self, a, shape, dtype=torch.float64):
        t = to_dev(a, dtype)
        if tuple(t.shape) != tuple(shape):
            t = t.reshape(shape)
        return t.contiguous()

    def rollout(self, x0, U, dtype=torch.float64):
        """control.py:80-93 for every item: returns X (B,T+1,n_x), J (B,) device tensors."""
        x0 = self._in(x0, (self.B, self.n_x), dtype); U = self._in(U, (self.B, self.T, self.n_u), dtype)
        X = empty((self.B, self.T + 1, self.n_x), dtype); J = empty((self.B,))
        fn = self._lib.dpilqr_rollout if dtype == torch.float64 else self._lib.dpilqr_rollout_f32
        _lib.check(fn(self._d, ptr(x0), ptr(U), ptr(X), ptr(J), stream_handle()))
        return X, J

    def rollout_wide(self, x0, U, trajectories=True):
        """The rollout of a FULL team of up to 256 agents (dpilqr_rollout_wide, include/dpilqr_swarm.h): rollout's definition for
        every item -- what J_full of a distributed solve of more than 64 agents is computed with -- plus min_sep and goal_dist as
        policy_rollout defines them.  Returns a dict of device tensors: J (B,), min_sep (B,), goal_dist (B,k) and, with
        trajectories=True, X (B,T+1,n_x).  Its sums have a fixed shape of their own: J agrees with rollout's to rounding, not bit
        for bit, and is the same bits run after run.  fp64 only."""
        if self.k > _lib.MAX_TEAM:
            raise ValueError(f"rollout_wide serves teams of up to {_lib.MAX_TEAM} agents, this batch has k = {self.k}")
        x0 = self._in(x0, (self.B, self.n_x)); U = self._in(U, (self.B, self.T, self.n_u))
        out = dict(J=empty((self.B,)), min_sep=empty((self.B,)), goal_dist=empty((self.B, self.k)))
        if trajectories:
            out["X"] = empty((self.B, self.T + 1, self.n_x))
        _lib.check(self._lib.dpilqr_rollout_wide(self._d, ptr(x0), ptr(U), ptr(out.get("X")), ptr(out["J"]), ptr(out["min_sep"]),
                                                 ptr(out["goal_dist"]), stream_handle()))
        return out

    def make_tiles(self, X, U, tiles=None):
        """linearize + quadraticize at every (X[t],U[t]) -> packed tile records (B,T+1,stride)."""
        X = self._in(X, (self.B, self.T + 1, self.n_x)); U = self._in(U, (self.B, self.T, self.n_u))
        tiles = self.tiles_buffer() if tiles is None else tiles
        _lib.check(self._lib.dpilqr_make_tiles(self._d, ptr(X), ptr(U), ptr(tiles), None, None, stream_handle()))
        return tiles

    def unpack_tiles(self, tiles):
        """Tile records -> dict of host arrays shaped like the plugin returns (per item, per step)."""
        t = tiles.cpu().numpy(); n, m = self.n_x, self.n_u
        shapes = dict(A=(n, n), B=(n, m), Lxx=(n, n), Lux=(m, n), Luu=(m, m), Lx=(1, n), Lu=(1, m))
        out = {}
        for key, (rows, cols) in shapes.items():
            off, ld = self.tile_offsets[key]
            idx = off + (np.arange(rows) * ld)[:, None] + np.arange(cols)[None, :]
            a = t[:, :, idx]
            out[key] = a[:, :, 0, :] if key in ("Lx", "Lu") else a
        return out

    def backward_pass(self, X, U, mu, tiles=None, dtype=torch.float64):
        """control.py:116-148: K (B,T,n_u,n_x), d (B,T,n_u)."""
        if dtype == torch.float64 and not self.fused_sweep and not _lib.route_flag("DPILQR_FORCE_BIG"):
            tiles = self.make_tiles(X, U, tiles)
            return backward_pass_tiles(tiles, self.B, self.T, self.n_x, self.n_u, mu, blocks=(self.n_s, self.n_c))
        B, T, n, m = self.B, self.T, self.n_x, self.n_u
        X = self._in(X, (B, T + 1, n), dtype); U = self._in(U, (B, T, m), dtype)
        mu_t = to_dev(np.broadcast_to(np.asarray(mu, dtype=np.float64), (B,))) if not isinstance(mu, torch.Tensor) else mu
        K = empty((B, T, m, n), dtype); d = empty((B, T, m), dtype)
        nbytes = self._lib.dpilqr_backward_pass_workspace_bytes(self._d, 8 if dtype == torch.float64 else 4)
        _lib.check(nbytes)
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device())
        fn = self._lib.dpilqr_backward_pass if dtype == torch.float64 else self._lib.dpilqr_backward_pass_f32
        _lib.check(fn(self._d, ptr(X), ptr(U), ptr(mu_t), ptr(K), ptr(d), ptr(ws), stream_handle()))
        return K, d

    def backward_pass_fused(self, X, U, mu):
        """The backward pass without tile records (dpilqr_backward_pass_fused); raises DpilqrError(EUNSUPPORTED) for batches
        the fused sweep does not serve."""
        B, T, n, m = self.B, self.T, self.n_x, self.n_u
        X = self._in(X, (B, T + 1, n)); U = self._in(U, (B, T, m))
        mu_t = to_dev(np.broadcast_to(np.asarray(mu, dtype=np.float64), (B,))) if not isinstance(mu, torch.Tensor) else mu
        K = empty((B, T, m, n)); d = empty((B, T, m))
        _lib.check(self._lib.dpilqr_backward_pass_fused(self._d, ptr(X), ptr(U), ptr(mu_t), ptr(K), ptr(d), None, stream_handle()))
        return K, d

    def forward_pass(self, X, U, K, d, alphas, dtype=torch.float64):
        """control.py:95-114 for all alphas: Xn (B,A,T+1,n_x), Un (B,A,T,n_u), Jn (B,A)."""
        X = self._in(X, (self.B, self.T + 1, self.n_x), dtype); U = self._in(U, (self.B, self.T, self.n_u), dtype)
        K = self._in(K, (self.B, self.T, self.n_u, self.n_x), dtype); d = self._in(d, (self.B, self.T, self.n_u), dtype)
        al = to_dev(np.asarray(alphas, dtype=np.float64)); A = int(al.numel())
        Xn = empty((self.B, A, self.T + 1, self.n_x), dtype); Un = empty((self.B, A, self.T, self.n_u), dtype); Jn = empty((self.B, A))
        fn = self._lib.dpilqr_forward_pass if dtype == torch.float64 else self._lib.dpilqr_forward_pass_f32
        _lib.check(fn(self._d, ptr(X), ptr(U), ptr(K), ptr(d), ptr(al), A, ptr(Xn), ptr(Un), ptr(Jn), stream_handle()))
        return Xn, Un, Jn

    # ------------------------------------------------------------------ the closed loop: what the eight methods share
    # method -> (route, neighbourhood gains?); the C entry is dpilqr_<method>
    CLOSED_LOOP = {"policy_rollout": ("small", False), "policy_rollout_large": ("large", False), "policy_rollout_dec": ("small", True),
                   "policy_rollout_dec_team": ("team", True), "policy_advance": ("small", False), "policy_advance_large": ("large", False),
                   "policy_advance_dec": ("small", True), "policy_advance_dec_team": ("team", True)}

    def _check_route(self, who, route, use):
        """ValueError, in `who`'s words, unless `route` serves this batch; `use`: the method a too small batch is sent to."""
        why = route_refusal(route, self.k, self.n_s, self.n_c)
        if why is not None:
            text = ROUTE_TEXT_OF.get(who, {}).get(why) or ROUTES[route]["text"][why]
            raise ValueError(text.format(who=who, use=use, n=self.n_x, k=self.k, n_s=self.n_s, n_c=self.n_c, **ROUTES[route]))

    def _check_u_lim(self, who, u_lim):
        if u_lim is not None:
            if _shape(u_lim) != (2, self.n_u):
                raise ValueError(f"{who}: u_lim has shape {_shape(u_lim)}, expected {(2, self.n_u)} (lower row, upper row)")
            lim = u_lim.cpu().numpy() if isinstance(u_lim, torch.Tensor) else np.asarray(u_lim, dtype=np.float64)
            if not bool((lim[0] <= lim[1]).all()):
                raise ValueError(f"{who}: u_lim has a lower limit above its upper limit")

    def _kc_max(self, who, Kc):
        """Kc (B,T,k,n_c,kc_max*n_s) -> kc_max."""
        B, T, k, n, ns, nc = self.B, self.T, self.k, self.n_x, self.n_s, self.n_c
        sk = _shape(Kc)
        if len(sk) != 5 or sk[:4] != (B, T, k, nc) or sk[4] < ns or sk[4] % ns or sk[4] > n:
            raise ValueError(f"{who}: Kc has shape {sk}, expected ({B}, {T}, {k}, {nc}, kc_max * {ns}) with 1 <= kc_max <= {k}")
        return sk[4] // ns

    def _rollout_shapes(self, who, X, U, K, nbr_bits, x0s, W, u_lim, check_masks=True):
        """Host-side validation of a rollout's arguments, in the order route, Kc, the arrays' shapes, u_lim, the masks; `who` is
        the method's name in the messages.  Returns (samples per item, kc_max, the masks as a host int64 array): the last two None
        for dense gains, the last None with check_masks=False.  Only the masks are read, and only when they are a device tensor
        (B * k words)."""
        B, T, k, n, m = self.B, self.T, self.k, self.n_x, self.n_u
        route, dec = self.CLOSED_LOOP[who]
        self._check_route(who, route, "policy_rollout")
        kc_max = self._kc_max(who, K) if dec else None
        others = (("U_ff", U, (B, T, m)), ("nbr_bits", nbr_bits, (B, k))) if dec else (("U", U, (B, T, m)), ("K", K, (B, T, m, n)))
        for name, a, want in (("X", X, (B, T + 1, n)),) + others:
            if _shape(a) != want:
                raise ValueError(f"{who}: {name} has shape {_shape(a)}, expected {want}")
        sx = _shape(x0s)
        if len(sx) != 3 or sx[0] != B or sx[2] != n or sx[1] < 1:
            raise ValueError(f"{who}: x0s has shape {sx}, expected ({B}, n_samples >= 1, {n})")
        S = int(sx[1])
        if W is not None and _shape(W) != (B, S, T, n):
            raise ValueError(f"{who}: W has shape {_shape(W)}, expected {(B, S, T, n)}")
        self._check_u_lim(who, u_lim)
        return S, kc_max, self._checked_masks(who, nbr_bits, kc_max) if dec and check_masks else None

    def _rollout(self, who, X, U, K, nbr_bits, x0s, W, u_lim, trajectories, masks_checked=None):
        """The four rollouts: validate, stage, call dpilqr_<who>, return the dict of outputs."""
        B, T, k, n, m, ns, nc = self.B, self.T, self.k, self.n_x, self.n_u, self.n_s, self.n_c
        dec = self.CLOSED_LOOP[who][1]
        trusted = dec and _masks_trusted(masks_checked, nbr_bits)
        S, kc_max, bits = self._rollout_shapes(who, X, U, K, nbr_bits, x0s, W, u_lim, check_masks=not trusted)
        X = self._in(X, (B, T + 1, n)); U = self._in(U, (B, T, m)); x0s = self._in(x0s, (B, S, n))
        W = None if W is None else self._in(W, (B, S, T, n))
        u_lim = None if u_lim is None else self._in(u_lim, (2, m))
        out = dict(J=empty((B, S)), min_sep=empty((B, S)), goal_dist=empty((B, S, k)))
        if trajectories:
            out["X"] = empty((B, S, T + 1, n)); out["U"] = empty((B, S, T, m))
        K = self._in(K, (B, T, k, nc, kc_max * ns) if dec else (B, T, m, n))
        gains = ()
        if dec:
            bits = nbr_bits.contiguous() if trusted else torch.from_numpy(bits).to(device())
            gains = (kc_max, ptr(bits))
        _lib.check(getattr(self._lib, "dpilqr_" + who)(self._d, ptr(X), ptr(U), ptr(K), *gains, S, ptr(x0s), ptr(W), ptr(u_lim),
                                                       ptr(out.get("X")), ptr(out.get("U")), ptr(out["J"]), ptr(out["min_sep"]),
                                                       ptr(out["goal_dist"]), stream_handle()))
        return out

    def _policy_shapes(self, X, U, K, x0s, W, u_lim):
        """Host-side validation of policy_rollout's arguments (no device access): returns the number of samples per item."""
        return self._rollout_shapes("policy_rollout", X, U, K, None, x0s, W, u_lim)[0]

    def _policy_large_shapes(self, X, U, K, x0s, W, u_lim):
        """Host-side validation of policy_rollout_large's arguments (no device access): returns the number of samples per item."""
        return self._rollout_shapes("policy_rollout_large", X, U, K, None, x0s, W, u_lim)[0]

    def _policy_dec_shapes(self, X, U_ff, Kc, nbr_bits, x0s, W, u_lim, check_masks=True):
        """Host-side validation of policy_rollout_dec's arguments: returns (samples per item, kc_max, the masks as a host
        int64 array -- None with check_masks=False)."""
        return self._rollout_shapes("policy_rollout_dec", X, U_ff, Kc, nbr_bits, x0s, W, u_lim, check_masks)

    def _policy_dec_team_shapes(self, X, U_ff, Kc, nbr_bits, x0s, W, u_lim, check_masks=True):
        """Host-side validation of policy_rollout_dec_team's arguments, as _policy_dec_shapes."""
        return self._rollout_shapes("policy_rollout_dec_team", X, U_ff, Kc, nbr_bits, x0s, W, u_lim, check_masks)

    def policy_rollout(self, X, U, K, x0s, W=None, u_lim=None, trajectories=False):
        """The closed-loop ensemble rollout (dpilqr_policy_rollout): every item's feedback policy u_t = U[t] + K[t] (x_t - X[t])
        run from S starts at once.  X (B,T+1,n_x), U (B,T,n_u), K (B,T,n_u,n_x): nominal and gains (backward_pass at that
        nominal); x0s (B,S,n_x); W (B,S,T,n_x) additive disturbance on x_{t+1} or None; u_lim (2,n_u) lower / upper control
        limits shared by all items or None.  Returns a dict of device tensors: J (B,S), min_sep (B,S), goal_dist (B,S,k) and,
        with trajectories=True, X (B,S,T+1,n_x), U (B,S,T,n_u)."""
        return self._rollout("policy_rollout", X, U, K, None, x0s, W, u_lim, trajectories)

    def policy_rollout_large(self, X, U, K, x0s, W=None, u_lim=None, trajectories=False):
        """policy_rollout for large clusters, 60 < n_x <= 240 with k <= 20 (dpilqr_policy_rollout_large): the same arguments and
        the same returned dict.  K[t] (x_t - X[t]) is formed on the fp64 matrix pipe -- the columns in ascending order, one fused
        multiply-add per term -- so a control may differ from policy_rollout's arithmetic in the last bits."""
        return self._rollout("policy_rollout_large", X, U, K, None, x0s, W, u_lim, trajectories)

    def _checked_masks(self, who, nbr_bits, kc_max):
        """The masks' contract -- DPILQR_EINVAL of include/dpilqr_policy.h, decided here because the C entry points only
        enqueue --: returns them as a host int64 array.  Reads them back when they are a device tensor (B * k words)."""
        B, k = self.B, self.k
        bits = nbr_bits.cpu().numpy() if isinstance(nbr_bits, torch.Tensor) else np.asarray(nbr_bits)
        if bits.dtype.kind not in "iu":
            raise ValueError(f"{who}: nbr_bits has dtype {bits.dtype}, expected integer bit masks")
        bits = np.ascontiguousarray(bits.astype(np.uint64) & np.uint64((1 << k) - 1))
        own = np.uint64(1) << np.arange(k, dtype=np.uint64)
        if not bool(((bits & own[None, :]) != 0).all()):
            raise ValueError(f"{who}: a neighbourhood mask lacks its agent's own bit (DPILQR_EINVAL)")
        count = np.zeros((B, k), dtype=np.int64)
        for j in range(k):
            count += ((bits >> np.uint64(j)) & np.uint64(1)).astype(np.int64)
        if int(count.max(initial=0)) > kc_max:
            raise ValueError(f"{who}: a neighbourhood mask has {int(count.max())} members, Kc holds kc_max = {kc_max} "
                             "(DPILQR_EINVAL)")
        return bits.view(np.int64)

    def policy_rollout_dec(self, X, U_ff, Kc, nbr_bits, x0s, W=None, u_lim=None, trajectories=False, masks_checked=None):
        """The closed loop of a distributed solution (dpilqr_policy_rollout_dec): agent i of item b applies
        u_i = U_ff[b][t][i] + Kc[b][t][i] (x - X[b][t]) over its neighbourhood nbr_bits[b][i] only (bit j = agent j, its own bit
        set).  X (B,T+1,n_x): the stitched trajectory; U_ff (B,T,n_u); Kc (B,T,k,n_c,kc_max*n_s): agent i's rows, the columns its
        neighbourhood's members in ascending order (columns past them are never read); nbr_bits (B,k) integer masks;
        x0s, W, u_lim, trajectories and the returned dict: as policy_rollout, on this (full k-agent) batch.
        masks_checked: the very int64 device tensor given as nbr_bits, if an earlier call has already checked it -- that call's
        read-back of the masks is then not repeated (DistributedPolicy.rollout in a loop)."""
        return self._rollout("policy_rollout_dec", X, U_ff, Kc, nbr_bits, x0s, W, u_lim, trajectories, masks_checked)

    def policy_rollout_dec_team(self, X, U_ff, Kc, nbr_bits, x0s, W=None, u_lim=None, trajectories=False, masks_checked=None):
        """policy_rollout_dec for a whole team of up to 64 agents at any n_x (dpilqr_policy_rollout_dec_team): the same arguments,
        the same definition and the same returned dict.  A mask is one 64-bit word (bit 63 a member like any other; int64 masks
        may be negative).  Where both serve a batch, X, U and goal_dist equal policy_rollout_dec's bit for bit, J and min_sep to
        rounding (the stage cost is summed agent by agent)."""
        return self._rollout("policy_rollout_dec_team", X, U_ff, Kc, nbr_bits, x0s, W, u_lim, trajectories, masks_checked)

    # ------------------------------------------------------------------ the closed loop of a team of up to 256 agents
    def _checked_masks_wide(self, who, nbr_bits, kc_max):
        """_checked_masks over (B, k, n_words) words -- word w, bit b = agent 64 w + b: own bit set, at most kc_max members, nothing
        at or past bit k.  Returns the masks as a host int64 array; reads them back when they are a device tensor."""
        B, k, nw = self.B, self.k, (self.k + 63) // 64
        bits = nbr_bits.cpu().numpy() if isinstance(nbr_bits, torch.Tensor) else np.asarray(nbr_bits)
        if bits.dtype.kind not in "iu":
            raise ValueError(f"{who}: nbr_bits has dtype {bits.dtype}, expected integer bit masks")
        bits = np.ascontiguousarray(bits.astype(np.uint64)).reshape(B, k, nw)
        agent = np.arange(k)
        own = np.uint64(1) << (agent % 64).astype(np.uint64)
        if not bool(((bits[:, agent, agent // 64] & own[None, :]) != 0).all()):
            raise ValueError(f"{who}: a neighbourhood mask lacks its agent's own bit (DPILQR_EINVAL)")
        valid = np.array([(1 << min(max(k - 64 * w, 0), 64)) - 1 for w in range(nw)], dtype=np.uint64)
        if bool((bits & ~valid[None, None, :]).any()):
            raise ValueError(f"{who}: a neighbourhood mask has a bit at or past agent k = {k} (DPILQR_EINVAL)")
        count = np.zeros((B, k), dtype=np.int64)
        for j in range(64):
            count += ((bits >> np.uint64(j)) & np.uint64(1)).astype(np.int64).sum(axis=2)
        if int(count.max(initial=0)) > kc_max:
            raise ValueError(f"{who}: a neighbourhood mask has {int(count.max())} members, Kc holds kc_max = {kc_max} "
                             "(DPILQR_EINVAL)")
        return bits.view(np.int64)

    def policy_rollout_dec_wide(self, X, U_ff, Kc, nbr_bits, x0s, W=None, u_lim=None, trajectories=False, masks_checked=None):
        """policy_rollout_dec_team for a whole team of up to 256 agents (dpilqr_policy_rollout_dec_wide,
        include/dpilqr_swarm_policy.h): the same definition and the same returned dict.  nbr_bits (B, k, n_words) integer masks,
        n_words = ceil(k / 64): word w, bit b = agent 64 w + b; a valid mask has its own bit set, at most kc_max members and
        nothing at or past bit k.  A neighbourhood is a sub-problem of the distributed solve: kc_max <= min(k, 64), whatever k is.
        With n_words = 1 every result equals policy_rollout_dec_team's bit for bit.  The other arguments, masks_checked included:
        as policy_rollout_dec.  fp64 only.  The receding-horizon advance of such teams: policy_advance_dec_wide."""
        who = "policy_rollout_dec_wide"
        B, T, k, n, m, ns, nc = self.B, self.T, self.k, self.n_x, self.n_u, self.n_s, self.n_c
        if k > _lib.MAX_TEAM:
            raise ValueError(f"{who} serves teams of up to {_lib.MAX_TEAM} agents, this batch has k = {k}")
        if ns == 5 and k > ROUTES["team"]["max_k_of_ns"][5]:
            raise ValueError(f"{who} serves the five-state family up to {ROUTES['team']['max_k_of_ns'][5]} agents, this batch has k = {k}")
        nw, kc_lim = (k + 63) // 64, min(k, _lib.MAX_AGENTS)
        sk = _shape(Kc)
        if len(sk) != 5 or sk[:4] != (B, T, k, nc) or sk[4] < ns or sk[4] % ns or sk[4] > kc_lim * ns:
            raise ValueError(f"{who}: Kc has shape {sk}, expected ({B}, {T}, {k}, {nc}, kc_max * {ns}) with 1 <= kc_max <= {kc_lim}")
        kc_max = sk[4] // ns
        for name, a, want in (("X", X, (B, T + 1, n)), ("U_ff", U_ff, (B, T, m)), ("nbr_bits", nbr_bits, (B, k, nw))):
            if _shape(a) != want:
                raise ValueError(f"{who}: {name} has shape {_shape(a)}, expected {want}")
        sx = _shape(x0s)
        if len(sx) != 3 or sx[0] != B or sx[2] != n or sx[1] < 1:
            raise ValueError(f"{who}: x0s has shape {sx}, expected ({B}, n_samples >= 1, {n})")
        S = int(sx[1])
        if W is not None and _shape(W) != (B, S, T, n):
            raise ValueError(f"{who}: W has shape {_shape(W)}, expected {(B, S, T, n)}")
        self._check_u_lim(who, u_lim)
        if _masks_trusted(masks_checked, nbr_bits):
            bits = nbr_bits.contiguous()
        else:
            bits = torch.from_numpy(self._checked_masks_wide(who, nbr_bits, kc_max)).to(device())
        X = self._in(X, (B, T + 1, n)); U_ff = self._in(U_ff, (B, T, m)); x0s = self._in(x0s, (B, S, n))
        Kc = self._in(Kc, (B, T, k, nc, kc_max * ns))
        W = None if W is None else self._in(W, (B, S, T, n))
        u_lim = None if u_lim is None else self._in(u_lim, (2, m))
        out = dict(J=empty((B, S)), min_sep=empty((B, S)), goal_dist=empty((B, S, k)))
        if trajectories:
            out["X"] = empty((B, S, T + 1, n)); out["U"] = empty((B, S, T, m))
        _lib.check(self._lib.dpilqr_policy_rollout_dec_wide(self._d, ptr(X), ptr(U_ff), ptr(Kc), kc_max, ptr(bits), S, ptr(x0s), ptr(W),
                                                            ptr(u_lim), ptr(out.get("X")), ptr(out.get("U")), ptr(out["J"]),
                                                            ptr(out["min_sep"]), ptr(out["goal_dist"]), nw, stream_handle()))
        return out

    # ------------------------------------------------------------------ the receding-horizon advance
    ADVANCE_STATE = ("x_cur", "n_done", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left", "U_next", "X_next")

    def advance_state(self, x0, L):
        """The state of a receding-horizon loop over S scenarios of this batch's shape with room for L executed steps, as
        policy_advance keeps it: a dict of device tensors x_cur (S,n_x) = x0, n_done (S,) int32 = 0, X_exec (S,L+1,n_x),
        U_exec (S,L,n_u), J_exec (S,) = 0, min_sep (S,) = +inf, dist_left (S,k) (NaN until a scenario's first advance),
        U_next (S,T,n_u), X_next (S,T+1,n_x)."""
        x0 = to_dev(x0).reshape(-1, self.n_x).contiguous().clone()
        S, L = int(x0.shape[0]), int(L)
        if L < 1:
            raise ValueError(f"advance_state: L = {L}, the capacity is at least one step")
        return dict(x_cur=x0, n_done=zeros((S,), torch.int32), X_exec=zeros((S, L + 1, self.n_x)), U_exec=zeros((S, L, self.n_u)),
                    J_exec=zeros((S,)), min_sep=torch.full((S,), float("inf"), dtype=torch.float64, device=x0.device),
                    dist_left=torch.full((S, self.k), float("nan"), dtype=torch.float64, device=x0.device),
                    U_next=zeros((S, self.T, self.n_u)), X_next=zeros((S, self.T + 1, self.n_x)))

    def _advance_shapes(self, who, X, h, state, scen, W, u_lim, n_d, others, large=False, team=False, wide=False):
        """Host-side validation of what policy_advance, policy_advance_dec, policy_advance_large and policy_advance_dec_team
        share (no device access): returns (S, L).  large: the size test is policy_advance_large's; team: the team advance's;
        wide: none here (policy_advance_dec_wide lies outside the route table and has tested its own limits)."""
        B, T, k, n, m = self.B, self.T, self.k, self.n_x, self.n_u
        if not wide:
            self._check_route(who, "team" if team else "large" if large else "small", "policy_advance")
        for name, a, want in (("X", X, (B, T + 1, n)),) + tuple(others):
            if a is not None and _shape(a) != want:
                raise ValueError(f"{who}: {name} has shape {_shape(a)}, expected {want}")
        if int(h) != h or not 1 <= h <= T:
            raise ValueError(f"{who}: h = {h}, a round executes 1 .. T = {T} steps")
        if int(n_d) != n_d or not 1 <= n_d <= self.n_s:
            raise ValueError(f"{who}: n_d = {n_d}, an agent has n_s = {self.n_s} states")
        get = (lambda f: state.get(f)) if isinstance(state, dict) else (lambda f: getattr(state, f, None))
        missing = [f for f in self.ADVANCE_STATE if not isinstance(get(f), torch.Tensor)]
        if missing:
            raise ValueError(f"{who}: state lacks the device tensors {missing} (ProblemBatch.advance_state makes one)")
        sx, su = _shape(get("x_cur")), _shape(get("U_exec"))
        if len(sx) != 2 or sx[1] != n or len(su) != 3 or su[1] < 1:
            raise ValueError(f"{who}: state x_cur {sx}, U_exec {su}: expected (S, {n}) and (S, L >= 1, {m})")
        S, L = int(sx[0]), int(su[1])
        want = dict(x_cur=(S, n), n_done=(S,), X_exec=(S, L + 1, n), U_exec=(S, L, m), J_exec=(S,), min_sep=(S,), dist_left=(S, k),
                    U_next=(S, T, m), X_next=(S, T + 1, n))
        for f, w in want.items():
            t = get(f)
            if _shape(t) != w or t.dtype != (torch.int32 if f == "n_done" else torch.float64) or not t.is_contiguous():
                raise ValueError(f"{who}: state {f} is {_shape(t)} {t.dtype}, expected contiguous {w} "
                                 f"{'int32' if f == 'n_done' else 'float64'}")
        if scen is None:
            if S < B:
                raise ValueError(f"{who}: the state holds {S} scenarios for {B} items and no scen names theirs")
        else:
            if _shape(scen) != (B,):
                raise ValueError(f"{who}: scen has shape {_shape(scen)}, expected {(B,)}")
            if not isinstance(scen, torch.Tensor):
                sc = np.asarray(scen)
                if sc.dtype.kind not in "iu" or (sc.size and (sc.min() < 0 or sc.max() >= S)) or np.unique(sc).size != sc.size:
                    raise ValueError(f"{who}: scen must name {B} distinct scenarios out of 0 .. {S - 1}")
            elif scen.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{who}: scen has dtype {scen.dtype}, expected integers")
        if W is not None and _shape(W) != (S, L, n):
            raise ValueError(f"{who}: W has shape {_shape(W)}, expected {(S, L, n)} (scenarios, capacity, n_x)")
        self._check_u_lim(who, u_lim)
        return S, L

    def _advance_args(self, X, U, state, scen, W, u_lim, S, L):
        B, T, n, m = self.B, self.T, self.n_x, self.n_u
        X = self._in(X, (B, T + 1, n)); U = self._in(U, (B, T, m))
        scen = None if scen is None else to_dev(scen, torch.int32)
        W = None if W is None else self._in(W, (S, L, n))
        u_lim = None if u_lim is None else self._in(u_lim, (2, m))
        st = [state[f] if isinstance(state, dict) else getattr(state, f) for f in self.ADVANCE_STATE]
        for name, t in (("U_next", st[7]), ("X_next", st[8])):
            if t.data_ptr() in (X.data_ptr(), U.data_ptr()):
                raise ValueError(f"policy_advance: state {name} aliases the plan it is the shift of")
        return X, U, scen, W, u_lim, [ptr(t) for t in st]

    def policy_advance(self, X, U, K, h, state, scen=None, W=None, u_lim=None, n_d=2):
        """The step between two solves of a receding-horizon loop (dpilqr_policy_advance): every item j -- a running scenario,
        s = scen[j] of the S the state holds (scen None: s = j) -- executes h steps of its own plan X (B,T+1,n_x), U (B,T,n_u)
        under the gains K (B,T,n_u,n_x) (None: open loop) from state['x_cur'][s], W (S,L,n_x) read at the scenario's own step
        count, u_lim (2,n_u) as policy_rollout.  `state` (advance_state) is updated in place: the executed states, controls
        and cost are appended at n_done[s] (never past the capacity L), min_sep and dist_left (over n_d coordinates) follow the
        plant, and U_next / X_next receive the plan shifted by the executed steps, the plant's state in front: the next
        round's warm start.  Scenarios not named are not touched.  Returns state."""
        return self._advance("policy_advance", X, U, K, None, h, state, scen, W, u_lim, n_d)

    def policy_advance_large(self, X, U, K, h, state, scen=None, W=None, u_lim=None, n_d=2):
        """policy_advance for large clusters, 60 < n_x <= 240 with k <= 20 (dpilqr_policy_advance_large): the same arguments, the
        same state dict (advance_state) and the same semantics.  K[i] (x - X[i]) is formed on the fp64 matrix pipe as
        policy_rollout_large forms it -- the columns in ascending order, one fused multiply-add per term -- so the executed
        prefix equals that rollout's bit for bit, and may differ from policy_advance's arithmetic in the last bits."""
        return self._advance("policy_advance_large", X, U, K, None, h, state, scen, W, u_lim, n_d)

    def policy_advance_dec(self, X, U_ff, Kc, nbr_bits, h, state, scen=None, W=None, u_lim=None, n_d=2, masks_checked=None):
        """policy_advance under a distributed solution's policy (dpilqr_policy_advance_dec): X the stitched trajectory, U_ff,
        Kc (B,T,k,n_c,kc_max*n_s) and nbr_bits (B,k) as policy_rollout_dec takes them, masks_checked included.  Kc None: the
        plan U_ff (then U_dec) is executed open loop and the masks are not read."""
        return self._advance("policy_advance_dec", X, U_ff, Kc, nbr_bits, h, state, scen, W, u_lim, n_d, masks_checked)

    def policy_advance_dec_team(self, X, U_ff, Kc, nbr_bits, h, state, scen=None, W=None, u_lim=None, n_d=2, masks_checked=None):
        """policy_advance_dec for a whole team of up to 64 agents at any n_x (dpilqr_policy_advance_dec_team): the same
        arguments, the same state dict (advance_state) and the same semantics, with policy_rollout_dec_team's arithmetic.  A mask
        is one 64-bit word (bit 63 a member like any other; int64 masks may be negative).  The executed prefix equals
        policy_rollout_dec_team's bit for bit; where policy_advance_dec serves the batch too, everything but J_exec and min_sep
        equals its results bit for bit, those two to rounding (the stage cost is summed agent by agent)."""
        return self._advance("policy_advance_dec_team", X, U_ff, Kc, nbr_bits, h, state, scen, W, u_lim, n_d, masks_checked)

    def _advance(self, who, X, U, K, nbr_bits, h, state, scen, W, u_lim, n_d, masks_checked=None):
        """The four advances: validate (Kc, _advance_shapes, the masks), stage, call dpilqr_<who>, return the state."""
        B, T, k, n, m, ns, nc = self.B, self.T, self.k, self.n_x, self.n_u, self.n_s, self.n_c
        route, dec = self.CLOSED_LOOP[who]
        kc_max, bits = 1, None
        if dec:
            if K is not None:
                kc_max = self._kc_max(who, K)
            others = (("U_ff", U, (B, T, m)),) + ((("nbr_bits", nbr_bits, (B, k)),) if K is not None else ())
        else:
            others = (("U", U, (B, T, m)), ("K", K, (B, T, m, n)))
        S, L = self._advance_shapes(who, X, h, state, scen, W, u_lim, n_d, others, large=route == "large", team=route == "team")
        if K is not None:
            if dec:
                if nbr_bits is None:
                    raise ValueError(f"{who}: gains without neighbourhood masks")
                trusted = _masks_trusted(masks_checked, nbr_bits)
                bits = nbr_bits.contiguous() if trusted else torch.from_numpy(self._checked_masks(who, nbr_bits, kc_max)).to(device())
            K = self._in(K, (B, T, k, nc, kc_max * ns) if dec else (B, T, m, n))
        X, U, scen, W, u_lim, st = self._advance_args(X, U, state, scen, W, u_lim, S, L)
        gains = (kc_max, ptr(bits)) if dec else ()
        _lib.check(getattr(self._lib, "dpilqr_" + who)(self._d, ptr(X), ptr(U), ptr(K), *gains, int(h), ptr(scen), S, L, int(n_d), ptr(W),
                                                       ptr(u_lim), *st, stream_handle()))
        return state

    def policy_advance_dec_wide(self, X, U_ff, Kc, nbr_bits, h, state, scen=None, W=None, u_lim=None, n_d=2, masks_checked=None):
        """policy_advance_dec_team for a whole team of up to 256 agents (dpilqr_policy_advance_dec_wide,
        include/dpilqr_swarm_advance.h): the same arguments, the same state dict (advance_state) and the same semantics, with
        policy_rollout_dec_wide's arithmetic and masks: nbr_bits (B, k, n_words), n_words = ceil(k / 64), word w, bit b =
        agent 64 w + b; kc_max <= min(k, 64).  The executed prefix equals policy_rollout_dec_wide's bit for bit; with
        n_words = 1 all nine state fields equal policy_advance_dec_team's bit for bit.  Kc None: the plan U_ff (then U_dec) is
        executed open loop and the masks are not read.  fp64 only."""
        who = "policy_advance_dec_wide"
        B, T, k, n, m, ns, nc = self.B, self.T, self.k, self.n_x, self.n_u, self.n_s, self.n_c
        if k > _lib.MAX_TEAM:
            raise ValueError(f"{who} serves teams of up to {_lib.MAX_TEAM} agents, this batch has k = {k}")
        if ns == 5 and k > ROUTES["team"]["max_k_of_ns"][5]:
            raise ValueError(f"{who} serves the five-state family up to {ROUTES['team']['max_k_of_ns'][5]} agents, this batch has k = {k}")
        nw, kc_lim, kc_max, bits = (k + 63) // 64, min(k, _lib.MAX_AGENTS), 1, None
        others = (("U_ff", U_ff, (B, T, m)),)
        if Kc is not None:
            sk = _shape(Kc)
            if len(sk) != 5 or sk[:4] != (B, T, k, nc) or sk[4] < ns or sk[4] % ns or sk[4] > kc_lim * ns:
                raise ValueError(f"{who}: Kc has shape {sk}, expected ({B}, {T}, {k}, {nc}, kc_max * {ns}) with 1 <= kc_max <= {kc_lim}")
            kc_max = sk[4] // ns
            if nbr_bits is None:
                raise ValueError(f"{who}: gains without neighbourhood masks")
            others += (("nbr_bits", nbr_bits, (B, k, nw)),)
        S, L = self._advance_shapes(who, X, h, state, scen, W, u_lim, n_d, others, wide=True)
        if Kc is not None:
            if _masks_trusted(masks_checked, nbr_bits):
                bits = nbr_bits.contiguous()
            else:
                bits = torch.from_numpy(self._checked_masks_wide(who, nbr_bits, kc_max)).to(device())
            Kc = self._in(Kc, (B, T, k, nc, kc_max * ns))
        X, U_ff, scen, W, u_lim, st = self._advance_args(X, U_ff, state, scen, W, u_lim, S, L)
        _lib.check(self._lib.dpilqr_policy_advance_dec_wide(self._d, ptr(X), ptr(U_ff), ptr(Kc), kc_max, ptr(bits), int(h), ptr(scen), S, L,
                                                            int(n_d), ptr(W), ptr(u_lim), *st, nw, stream_handle()))
        return state

    def cost(self, x, u, terminal=False):
        """GameCost.__call__ at n_pts points per item: x (B,n_pts,n_x), u (B,n_pts,n_u) -> (B,n_pts)."""
        return self._cost("dpilqr_cost_eval", x, u, terminal)

    def cost_wide(self, x, u, terminal=False):
        """cost for a team of up to 256 agents (dpilqr_cost_eval_wide, include/dpilqr_swarm_advance.h): the same kernel, so at
        k <= 64 the same bits.  One thread per point walks all k (k - 1) / 2 pairs: for a few points (a loop's terminal cost)."""
        if self.k > _lib.MAX_TEAM:
            raise ValueError(f"cost_wide serves teams of up to {_lib.MAX_TEAM} agents, this batch has k = {self.k}")
        return self._cost("dpilqr_cost_eval_wide", x, u, terminal)

    def _cost(self, entry, x, u, terminal):
        x = to_dev(x).reshape(self.B, -1, self.n_x).contiguous()
        n_pts = x.shape[1]
        u = to_dev(u).reshape(self.B, n_pts, self.n_u).contiguous()
        out = empty((self.B, n_pts))
        _lib.check(getattr(self._lib, entry)(self._d, n_pts, ptr(x), ptr(u), int(bool(terminal)), ptr(out), stream_handle()))
        return out

    # ------------------------------------------------------------------ whole solve
    def workspace_bytes(self, window, gains_in_ws, dtype=torch.float64):
        fn = self._lib.dpilqr_solve_workspace_bytes if dtype == torch.float64 else self._lib.dpilqr_solve_workspace_bytes_f32
        nbytes = fn(self._d, int(window), int(bool(gains_in_ws)))
        _lib.check(nbytes)
        return int(nbytes)

    def default_window(self, dtype=torch.float64):
        """Items in flight when the caller does not say: 6144 (two rounds of three sweep wavefronts per SIMD on an
        MI355X) for small clusters, fewer where the per-item buffers (gains, line-search candidates; tile records where a
        record-fed sweep serves the batch) are large, so that one solve's workspace stays near 4 GB: several cluster sizes
        are solved concurrently (dispatch.py), and workspaces of 10 GB each did not fit the pool of reusable buffers --
        the fresh multi-GB allocations that followed cost a many-scenario call up to half a second, at random.  The
        workgroup-per-item sweeps hold 2-4 sub-problems per CU, so a thousand in flight fill the device: never below
        1024, except on the large-cluster path (one workgroup per item: 256 = one per CU)."""
        per_item = self.workspace_bytes(2, True, dtype) - self.workspace_bytes(1, True, dtype)
        floor = 256 if (self.fused_sweep or dtype != torch.float64) else 1024
        w = max(floor, (4 << 30) // max(per_item, 1))
        if self.n_x <= 24 and dtype == torch.float64:
            # the wavefront sweeps deal items in layers of 1024 (one wavefront per SIMD of every CU): a window of 2450 items
            # would run every sweep as a full round plus a fifth of one
            w = max(1024, (w // 1024) * 1024)
        return int(min(self.B, 6144, w))

    def solve(self, x0, U0, n_lqr_iter=50, tol=1e-3, trace=False, gains=False, window=None, dtype=torch.float64, out=None,
              progress=None, t_kill=None):
        """ilqrSolver.solve (control.py:150-225) for all B items.

        window: most items in flight at once (default: default_window()); finished items are retired on the device and
        replaced by not-yet-started ones, so launches stay full and memory is bounded.
        out: dict of pre-allocated device tensors X (B,T+1,n_x), U (B,T,n_u), J (B,), status, n_bwd, n_fwd (B,) int32 to
        write the results into (sharding.ResultBuffers: the solve then writes straight into the collective's send buffer).
        progress: callable(n_finished, n_items), called from inside the solve as a PREFIX of the batch finishes (X, U,
        status, n_bwd, n_fwd of items below n_finished are final; see dpilqr_solver_set_progress).
        t_kill: seconds of solve time each item may use (control.py:213-218, every item's clock starts when it is admitted
        to the window); an item whose time is up after an accepted, unconverged step ends with status STATUS_KILLED and
        that step's iterate.  None / 0: no limit.
        Returns a dict of device tensors: X, U, J, status, n_bwd, n_fwd (+ trace, K, d on request).
        """
        B, T, n, m = self.B, self.T, self.n_x, self.n_u
        window = self.default_window(dtype) if window is None else int(window)
        x0 = self._in(x0, (B, n), dtype)
        if out is not None:
            U = out["U"]; U.copy_(self._in(U0, (B, T, m), dtype))
            X, J, status, n_bwd, n_fwd = out["X"], out["J"], out["status"], out["n_bwd"], out["n_fwd"]
            for t_, shp, dt_ in ((X, (B, T + 1, n), dtype), (U, (B, T, m), dtype), (J, (B,), torch.float64),
                                 (status, (B,), torch.int32), (n_bwd, (B,), torch.int32), (n_fwd, (B,), torch.int32)):
                if tuple(t_.shape) != shp or t_.dtype != dt_ or not t_.is_contiguous():
                    raise ValueError(f"out tensor of shape {tuple(t_.shape)} / {t_.dtype}: expected contiguous {shp} {dt_}")
        else:
            U = self._in(U0, (B, T, m), dtype).clone()
            X = empty((B, T + 1, n), dtype); J = empty((B,))
            status = empty((B,), torch.int32); n_bwd = empty((B,), torch.int32); n_fwd = empty((B,), torch.int32)
        tr = torch.full((B, max(n_lqr_iter, 1), 5), float("nan"), dtype=torch.float64, device=device()) if trace else None
        K = empty((B, T, m, n), dtype) if gains else None
        d = empty((B, T, m), dtype) if gains else None
        ws = _workspace_pool.acquire(self.workspace_bytes(window, not gains, dtype))
        fn = self._lib.dpilqr_solve_batch if dtype == torch.float64 else self._lib.dpilqr_solve_batch_f32
        out = dict(X=X, U=U, J=J, status=status, n_bwd=n_bwd, n_fwd=n_fwd)
        if trace:
            out["trace"] = tr
        if gains:
            out["K"], out["d"] = K, d
        ok = False
        try:
            with _lib.progress_callback(progress):
                _lib.check(fn(_lib.solver(), self._d, ptr(x0), ptr(U), int(n_lqr_iter), float(tol), float(t_kill or 0.0), window,
                              ptr(ws), ws.numel(),
                              ptr(X), ptr(J), ptr(status), ptr(n_bwd), ptr(n_fwd), ptr(tr), ptr(K), ptr(d), stream_handle()))
            ok = True
        except _lib.DpilqrError as e:
            # DPILQR_EHIP because the device gave items up (STATUS_FAULT): the solve ran to its end, the other items' results
            # are valid -- they travel with the exception
            e.results = out
            raise
        finally:
            if ok:
                _workspace_pool.release(ws)   # solve_batch has synchronised its stream: the buffer is idle
            # a failed solve's buffer is dropped, not pooled: the allocator frees it in stream order
        return out

    def solve_enqueue(self, x0, U0, n_global_iter, n_lqr_iter=None, tol=None, window=None, state=None, t_kill=None):
        """The same solve as pure enqueue on torch's current stream (dpilqr_solve_enqueue): nothing is waited for.
        Returns (results dict, state); pass `state` back to continue with another n_global_iter iterations.  An item is
        finished when its status is no longer 0 (STATUS_ACTIVE).
        n_lqr_iter (default 50), tol (1e-3) and t_kill (none) are fixed by the FIRST call and kept in `state`: a continuing call
        need not repeat them and may not change them (the per-item admission clocks t_kill reads are stamped only by a solve that
        started with a limit)."""
        B, T, n, m = self.B, self.T, self.n_x, self.n_u
        if state is None:
            window = self.default_window() if window is None else int(window)
            x0 = self._in(x0, (B, n)); U = self._in(U0, (B, T, m)).clone()
            r = dict(X=empty((B, T + 1, n)), U=U, J=empty((B,)), status=empty((B,), torch.int32),
                     n_bwd=empty((B,), torch.int32), n_fwd=empty((B,), torch.int32))
            ws = torch.empty(self.workspace_bytes(window, True), dtype=torch.uint8, device=device())
            state = dict(r=r, ws=ws, x0=x0, window=window, resume=0, n_lqr_iter=int(50 if n_lqr_iter is None else n_lqr_iter),
                         tol=float(1e-3 if tol is None else tol), t_kill=float(t_kill or 0.0))
        else:
            for name, given in (("n_lqr_iter", n_lqr_iter), ("tol", tol), ("t_kill", t_kill)):
                if given is not None and float(given) != float(state[name]):
                    raise ValueError(f"solve_enqueue: {name}={given} on a continuing call, the solve was started with {state[name]}")
        r, ws = state["r"], state["ws"]
        _lib.check(self._lib.dpilqr_solve_enqueue(self._d, ptr(state["x0"]), ptr(r["U"]), state["n_lqr_iter"], state["tol"],
                                                  state["t_kill"], state["window"], ptr(ws), ws.numel(), ptr(r["X"]), ptr(r["J"]),
                                                  ptr(r["status"]), ptr(r["n_bwd"]), ptr(r["n_fwd"]), None, None, None,
                                                  int(n_global_iter), state["resume"], stream_handle()))
        state["resume"] = 1
        return r, state

    def iterations_bound(self, n_lqr_iter=50, window=None):
        window = self.default_window() if window is None else int(window)
        return int(self._lib.dpilqr_solve_iterations_bound(self._d, window, int(n_lqr_iter)))


def backward_pass_tiles(tiles, B, T, n_x, n_u, mu, singular=None, blocks=None):
    """The Riccati sweep on explicit tile records -- the plugin contract (any linearize/quadraticize).

    blocks=(n_s, n_c): the caller's promise that A, B of every record are block diagonal with per-agent
    blocks of that size (MultiDynamicalModel.linearize, dynamics.py:173-186); same gains, fewer products."""
    lib = _lib.load()
    mu_t = to_dev(np.broadcast_to(np.asarray(mu, dtype=np.float64), (B,))) if not isinstance(mu, torch.Tensor) else mu
    K = empty((B, T, n_u, n_x)); d = empty((B, T, n_u))
    ns, nc = blocks if blocks else (0, 0)
    _lib.check(lib.dpilqr_backward_pass_tiles_blocks(B, T, n_x, n_u, ns, nc, ptr(tiles), ptr(mu_t), ptr(K), ptr(d),
                                                     ptr(singular), None, None, stream_handle()))
    return K, d


def pack_tiles(A, Bm, Lx, Lu, Lxx, Luu, Lux):
    """Host plugin outputs -> device tile records.

    A (B,T,n,n), Bm (B,T,n,m); Lx (B,T+1,n), Lu (B,T+1,m), Lxx (B,T+1,n,n), Luu (B,T+1,m,m),
    Lux (B,T+1,m,n), entry T being the terminal quadraticisation.
    """
    A = np.asarray(A, dtype=np.float64); Bm = np.asarray(Bm, dtype=np.float64)
    Bn, T, n, m = Bm.shape
    lay, stride = _lib.tile_layout(n, m)
    rec = np.zeros((Bn, T + 1, stride))

    def put(key, arr, rows, cols, steps):
        off, ld = lay[key]
        idx = off + (np.arange(rows) * ld)[:, None] + np.arange(cols)[None, :]
        rec[:, :steps, idx] = np.asarray(arr, dtype=np.float64).reshape(Bn, steps, rows, cols)

    put("A", A, n, n, T); put("B", Bm, n, m, T)
    put("Lxx", Lxx, n, n, T + 1); put("Lux", Lux, m, n, T + 1); put("Luu", Luu, m, m, T + 1)
    put("Lx", Lx, 1, n, T + 1); put("Lu", Lu, 1, m, T + 1)
    return to_dev(rec)
