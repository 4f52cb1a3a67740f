"""Host helpers around the hot path: agent slicing, graph splitting, scenario generation.

Mirrors the names of the reference's dpilqr/util.py that the hot path and its callers use
(util.py:20-117,125-236).  These are bookkeeping on small host arrays (shapes, ids, RNG draws);
no solver arithmetic happens here.
"""
import itertools
from dataclasses import dataclass

import numpy as np

π = np.pi


@dataclass
class Point:
    """3-D point with z defaulting to 0 (util.py:20-45)."""
    x: float
    y: float
    z: float = 0

    @property
    def ndim(self):
        return 3 if self.z != 0 else 2

    def _zip(self, other, op):
        return Point(op(self.x, other.x), op(self.y, other.y), op(self.z, other.z))

    def __add__(self, other):
        return self._zip(other, lambda a, b: a + b)

    def __sub__(self, other):
        return self._zip(other, lambda a, b: a - b)

    def __mul__(self, other):
        return self._zip(other, lambda a, b: a * b)

    def hypot2(self):
        return self.x ** 2 + self.y ** 2 + self.z ** 2

    def __repr__(self):
        return str((self.x, self.y, self.z))


def _pairs(n):
    return list(itertools.combinations(range(n), 2))


def compute_pairwise_distance(X, x_dims, n_d=2):
    """Distances between every pair of agents over the first n_d coordinates (util.py:48-61).
    X: (N, n_x) or (n_x,); returns (N, n_pairs) in itertools.combinations order."""
    if len(set(x_dims)) != 1:
        raise AssertionError("agents must share one state dimension")
    k, ns = len(x_dims), x_dims[0]
    if k == 1:
        raise ValueError("Can't compute pairwise distance for one agent.")
    P = np.asarray(X, dtype=float).reshape(-1, k, ns)[:, :, :n_d]
    ij = np.array(_pairs(k))
    diff = P[:, ij[:, 0], :] - P[:, ij[:, 1], :]
    return np.sqrt(np.sum(diff * diff, axis=2))


def compute_pairwise_distance_nd(X, x_dims, n_dims, dec_ind=None):
    """Like compute_pairwise_distance with min(n_dims_i, n_dims_j) coordinates per pair (util.py:64-87)."""
    X = np.atleast_2d(np.asarray(X, dtype=float))
    ns, k = x_dims[0], len(x_dims)
    cols = []
    for i, j in _pairs(k):
        if dec_ind is not None and dec_ind not in (i, j):
            continue
        nd = min(n_dims[i], n_dims[j])
        diff = X[:, i * ns:i * ns + nd] - X[:, j * ns:j * ns + nd]
        cols.append(np.sqrt(np.sum(diff * diff, axis=1)))
    return np.stack(cols, axis=1) if cols else np.zeros((X.shape[0], 0))


def split_agents(Z, z_dims):
    """Column-split a joint state/control into per-agent pieces (util.py:90-92)."""
    return np.split(np.atleast_2d(Z), np.cumsum(z_dims[:-1]), axis=1)


def split_agents_gen(z, z_dims):
    """Generator over per-agent slices; uses z_dims[0] for every agent like the reference (util.py:95-99)."""
    w = z_dims[0]
    for i in range(len(z_dims)):
        yield z[i * w:(i + 1) * w]


def split_graph(Z, z_dims, graph):
    """Gather, for every sub-problem of `graph`, the columns of its member agents (util.py:102-117)."""
    if len(set(z_dims)) != 1:
        raise AssertionError("agents must share one dimension")
    w = z_dims[0]
    where = {id_: pos for pos, id_ in enumerate(graph)}
    return [np.concatenate([Z[:, where[i] * w:(where[i] + 1) * w] for i in members], axis=1)
            for members in graph.values()]


def pos_mask(x_dims, n_d=2):
    return np.array([(i % x_dims[0]) < n_d for i in range(sum(x_dims))])


def uniform_block_diag(*arrs):
    """Block-diagonal matrix of equally shaped blocks (util.py:229-236)."""
    r, c = arrs[0].shape
    out = np.zeros((len(arrs) * r, len(arrs) * c))
    for i, blk in enumerate(arrs):
        out[i * r:(i + 1) * r, i * c:(i + 1) * c] = blk
    return out


def distance_to_goal(x, x_goal, n_agents, n_states, n_d):
    return np.linalg.norm((x - x_goal).reshape(n_agents, n_states)[:, :n_d], axis=1)


# ------------------------------------------------------------------ scenario generation
# The Monte-Carlo scenario distribution of scripts/analysis.py:45-54 draws from NumPy's legacy global
# RNG; the calls below are made in the same order so that np.random.seed(s) reproduces its scenarios.

def randomize_locs(n_pts, random=False, rel_dist=3.0, var=3.0, n_d=2):
    """util.py:125-149: uniform points in [-var, var]^n_d; unless `random`, pushed apart until every
    pair is farther than rel_dist."""
    x = var * np.random.uniform(-1, 1, (n_pts, n_d))
    if random:
        return x
    push = 0.1 * n_pts
    ij = np.array(_pairs(n_pts))
    while True:
        centre = x.mean(axis=0)
        dist = compute_pairwise_distance(x.flatten(), [n_d] * n_pts, n_d=2).T
        close = ij[dist.flatten() <= rel_dist]
        if not close.size:
            return x
        x[close] += push * (x[close] - centre)


def separate_locs(x, rel_dist, max_iter=None):
    """The loop of randomize_locs(random=False) on a (k, n_d) array that is already drawn, stated point by point as the device
    computes it (include/dpilqr_separated_setup.h): per round the centre, the distances over the first two coordinates, a flag per
    point with another point within rel_dist, and every flagged point pushed once, x + 0.1 k (x - centre), all from the old
    positions.  Returns (x, rounds): a copy, and the number of rounds, the last one -- which finds no flag -- included.  With
    max_iter, a set that still has a flagged point in round max_iter comes back as it stands after that round's push, with
    rounds = -1.  One point raises like the reference's compute_pairwise_distance."""
    x = np.array(x, dtype=np.float64)
    k, n_d = x.shape
    if k == 1:
        raise ValueError("Can't compute pairwise distance for one agent.")
    push = 0.1 * k
    rounds = 0
    while True:
        rounds += 1
        centre = x.mean(axis=0)
        with np.errstate(invalid="ignore", over="ignore"):
            d = x[:, None, :2] - x[None, :, :2]
            q = d[..., 0] * d[..., 0]
            if d.shape[2] == 2:
                q = q + d[..., 1] * d[..., 1]
            close = np.sqrt(q) <= rel_dist
            np.fill_diagonal(close, False)
            flag = close.any(axis=1)
            if not flag.any():
                return x, rounds
            x[flag] = x[flag] + push * (x[flag] - centre)
        if max_iter is not None and rounds >= max_iter:
            return x, -1


def compute_energy(x, x_dims, n_d=2):
    return np.linalg.norm(x[pos_mask(x_dims, n_d)].reshape(-1, n_d), axis=1).sum()


def normalize_energy(x, x_dims, energy=10.0, n_d=2):
    """Centre the positions and scale them so the summed distance from the origin is `energy` (util.py:203-217)."""
    x = x.copy()
    mask = pos_mask(x_dims, n_d)
    centre = x[mask].reshape(-1, n_d).mean(0)
    x[mask] -= np.tile(centre, len(x_dims)).reshape(-1, 1)
    x[mask] *= energy / compute_energy(x, x_dims, n_d)
    return x


def random_setup(n_agents, n_states, is_rotation=False, n_d=2, energy=None, do_face=False, **kwargs):
    """Random start/goal pair (util.py:165-195).  Rotation/facing variants are not part of the hot path's
    scenario distribution and are not provided."""
    if is_rotation or do_face:
        raise NotImplementedError("only the is_rotation=False, do_face=False scenarios of scripts/analysis.py")
    starts = randomize_locs(n_agents, n_d=n_d, **kwargs)
    goals = randomize_locs(n_agents, n_d=n_d, **kwargs)
    pad = np.zeros((n_agents, n_states - n_d))
    x0 = np.c_[starts, pad].reshape(-1, 1)
    xf = np.c_[goals, pad].reshape(-1, 1)
    if energy:
        dims = [n_states] * n_agents
        x0 = normalize_energy(x0, dims, energy, n_d)
        xf = normalize_energy(xf, dims, energy, n_d)
    return x0, xf


def perturb_state(x, x_dims, n_d=2, var=0.5):
    x = x.copy()
    mask = pos_mask(x_dims, n_d)
    x[mask] += var * np.random.randn(*x[mask].shape)
    return x


def perturbed_starts(x0, x_dims, n_samples, n_d=2, var=0.5, seed=None):
    """(n_samples, n_x) starts around x0 for a closed-loop ensemble (ilqrSolver.closed_loop, ProblemBatch.policy_rollout): row i
    is what the i-th call of perturb_state(x0, x_dims, n_d, var) returns after np.random.seed(seed) -- host NumPy, the legacy
    global stream, so that the ensemble is the one a loop over the reference's perturb_state draws.  seed=None: the stream as
    it stands."""
    if seed is not None:
        np.random.seed(seed)
    x0 = np.asarray(x0, dtype=np.float64)
    return np.stack([perturb_state(x0, x_dims, n_d=n_d, var=var).reshape(-1) for _ in range(int(n_samples))])


def separate_setups(x0, xf, seeds, n_agents, n_states, n_d, rel_dist, energy, max_iter=256, who="separate_setups"):
    """dpilqr_setup_separate (include/dpilqr_separated_setup.h) on device tensors x0, xf (S, n_agents * n_states) of RAW draws, in
    place: the position columns become those of random_setup(..., rel_dist=rel_dist, random=False, energy=energy).  The (S, 2)
    round counts (starts, goals) are read back once and returned; a set that did not separate within max_iter rounds is a
    ValueError naming its seed (seeds: the S seeds, for that message) and set."""
    from . import _lib
    if n_agents == 1:
        raise ValueError("Can't compute pairwise distance for one agent.")
    if not 2 <= n_agents <= _lib.MAX_TEAM:
        raise ValueError(f"{who}: {n_agents} agents -- separated=True serves teams of 2 .. {_lib.MAX_TEAM}")
    import torch
    from .device import empty, ptr, stream_handle
    S = x0.shape[0]
    n_iter = empty((S, 2), torch.int32)
    _lib.check(_lib.load().dpilqr_setup_separate(S, n_agents, n_states, n_d, float(rel_dist), float(energy or 0.0), int(max_iter), ptr(x0),
                                                 ptr(xf), ptr(n_iter), stream_handle()))
    rounds = n_iter.cpu().numpy()
    if (rounds < 0).any():
        stuck = ", ".join(f"seed {int(seeds[s])} ({'starts' if w == 0 else 'goals'})" for s, w in np.argwhere(rounds < 0))
        raise ValueError(f"{who}: not separated to rel_dist={rel_dist} within max_iter={max_iter} rounds: {stuck}")
    return rounds


def random_setup_batch(seeds, n_agents, n_states, var, n_d=2, energy=None, wide=False, separated=False, rel_dist=3.0, max_iter=256,
                       return_rounds=False):
    """(x0, xf) device tensors (S, n_agents * n_states) of the scenarios np.random.seed(s); random_setup(n_agents, n_states,
    is_rotation=False, var=var, n_d=n_d, random=True, energy=energy) for s in range(seeds[0], seeds[0] + S) -- generated on
    the device, bit for bit what the host loop gives (dpilqr_random_setup).  seeds: (first seed, count) or a range.
    Without wide=True a team of more than 64 agents is a ValueError (that generator keeps a team's draws in one thread's private
    memory).  wide=True serves 1 .. 256 agents through dpilqr_trial_inputs with no warm start (include/dpilqr_swarm_study.h: a
    wavefront per scenario, the generator's state in LDS), the same bits where both serve.
    separated=True: random_setup(..., rel_dist=rel_dist, random=False, ...) instead -- every pair of starts and every pair of goals
    farther apart than rel_dist before the energy is normalised -- for 2 .. 256 agents whatever `wide` is: the raw draws of
    dpilqr_trial_inputs, then dpilqr_setup_separate (include/dpilqr_separated_setup.h).  The round counts are read back once; a
    set that did not separate within max_iter rounds is a ValueError naming its seed.  return_rounds=True (separated only) also
    returns the (S, 2) counts of the start and goal sets."""
    from . import _lib
    if separated:
        if n_agents == 1:
            raise ValueError("Can't compute pairwise distance for one agent.")
        if not 2 <= n_agents <= _lib.MAX_TEAM:
            raise ValueError(f"random_setup_batch: {n_agents} agents -- separated=True serves teams of 2 .. {_lib.MAX_TEAM}")
        from .device import empty, ptr, stream_handle
        if isinstance(seeds, range) and seeds.step != 1:
            raise ValueError("consecutive seeds only")
        seed0, S = (seeds.start, len(seeds)) if isinstance(seeds, range) else (int(seeds[0]), int(seeds[1]))
        x0 = empty((S, n_agents * n_states)); xf = empty((S, n_agents * n_states))
        _lib.check(_lib.load().dpilqr_trial_inputs(S, seed0, None, n_agents, n_states, n_d, float(var), 0.0, 0, 0, 0, 0.0, ptr(x0), ptr(xf),
                                                   None, None, stream_handle()))
        rounds = separate_setups(x0, xf, range(seed0, seed0 + S), n_agents, n_states, n_d, rel_dist, energy, max_iter, "random_setup_batch")
        return (x0, xf, rounds) if return_rounds else (x0, xf)
    if return_rounds:
        raise ValueError("random_setup_batch: return_rounds=True goes with separated=True")
    if wide:
        if not 1 <= n_agents <= _lib.MAX_TEAM:
            raise ValueError(f"random_setup_batch: {n_agents} agents -- wide=True serves teams of 1 .. {_lib.MAX_TEAM}")
        from .device import empty, ptr, stream_handle
        if isinstance(seeds, range) and seeds.step != 1:
            raise ValueError("consecutive seeds only")
        seed0, S = (seeds.start, len(seeds)) if isinstance(seeds, range) else (int(seeds[0]), int(seeds[1]))
        x0 = empty((S, n_agents * n_states)); xf = empty((S, n_agents * n_states))
        _lib.check(_lib.load().dpilqr_trial_inputs(S, seed0, None, n_agents, n_states, n_d, float(var), float(energy or 0.0), 0, 0, 0, 0.0,
                                                   ptr(x0), ptr(xf), None, None, stream_handle()))
        return x0, xf
    if n_agents > _lib.MAX_AGENTS:
        raise ValueError(f"random_setup_batch: {n_agents} agents -- the device generator is not built for teams of more than "
                         f"{_lib.MAX_AGENTS}; draw the scenarios on the host (util.random_setup)")
    from .device import empty, ptr, stream_handle
    seed0, S = (seeds.start, len(seeds)) if isinstance(seeds, range) else (int(seeds[0]), int(seeds[1]))
    if isinstance(seeds, range) and seeds.step != 1:
        raise ValueError("consecutive seeds only")
    x0 = empty((S, n_agents * n_states)); xf = empty((S, n_agents * n_states))
    _lib.check(_lib.load().dpilqr_random_setup(S, seed0, n_agents, n_states, n_d, float(var), float(energy or 0.0), ptr(x0), ptr(xf),
                                               stream_handle()))
    return x0, xf
