"""The Monte-Carlo study of the reference (scripts/analysis.py:35-107 multi_agent_run, :110-123 setup_logger,
:126-174 monte_carlo_analysis) over the batched device path: centralized vs distributed receding-horizon control over
models x team sizes x trials, logged as the reference's CSV.

The reference runs one trial at a time: random_setup, solve_rhc(centralized=True), solve_rhc(centralized=False), each a
loop of single solves.  Here all trials of one (model, team size) run in lock step -- every receding-horizon round of
every trial is ONE batched solve (distributed.solve_rhc_scenarios) -- and the rows come out in the reference's order
(trial by trial, the centralized branch's rows, then the distributed branch's).

Randomness.  The reference never seeds: a trial consumes NumPy's global stream for random_setup and then for the warm
start of each branch's solve_rhc (distributed.py:152).  Here trial i of a (model, team size) cell is seeded
(np.random.seed(seed_of(...))) and consumes the stream in exactly that order, so a trial is reproducible and a
per-trial run of solve_rhc on the same seed sees the same inputs (tests/test_gpu_analysis.py compares the rows).

limit_solve_time (analysis 2, the reference's default, analysis.py:179): t_kill = dt reaches every solve -- inside the
batched device solve (include/dpilqr_hip.h: every item's own clock from its admission) -- and t_diverge = N dt.
What that clock measures differs in kind from the reference's: there a solve has a CPU core to itself and perf_counter() runs
over its own work; here an item shares every launch with the rest of the window, so its elapsed time includes the work the GPU
does for up to `window` other items.  Which solves are killed therefore depends on the batch size, the window and whatever else
the GPU runs, and varies from run to run: analysis-2 rows answer "what does a real-time budget of dt buy on THIS device at THIS
load", not the reference's question, and cannot be compared row by row with its CSV.  For a reproducible budget pass
n_lqr_iter (a cap on iterations per solve, deterministic) instead of, or beside, limit_solve_time.
"""
import logging
from os import getpid
from pathlib import Path
from time import strftime

import numpy as np

from .cost import GameCost, ProximityCost, ReferenceCost
from .distributed import solve_rhc_scenarios
from .dynamics import DoubleIntDynamics4D, MultiDynamicalModel, QuadcopterDynamics6D, UnicycleDynamics4D
from .problem import ilqrProblem
from .util import random_setup, separate_setups, split_agents_gen

HEADER = "dynamics,n_agents,trial,centralized,last,t,J,horizon,dt,converged,ids,times,subgraphs,dist_left"   # analysis.py:120-123
STEP_SIZE = 3                                                                                                # analysis.py:43
MODELS = (DoubleIntDynamics4D, UnicycleDynamics4D, QuadcopterDynamics6D)                                     # analysis.py:133-137


def seed_of(model, n_agents, i_trial, seed0=0):
    """The seed of one trial: distinct per (model, team size, trial), stable across runs."""
    return int(seed0) + 100003 * MODELS.index(model) + 1009 * int(n_agents) + int(i_trial)


def trial_inputs(n_agents, n_states, n_u, N, energy, n_d, seed, separated=False, rel_dist=None):
    """What one trial of multi_agent_run draws, in the order the reference draws it: (x0, xf) from random_setup
    (analysis.py:45-54), then the warm start of the centralized and of the distributed solve_rhc (distributed.py:152).
    separated=True: random_setup's random=False with the same arguments -- every pair of starts and of goals farther apart than
    rel_dist (None: n_agents, what the study passes) before the energy is normalised.  The push draws nothing: the warm starts are
    those of separated=False."""
    np.random.seed(seed)
    x0, xf = random_setup(n_agents, n_states, is_rotation=False, rel_dist=n_agents if rel_dist is None else rel_dist, var=n_agents / 2,
                          n_d=n_d, random=not separated, energy=energy)
    U_c = np.random.rand(N, n_u) * 0.01
    U_d = np.random.rand(N, n_u) * 0.01
    return x0, xf, U_c, U_d


def trial_inputs_batch(n_agents, n_states, n_u, N, energy, n_d, seeds, separated=False, rel_dist=None, max_iter=256):
    """trial_inputs for the S trials seeded `seeds`, drawn on the device (dpilqr_trial_inputs, include/dpilqr_swarm_study.h): device
    tensors x0, xf (S, n_agents * n_states) and U_c, U_d (S, N, n_u), bit for bit trial_inputs' four arrays of every seed, for
    teams of 1 .. 256 agents -- var = n_agents / 2 and the warm starts scaled by 0.01 as there.  seeds: any sequence of integers
    of [0, 2^32); a consecutive run is passed as its first seed, anything else as a device array.
    separated=True: trial_inputs(separated=True)'s arrays for teams of 2 .. 256 agents -- the raw draws (energy 0), then
    dpilqr_setup_separate (include/dpilqr_separated_setup.h) with rel_dist (None: n_agents); the round counts are read back once and
    a set that did not separate within max_iter rounds is a ValueError naming its seed (util.separate_setups)."""
    import torch
    from . import _lib
    from .device import empty, ptr, stream_handle, to_dev
    seeds = [int(s) for s in seeds]
    S = len(seeds)
    if separated and n_agents == 1:
        raise ValueError("Can't compute pairwise distance for one agent.")
    if not 1 <= n_agents <= _lib.MAX_TEAM:
        raise ValueError(f"trial_inputs_batch: {n_agents} agents -- the device generator serves teams of 1 .. {_lib.MAX_TEAM}")
    if any(not 0 <= s < 2 ** 32 for s in seeds):
        raise ValueError("trial_inputs_batch: np.random.seed takes seeds of [0, 2^32)")
    x0 = empty((S, n_agents * n_states)); xf = empty((S, n_agents * n_states))
    U_c = empty((S, N, n_u)); U_d = empty((S, N, n_u))
    consecutive = all(b == a + 1 for a, b in zip(seeds, seeds[1:]))
    seeds_d = None if consecutive else to_dev(torch.tensor(seeds, dtype=torch.int64), torch.int64)
    _lib.check(_lib.load().dpilqr_trial_inputs(S, seeds[0] if S and consecutive else 0, ptr(seeds_d), n_agents, n_states, n_d,
                                               float(n_agents / 2), 0.0 if separated else float(energy or 0.0), 2, N, n_u, 0.01, ptr(x0),
                                               ptr(xf), ptr(U_c), ptr(U_d), stream_handle()))
    if separated:
        separate_setups(x0, xf, seeds, n_agents, n_states, n_d, float(n_agents if rel_dist is None else rel_dist), energy, max_iter,
                        "trial_inputs_batch")
    return x0, xf, U_c, U_d


def weights_of(model, n_states):
    """analysis.py:62-69"""
    if model in (DoubleIntDynamics4D, UnicycleDynamics4D):
        Q = 1.0 * np.diag([1, 1] + [0] * (n_states - 2)); R = np.eye(2)
    elif model is QuadcopterDynamics6D:
        Q = np.eye(n_states) * 50; R = np.eye(3)
    else:
        raise ValueError(f"no weights defined for {model.__name__} (analysis.py:62-67 knows three models)")
    return Q, R, 1000.0 * np.eye(n_states)


def build_problem(model, n_agents, dt, radius, xf, n_d):
    """analysis.py:56-78: ids 100.., one ReferenceCost per agent, the proximity cost, the game cost, the problem."""
    n_states = model(-1).n_x
    x_dims, n_dims = [n_states] * n_agents, [n_d] * n_agents
    ids = [100 + i for i in range(n_agents)]
    dynamics = MultiDynamicalModel([model(dt, id_) for id_ in ids])
    Q, R, Qf = weights_of(model, n_states)
    goal_costs = [ReferenceCost(xf_i, Q.copy(), R.copy(), Qf.copy(), id_)
                  for xf_i, id_ in zip(split_agents_gen(np.asarray(xf).reshape(-1, 1), x_dims), ids)]
    return ilqrProblem(dynamics, GameCost(goal_costs, ProximityCost(x_dims, radius, n_dims)))


def multi_agent_run(model, x_dims, dt, N, radius, energy=10.0, n_d=2, trials=(0,), seed0=0, emit=logging.info, window=None,
                    branches=(True, False), wide=False, max_cluster=None, device_inputs=False, separated=False, **kwargs):
    """multi_agent_run (analysis.py:35-107) for all `trials` of one (model, team size) at once: both branches, every
    receding-horizon round of every trial one batched solve.  kwargs as the reference passes them: t_kill, dist_converge,
    t_diverge (i_trial is replaced by `trials`; energy is consumed here).  Emits the rows in the reference's order and
    returns {trial: ((Xc, Uc, Jc, converged), (Xd, Ud, Jd, converged))}.
    branches: which of the two loops run, as values of `centralized` -- (True, False) both, (False,) the distributed loop alone,
    whose rows are then the only ones emitted (in the order they have in the two-branch run) and whose tuple is the only one
    returned per trial.  A trial draws what it always draws -- both warm starts, the distributed loop takes the second -- so the
    rows of a branch do not depend on which other branch ran.
    wide, max_cluster reach the distributed branch's solve_rhc_scenarios: with wide=True a swarm of up to 256 agents is studied,
    distributed only (no centralized solve is built above n_x = 240: wide=True with True in branches is a ValueError).
    device_inputs=True draws the trials' inputs on the device (trial_inputs_batch: the same bits) and hands the device tensors
    to the loops; they never come to the host.
    separated=True draws every trial with trial_inputs(separated=True) -- random_setup's random=False, pairs of starts and of goals
    farther apart than rel_dist = n_agents before normalisation -- on either input path (the same bits)."""
    if not len(set(x_dims)) == 1:
        raise ValueError("Dynamics dimensions must be consistent")
    branches = tuple(bool(b) for b in branches)
    if not branches or len(set(branches)) != len(branches):
        raise ValueError(f"multi_agent_run: branches={branches}, expected a non-empty selection of (True, False) without repeats")
    if wide and True in branches:
        raise ValueError("multi_agent_run: wide=True studies the distributed loop alone (branches=(False,)); no centralized solve "
                         "is built for the teams it serves")
    kwargs.pop("i_trial", None); kwargs.pop("verbose", None)
    n_agents, n_states = len(x_dims), x_dims[0]
    trials = list(trials)
    n_u = n_agents * model(-1).n_u
    seeds = [seed_of(model, n_agents, i, seed0) for i in trials]
    if device_inputs:
        x0, xf, U_c, U_d = trial_inputs_batch(n_agents, n_states, n_u, N, energy, n_d, seeds, separated=separated)
        warm = {True: U_c, False: U_d}
        xf_first = xf[0].cpu().numpy()
    else:
        drawn = [trial_inputs(n_agents, n_states, n_u, N, energy, n_d, seed, separated=separated) for seed in seeds]
        x0 = np.stack([d[0].ravel() for d in drawn]); xf = np.stack([d[1].ravel() for d in drawn])
        warm = {centralized: np.stack([d[col] for d in drawn]) for centralized, col in ((True, 2), (False, 3)) if centralized in branches}
        xf_first = xf[0]
    problem = build_problem(model, n_agents, dt, radius, xf_first, n_d)     # per-trial goals go in as `xf` below
    out, rows = {}, {}
    for centralized in (True, False):
        if centralized not in branches:
            continue
        r = []
        own = {} if centralized else {key: v for key, v in (("wide", wide), ("max_cluster", max_cluster)) if v}
        res = solve_rhc_scenarios(problem, x0, N, radius, xf=xf, U0=warm[centralized], centralized=centralized,
                                  n_d=n_d, step_size=STEP_SIZE, i_trial=trials, rows=r, window=window, **own, **kwargs)
        rows[centralized] = r
        for j, i in enumerate(trials):
            out.setdefault(i, []).append(res[j])
    for j, i in enumerate(trials):
        for centralized in (True, False):
            for row in rows.get(centralized, [[]] * len(trials))[j]:
                emit(row)
    return {i: tuple(v) for i, v in out.items()}


LOGGER_NAME = "dpilqr.analysis"


def setup_logger(limit_solve_time, log_file=None):
    """setup_logger (analysis.py:110-123): logs/dec-mc-{1|2}_<date>_<pid>.csv beside the repository's scripts unless a
    file is named; the header row first.  Returns the path.  The reference configures the ROOT logger of its own script; a
    library must not (the embedding application's handlers are its own): the rows go through the logger `dpilqr.analysis`, which
    gets the file handler and does not propagate."""
    analysis = "1" if not limit_solve_time else "2"
    if log_file is None:
        log_path = Path(__file__).resolve().parent.parent / "logs"
        log_path.mkdir(exist_ok=True)
        log_file = log_path / strftime(f"dec-mc-{analysis}_%m-%d-%y_%H.%M.%S_{getpid()}.csv")
    print(f"Logging results to {log_file}")
    logger = logging.getLogger(LOGGER_NAME)
    for h in list(logger.handlers):            # a previous study's file
        logger.removeHandler(h); h.close()
    handler = logging.FileHandler(log_file)
    handler.setFormatter(logging.Formatter("%(message)s"))
    logger.addHandler(handler)
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.info(HEADER)
    return Path(log_file)


def monte_carlo_analysis(limit_solve_time=False, n_trials=2, n_agents_iter=(3, 4, 5, 6, 7), models=MODELS, dt=0.1, N=50,
                         energy=10.0, radius=0.50, seed0=0, log_file=None, emit=None, window=None, branches=(True, False), wide=False,
                         max_cluster=None, device_inputs=False, separated=False):
    """monte_carlo_analysis (analysis.py:126-174): the same loops, constants and stopping rules; the innermost loop (the
    trials) is the batch.  n_trials may be thousands -- that is what the batched path is for.
    branches, wide, max_cluster, device_inputs, separated: multi_agent_run's, passed through -- branches=(False,), wide=True studies
    swarms of up to 256 agents, distributed only.  energy may be a callable of n_agents: the reference's fixed 10.0 puts 256
    agents within one radius of each other, a swarm needs an energy that grows with the team."""
    if emit is None:
        setup_logger(limit_solve_time, log_file)
        emit = logging.getLogger(LOGGER_NAME).info
    if limit_solve_time:
        t_kill, t_diverge = dt, N * dt
    else:
        t_kill, t_diverge = None, 4 * N * dt
    results = {}
    for model in models:
        print(f"{model.__name__}")
        for n_agents in n_agents_iter:
            print(f"\tn_agents: {n_agents}")
            n_d = 3 if model is QuadcopterDynamics6D else 2
            x_dims = [model(-1).n_x] * n_agents
            results[(model.__name__, n_agents)] = multi_agent_run(
                model, x_dims, dt, N, radius, n_d=n_d, t_kill=t_kill, dist_converge=0.1, t_diverge=t_diverge,
                energy=energy(n_agents) if callable(energy) else energy, trials=range(n_trials), seed0=seed0, emit=emit, window=window,
                branches=branches, wide=wide, max_cluster=max_cluster, device_inputs=device_inputs, separated=separated, verbose=False)
    return results
