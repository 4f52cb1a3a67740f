"""DP-iLQR driver: same entry points as the reference's dpilqr/distributed.py
(solve_distributed :25-103, solve_rhc :106-221, define_inter_graph_threshold :224-247, solve_centralized :250-258).

The per-agent sub-problem loop (and its optional multiprocessing pool) is replaced by one batched device
dispatch (dispatch.solve_problem_list); graph construction and stitching are unchanged in meaning.
"""
import itertools
import logging
from time import perf_counter as pc

import numpy as np

from .control import ilqrSolver
from .dispatch import solve_kwargs, solve_problem_list, solve_scenarios_distributed  # noqa: F401
from .util import compute_pairwise_distance, split_graph


def define_inter_graph_threshold(X, radius, x_dims, ids):
    """Interaction graph {id: sorted ids within 2*radius (planar) at any sampled step, incl. itself}."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n_rows = X.shape[0]
    step = max(n_rows // 10, 1)                      # ~10 samples over the trajectory
    near = compute_pairwise_distance(X, x_dims)[0:n_rows + 1:step] < 2 * radius
    graph = {id_: [id_] for id_ in ids}
    # like the reference (distributed.py:240-246, quirk Q10) the neighbours come out of a NumPy array of id pairs, i.e.
    # as NumPy integers next to the agent's own Python int: they compare and hash like ints, but they print differently
    # inside the `subgraphs` field of solve_rhc's CSV rows, which is reproduced byte for byte
    for col, (a, b) in enumerate(np.array(list(itertools.combinations(ids, 2))).reshape(-1, 2)):
        if near[:, col].any():
            graph[int(a)].append(b)
            graph[int(b)].append(a)
    return {id_: sorted(members) for id_, members in graph.items()}


def nearest_neighbourhoods(X, radius, x_dims, ids, max_cluster):
    """define_inter_graph_threshold with every neighbourhood capped at its max_cluster nearest agents -- the definition of
    include/dpilqr_nearest.h in NumPy.  Over the sampled rows r (the same rows), d_r(i, j) = sqrt(dx*dx + dy*dy) over the planar
    positions, key(i, j) = min_r d_r(i, j) (a comparison with a NaN is false: a NaN distance is never the minimum, a NaN key
    never a neighbour), nbr(i) = {i} + {j : key(i, j) < 2 radius}.  A neighbourhood of at most m = min(max_cluster, k) members is
    kept; a larger one becomes i and the m - 1 members j != i smallest under the lexicographic order on (key(i, j), j): ties go
    to the lower agent index.  The result need not be symmetric.  Returns what define_inter_graph_threshold returns:
    {id: sorted ids, the agent's own included}.  max_cluster: an integer 1 .. 64."""
    from .dispatch import checked_max_cluster
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    k = len(ids)
    m = checked_max_cluster(max_cluster, k)
    n_rows = X.shape[0]
    rows = X[0:n_rows + 1:max(n_rows // 10, 1)]
    start = np.concatenate([[0], np.cumsum(x_dims)[:-1]]).astype(int)
    px, py = rows[:, start], rows[:, start + 1]                       # (rows, k)
    dx, dy = px[:, :, None] - px[:, None, :], py[:, :, None] - py[:, None, :]
    with np.errstate(invalid="ignore"):
        key = np.fmin.reduce(np.sqrt(dx * dx + dy * dy), axis=0)      # fmin skips a NaN; all NaN stays NaN and compares false
        near = key < 2 * radius
    np.fill_diagonal(near, False)
    ids_np = np.array(ids)                                            # neighbours as NumPy integers, as define_inter_graph_threshold's (Q10)
    graph = {}
    for i, id_ in enumerate(ids):
        cand = np.nonzero(near[i])[0]
        if cand.size + 1 > m:
            cand = cand[np.lexsort((cand, key[i, cand]))][:m - 1]
        graph[id_] = sorted([id_] + [ids_np[j] for j in cand])
    return graph


def solve_distributed(problem, X, U, radius, ignore_ids=None, pool=None, verbose=True, max_cluster=None, **kwargs):
    """One sub-problem per agent (its closed neighbourhood), all solved in one batched dispatch.

    Returns X_dec (N+1, n_x), U_dec (N, n_u), J_full, solve_info {id: (seconds, neighbourhood)}.
    `pool` is accepted for signature compatibility; the device batch takes its place.  `ignore_ids=None`
    means "ignore nobody" (the reference raises TypeError there, quirk Q9).  Teams of up to 256 agents are served (J_full of
    more than 64 agents through ProblemBatch.rollout_wide); every neighbourhood must lie within the solver's own limits.
    max_cluster=m (an integer 1 .. 64; None: no cap): every agent plans with itself and at most the m - 1 nearest of its
    neighbours -- the graph is nearest_neighbourhoods(X, radius, x_dims, ids, m); solve_rhc passes it on as it passes radius."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64)); U = np.asarray(U, dtype=np.float64)
    x_dims, u_dims = problem.game_cost.x_dims, problem.game_cost.u_dims
    N, n_s, n_c, ids = U.shape[0], x_dims[0], u_dims[0], problem.ids
    ignore_ids = list(ignore_ids) if ignore_ids else []
    if any(id_ not in ids for id_ in ignore_ids):
        raise ValueError(f"Some of {ignore_ids} not in {ids}.")
    if max_cluster is None:
        graph = define_inter_graph_threshold(X, radius, x_dims, ids)
    else:
        graph = nearest_neighbourhoods(X, radius, x_dims, ids, max_cluster)
    if verbose:
        print("=" * 80 + f"\nInteraction Graph: {graph}")
    x0_split = split_graph(X[np.newaxis, 0], x_dims, graph)
    U_split = split_graph(U, u_dims, graph)
    subproblems = problem.split(graph)
    todo = [i for i, id_ in enumerate(ids) if id_ not in ignore_ids]
    t0 = pc()
    res = solve_problem_list([subproblems[i] for i in todo], [x0_split[i] for i in todo], [U_split[i] for i in todo],
                             keys=[tuple(graph[ids[i]]) for i in todo], **kwargs)
    dt_each = (pc() - t0) / max(len(todo), 1)
    X_dec = np.zeros((N + 1, len(ids) * n_s)); U_dec = np.zeros((N, len(ids) * n_c))
    solve_info = {}
    for i, (Xi, Ui, _, _) in zip(todo, res):
        Xa, Ua = subproblems[i].extract(Xi, Ui, ids[i])
        X_dec[:, i * n_s:(i + 1) * n_s] = Xa
        U_dec[:, i * n_c:(i + 1) * n_c] = Ua
        solve_info[ids[i]] = (dt_each, graph[ids[i]])
    for id_ in ignore_ids:
        solve_info[id_] = (0.0, [id_])
    _, J_full = ilqrSolver(problem, N)._rollout(X[0], U_dec)
    return X_dec, U_dec, J_full, solve_info


def closed_loop_distributed(problem, X, U, radius, x0s, W=None, u_lim=None, mu=0.0, trajectories=False, wide=False, max_cluster=None,
                            **solve_kwargs):
    """The closed loop of solve_distributed's solution for one scenario: solve the sub-problems from (X, U) as
    solve_scenarios_distributed does, take every sub-problem's gains from one backward pass at its solution (regularisation
    mu, as ilqrSolver.closed_loop), and run the agents' own feedback laws -- each over its neighbourhood only -- on the full
    problem from the starts x0s (n_samples, n_x).  W (n_samples, N, n_x): additive disturbance; u_lim (2, n_u): control limits.
    Returns host arrays: J, min_sep (n_samples,), goal_dist (n_samples, k), X_dec, U_dec of the solve and, with
    trajectories=True, X (n_samples, N+1, n_x), U (n_samples, N, n_u).  Device problems only.
    wide=True: solve_scenarios_distributed(policy="wide") -- any team of up to 256 agents, multi-word neighbourhood masks,
    ProblemBatch.policy_rollout_dec_wide; the default serves teams of up to 64 agents as ever.
    max_cluster=m (an integer 1 .. 64; None: no cap): solve_scenarios_distributed(max_cluster=m) -- every agent plans, and feeds
    back, over itself and at most the m - 1 nearest of its neighbours."""
    from .lowering import is_lowerable
    if not is_lowerable(problem):
        raise NotImplementedError("closed_loop_distributed runs the policy on the device and needs a problem built from the "
                                  "recognised plugin types: this one contains host plugins, whose dynamics and cost only exist as "
                                  "Python callables")
    X = np.atleast_2d(np.asarray(X, dtype=np.float64)); U = np.asarray(U, dtype=np.float64)
    n_x = problem.dynamics.n_x
    if max_cluster is not None:
        from .dispatch import checked_max_cluster
        checked_max_cluster(max_cluster, problem.n_agents)
    x0s = np.asarray(x0s, dtype=np.float64)
    if x0s.ndim != 2 or x0s.shape[1] != n_x:
        raise ValueError(f"closed_loop_distributed: x0s has shape {x0s.shape}, expected (n_samples, {n_x})")
    if U.ndim != 2 or X.shape[1] != n_x or X.shape[0] not in (1, U.shape[0] + 1):
        raise ValueError(f"closed_loop_distributed: X {X.shape}, U {U.shape}: expected (N+1 or 1, {n_x}) and (N, n_u)")
    X_dec, U_dec, _, info = solve_scenarios_distributed(problem, X[None], U[None], radius, device_out=True, policy="wide" if wide else True,
                                                        policy_mu=float(mu), max_cluster=max_cluster, **solve_kwargs)
    r = info["policy"].rollout(x0s[None], W=None if W is None else np.asarray(W, dtype=np.float64)[None], u_lim=u_lim,
                               trajectories=trajectories)
    out = {key: v[0].cpu().numpy() for key, v in r.items()}
    out["X_dec"], out["U_dec"] = X_dec[0].cpu().numpy(), U_dec[0].cpu().numpy()
    return out


def solve_centralized(solver, xi, U, ids, verbose, **kwargs):
    t0 = pc()
    X, U, J = solver.solve(xi, U, verbose=verbose, **kwargs)
    dt = pc() - t0
    return X, U, J, {id_: (dt, ids) for id_ in ids}


def rhc_log_row(model_name, n_agents, i_trial, centralized, last, t, J, N, dt, converged, ids, times, subgraphs, left):
    """One CSV row of solve_rhc's log, in the format of distributed.py:190-194 / :215-219 (header: analysis.py:120-123):
    dynamics,n_agents,trial,centralized,last,t,J,horizon,dt,converged,ids,times,subgraphs,dist_left."""
    return (f'"{model_name}",{n_agents},{i_trial},{centralized},{last},{t},{J},{N},{dt},{converged},"{ids}",'
            f'"{times}","{subgraphs}","{left}"')


def rhc_subgraphs(bits, ids):
    """The `subgraphs` field of a round's CSV row from the round's neighbourhood masks: bits (k,) one 64-bit word per agent, or
    (k, n_words) -- member q is bit q % 64 of word q // 64 (a word may come as a signed integer: bit 63 is its sign).  Per agent
    the sorted ids of its neighbourhood, its own id as a Python int and its neighbours as NumPy ints (quirk Q10), so that the
    list prints as solve_distributed's graph prints inside solve_rhc's rows."""
    bits = np.asarray(bits)
    k = len(ids)
    words = bits.reshape(k, -1)
    out = []
    for i in range(k):
        w = [int(v) for v in words[i]]
        out.append(sorted([ids[i]] + [np.int64(ids[q]) for q in range(k) if q != i and (w[q >> 6] >> (q & 63)) & 1]))
    return out


def solve_rhc(problem, x0, N, *args, centralized=True, n_d=2, step_size=1, J_converge=None, dist_converge=None,
              t_diverge=None, i_trial=None, verbose=False, **kwargs):
    """Receding-horizon loop around solve_centralized / solve_distributed (distributed.py:106-221); logs the
    same CSV rows through `logging.info`.  The warm start is drawn from NumPy's global RNG as in the reference."""
    if (J_converge is None) == (dist_converge is None):
        raise ValueError("Must either specify a convergence cost or distance")
    xf = problem.game_cost.xf
    n_states, n_agents = problem.dynamics.x_dims[0], problem.n_agents
    n_x, n_u = problem.dynamics.n_x, problem.dynamics.n_u

    def distance_to_goal(x):
        return np.linalg.norm((x - xf).reshape(n_agents, n_states)[:, :n_d], axis=1)

    if J_converge:
        keep_going = lambda x, J: J >= J_converge
    else:
        keep_going = lambda x, J: bool(np.any(distance_to_goal(x) > dist_converge))
    model_name = type(problem.dynamics.submodels[0]).__name__
    xi = np.asarray(x0, dtype=np.float64).reshape(1, -1)
    X = xi.copy()
    U = np.random.rand(N, n_u) * 0.01
    solver = ilqrSolver(problem, N)
    t, J, converged, dt, ids = 0, np.inf, True, problem.dynamics.dt, list(problem.ids)
    X_full = np.zeros((0, n_x)); U_full = np.zeros((0, n_u))
    times, subgraphs, left = [], [], distance_to_goal(xi.ravel()).tolist()
    while keep_going(xi.ravel(), J):
        if centralized:
            X, U, J, info = solve_centralized(solver, xi, U, ids, False, **kwargs)
        else:
            X, U, J, info = solve_distributed(problem, X, U, *args, verbose=False, **kwargs)
        xi = X[step_size]
        X_full = np.r_[X_full, X[:step_size]]; U_full = np.r_[U_full, U[:step_size]]
        X = np.r_[X[step_size:], np.tile(X[-1], (step_size, 1))]     # stay at the last visited state
        U = np.r_[U[step_size:], np.zeros((step_size, n_u))]
        times = [v[0] for v in info.values()]; subgraphs = [v[1] for v in info.values()]
        left = distance_to_goal(xi).tolist()
        logging.info(rhc_log_row(model_name, n_agents, i_trial, centralized, False, t, J, N, dt, converged, ids, times,
                                 subgraphs, left))
        if t_diverge and t >= t_diverge:
            converged = False
            break
        t += step_size * dt
    if not X_full.size and not U_full.size:
        X_full = np.asarray(x0, dtype=np.float64).copy(); U_full = np.zeros((1, n_u))
    _, J_full = ilqrSolver(problem, U_full.shape[0])._rollout(np.asarray(x0, dtype=np.float64), U_full)
    logging.info(rhc_log_row(model_name, n_agents, i_trial, centralized, True, U_full.shape[0] * dt, J_full, N, dt, converged,
                             ids, times, subgraphs, left))
    return X_full, U_full, J_full


def solve_rhc_scenarios(problem, x0, N, radius, xf=None, U0=None, centralized=False, n_d=2, step_size=1,
                        J_converge=None, dist_converge=None, t_diverge=None, window=None, i_trial=None, rows=None, max_cluster=None,
                        wide=False, **kwargs):
    """solve_rhc (distributed.py:106-221) for S Monte-Carlo scenarios of one k-agent problem in lock step: every
    receding-horizon round is ONE batched solve over the scenarios still running (solve_scenarios_distributed, or one
    ProblemBatch when centralized), with the reference's warm-start shift and stopping rules applied per scenario.
    The state of the loop -- current states, shifted warm starts (:184-185), executed prefixes -- stays on the device
    between rounds; per round only the S stopping flags come to the host.

    x0 (S, n_x); xf (S, n_x) goals (default: the problem's own); U0 (S, N, n_u) warm starts (default: drawn per
    scenario, in order, as solve_rhc draws them: np.random.rand(N, n_u) * 0.01).
    rows: a list to fill with S lists of CSV rows -- for every scenario exactly the rows solve_rhc logs for it
    (distributed.py:190-194,215-219: one per receding-horizon round and the closing one), in its format (rhc_log_row);
    i_trial: their trial numbers (a sequence of S, or one value).  The `times` field is wall-clock there and here: each
    agent is given its share of the round's batched solve.  kwargs: n_lqr_iter, tol, t_kill reach every solve.
    Without wide=True a team of more than 64 agents (centralized or not) is a ValueError before any device work.
    max_cluster=m (an integer 1 .. 64; None: no cap; the distributed branch): every round's solve_scenarios_distributed caps the
    neighbourhoods at their m nearest agents, and the rows' `subgraphs` field shows the capped neighbourhoods.
    wide=True serves the DISTRIBUTED loop (centralized=False) of any lowerable team of 1 .. 256 agents: every round is
    solve_scenarios_distributed on the wide front end (multi-word masks, max_cluster honoured), the warm-start shift, the stopping
    rules, t_diverge, the rows and the returned tuples are the ones above, and the rows' `subgraphs` field is decoded from the
    multi-word masks (rhc_subgraphs).  J_full of a team of more than 64 agents is one ProblemBatch.rollout_wide per executed
    length; a smaller team keeps ProblemBatch.rollout, so that at k <= 64 wide=True returns the default route's arrays and rows
    (the wall-clock `times` field apart).  x0, xf and U0 may be device tensors (they are not modified).  It is opt-in; with
    centralized=True, ignore_ids or shard=, more than 256 agents, or more than 12 agents of the five-state family it is a
    ValueError before any device work.  Not built: fp32, shard=, ignore_ids; the wide route as a default; a centralized branch
    for such teams.
    Returns a list of S tuples (X_full, U_full, J_full, converged), what solve_rhc returns plus its `converged` flag."""
    import torch
    from .batch import ProblemBatch
    from .device import to_dev
    from .dispatch import device_constants, solve_scenarios_distributed
    from .lowering import describe
    if (J_converge is None) == (dist_converge is None):
        raise ValueError("Must either specify a convergence cost or distance")
    from . import _lib
    if wide:      # refused before the problem is even described: nothing here touches the device
        from .batch import ROUTES
        k_w = problem.n_agents
        if centralized:
            raise ValueError("solve_rhc_scenarios: wide=True is the distributed loop (centralized=False) of a team of up to "
                             f"{_lib.MAX_TEAM} agents; no centralized solve is built for such teams")
        if kwargs.get("ignore_ids") or kwargs.get("shard") is not None:
            raise ValueError("solve_rhc_scenarios: wide=True serves neither shard= nor ignore_ids")
        if k_w > _lib.MAX_TEAM:
            raise ValueError(f"solve_rhc_scenarios: wide=True serves teams of up to {_lib.MAX_TEAM} agents (this one has {k_w})")
        if problem.dynamics.n_x // k_w == 5 and k_w > ROUTES["team"]["max_k_of_ns"][5]:
            raise ValueError(f"solve_rhc_scenarios: wide=True serves the five-state family up to 12 agents, this one has k = {k_w}")
    d = describe(problem)
    k, dt = d["k"], d["dt"]
    if k > _lib.MAX_AGENTS and not wide:
        raise ValueError(f"solve_rhc_scenarios is not built for teams of more than {_lib.MAX_AGENTS} agents (this one has {k}): "
                         "solve_scenarios_distributed and solve_distributed serve them, round by round")
    if max_cluster is not None:
        from .dispatch import checked_max_cluster
        checked_max_cluster(max_cluster, k)
        if centralized:
            raise ValueError("solve_rhc_scenarios: max_cluster caps the neighbourhoods of the distributed solve (centralized=False)")
    n_x, n_u = problem.dynamics.n_x, problem.dynamics.n_u
    n_s = n_x // k
    on_device = lambda a: isinstance(a, torch.Tensor)      # inputs given as device tensors stay there (and stay the caller's)
    x0 = to_dev(x0).reshape(-1, n_x) if on_device(x0) else np.asarray(x0, dtype=np.float64).reshape(-1, n_x)
    S = x0.shape[0]
    if xf is None:
        xf_h = np.broadcast_to(d["xf"], (S, n_x)).copy()
    else:
        xf_h = to_dev(xf).reshape(S, n_x) if on_device(xf) else np.asarray(xf, dtype=np.float64).reshape(S, n_x)
    if U0 is None:
        U_h = np.stack([np.random.rand(N, n_u) * 0.01 for _ in range(S)])
    else:
        U_h = to_dev(U0).clone() if on_device(U0) else np.array(U0, dtype=np.float64)
    solve_kw = solve_kwargs(kwargs, "solve_rhc_scenarios")
    xf_d, U, xi = to_dev(xf_h), to_dev(U_h), to_dev(x0).clone()
    X = None                                       # first round: the graph is built from x0 alone (distributed.py:152)
    J = torch.full((S,), float("inf"), dtype=torch.float64, device=xi.device)
    t = [0] * S                                    # the reference's t: the int 0 until the first `t += step_size * dt`
    converged = np.ones(S, dtype=bool)
    X_parts = [[] for _ in range(S)]; U_parts = [[] for _ in range(S)]
    want_rows = rows is not None
    ids = list(problem.ids)
    model_name = type(problem.dynamics.submodels[0]).__name__
    trial_of = list(i_trial) if isinstance(i_trial, (list, tuple, np.ndarray)) else [i_trial] * S
    row_log = [[] for _ in range(S)]
    last_fields = [([], [], None) for _ in range(S)]       # (times, subgraphs, distance left) of a scenario's last round

    def distance_left(idx):
        return torch.linalg.vector_norm((xi[idx] - xf_d[idx]).reshape(len(idx), k, n_s)[:, :, :n_d], dim=2)

    if want_rows:                                  # what solve_rhc holds before any round (a loop that never runs)
        left0 = distance_left(torch.arange(S, device=xi.device)).cpu().numpy()
        last_fields = [([], [], left0[s].tolist()) for s in range(S)]

    def keep_going(idx):      # one small device -> host read per round: the stopping flags
        if J_converge:
            return (J[idx] >= J_converge).cpu().numpy()
        return (distance_left(idx) > dist_converge).any(dim=1).cpu().numpy()

    active = np.nonzero(keep_going(torch.arange(S, device=xi.device)))[0]
    while active.size:
        ia = torch.as_tensor(active, device=xi.device)
        t_round = pc()
        bits = None
        if centralized:
            c = device_constants(d)
            pb = ProblemBatch(c["model"], c["n_dims"], xf_d[ia], c["Q"], c["R"], c["Qf"], d["radius"], dt, N,
                              w_ref=d["w_ref"], w_prox=d["w_prox"], B=len(active), hints=(k, n_s, n_u // k, c["word"]))
            r = pb.solve(xi[ia], U[ia], window=window, **solve_kw)
            Xa, Ua, Ja = r["X"], r["U"], r["J"]
        else:
            Xin = xi[ia][:, None, :] if X is None else X[ia]
            Xa, Ua, Ja, info = solve_scenarios_distributed(problem, Xin, U[ia], radius, xf=xf_d[ia], window=window, device_out=True,
                                                           desc=d, max_cluster=max_cluster, **({"wide": True} if wide else {}),
                                                           **solve_kw)
            bits = info["cluster_bits"]
        if X is None:
            X = torch.zeros((S, N + 1, n_x), dtype=torch.float64, device=xi.device)
        # what the round contributes to the executed trajectory: ONE (|active|, step_size, .) copy per round.  (Views into
        # Xa / Ua here kept every round's whole (|active|, N + 1, n_x) result alive on the device until the end.)
        Xkeep, Ukeep = Xa[:, :step_size].clone(), Ua[:, :step_size].clone()
        for j, s in enumerate(active):
            X_parts[s].append(Xkeep[j]); U_parts[s].append(Ukeep[j])
        xi[ia] = Xa[:, step_size]
        # warm start of the next round: shift, stay at the last visited state, zero controls (distributed.py:184-185)
        X[ia] = torch.cat([Xa[:, step_size:], Xa[:, -1:].expand(-1, step_size, -1)], dim=1)
        U[ia] = torch.cat([Ua[:, step_size:], torch.zeros((len(active), step_size, n_u), dtype=torch.float64, device=xi.device)], dim=1)
        J[ia] = Ja
        if want_rows:
            share = (pc() - t_round) / (len(active) * k)
            J_h, left_h = Ja.cpu().numpy(), distance_left(ia).cpu().numpy()
            for j, s in enumerate(active):
                if centralized:
                    subgraphs = [ids] * k                                    # solve_centralized: {id: (dt, ids)}
                else:
                    subgraphs = rhc_subgraphs(bits[j], ids)
                last_fields[s] = ([share] * k, subgraphs, left_h[j].tolist())
                row_log[s].append(rhc_log_row(model_name, k, trial_of[s], centralized, False, t[s], float(J_h[j]), N, dt,
                                              bool(converged[s]), ids, *last_fields[s]))
        diverged = np.zeros(len(active), dtype=bool)
        if t_diverge:
            diverged = np.array([t[s] >= t_diverge for s in active])
            converged[active[diverged]] = False
        for s in active[~diverged]:
            t[s] += step_size * dt
        still = keep_going(ia) & ~diverged
        active = active[still]
    # the executed trajectories, and J_full = the cost of rolling the executed controls out from x0 (distributed.py:208): one
    # batched rollout per executed length instead of one launch per scenario
    XU = []
    for s in range(S):
        if X_parts[s]:
            XU.append((torch.cat(X_parts[s]).cpu().numpy(), torch.cat(U_parts[s]).cpu().numpy()))
        else:
            XU.append((x0[s].cpu().numpy() if on_device(x0) else x0[s].copy(), np.zeros((1, n_u))))
    J_full = np.zeros(S)
    by_len = {}
    for s in range(S):
        by_len.setdefault(XU[s][1].shape[0], []).append(s)
    for L_exec, idx in by_len.items():
        pbl = ProblemBatch(d["model"], d["n_dims"], xf_h[idx], d["Q"], d["R"], d["Qf"], d["radius"], dt, L_exec,
                           w_ref=d["w_ref"], w_prox=d["w_prox"], B=len(idx))
        if k > _lib.MAX_AGENTS:      # the full-team rollout of the wide entries (as solve_scenarios_distributed's own J_full)
            Jl = pbl.rollout_wide(x0[idx], np.stack([XU[s][1] for s in idx]), trajectories=False)["J"]
        else:
            _, Jl = pbl.rollout(x0[idx], np.stack([XU[s][1] for s in idx]))
        J_full[idx] = Jl.cpu().numpy()
    out = []
    for s in range(S):
        Xf, Uf = XU[s]
        out.append((Xf, Uf, float(J_full[s]), bool(converged[s])))
        if want_rows:
            row_log[s].append(rhc_log_row(model_name, k, trial_of[s], centralized, True, Uf.shape[0] * dt, out[-1][2], N, dt,
                                          bool(converged[s]), ids, *last_fields[s]))
    if want_rows:
        rows.extend(row_log)
    return out


def solve_rhc_closed_loop(problem, x0, N, radius=None, xf=None, U0=None, centralized=True, feedback=True, W=None, u_lim=None,
                          policy_mu=0.0, n_d=2, step_size=1, dist_converge=None, J_converge=None, max_steps=None, window=None,
                          large=False, team=False, wide=False, max_cluster=None, **kwargs):
    """The receding-horizon loop on a REAL plant, for S scenarios in lock step: plan, execute step_size steps of the plan's
    feedback policy under a disturbance and actuator limits, re-plan from where the plant ended up.  solve_rhc and
    solve_rhc_scenarios keep the reference's ideal plant (xi = X[step_size]); here every round is one batched solve over the
    scenarios still running -- ProblemBatch.solve and, with feedback, one backward_pass(X, U, policy_mu) at the solution when
    centralized, solve_scenarios_distributed(policy=feedback, policy_mu=...) otherwise -- followed by ONE launch of
    ProblemBatch.policy_advance / policy_advance_dec, which executes u = U[t] + K[t] (x - X[t]) (feedback=False: u = U[t])
    from every scenario's plant state, appends to the executed trajectories and shifts the warm start (distributed.py:184-185
    with the plant's state in front).  Only the stopping flags come to the host each round, by solve_rhc's rules: the planned
    J >= J_converge, or any agent further than dist_converge from its goal over n_d coordinates.

    x0 (S, n_x); xf (S, n_x) goals (default: the problem's own); U0 (S, N, n_u) warm starts (default: drawn as solve_rhc draws
    them); W (S, L, n_x) additive disturbance on the plant, read at a scenario's own executed step; u_lim (2, n_u) control
    limits; radius: the graph threshold of the distributed solve.  The capacity L = max_steps (default: W's length) bounds the
    executed steps as t_diverge bounds solve_rhc: a scenario that reaches it without meeting its criterion has converged =
    False.  kwargs: n_lqr_iter, tol, t_kill reach every solve.
    Returns a dict: X, U -- lists of S host arrays (n_s + 1, n_x), (n_s, n_u) of the executed lengths --, J (S,) the realised
    cost (stage costs of the executed points plus the terminal cost of the final state), min_sep (S,), goal_dist (S, k),
    converged (S,), n_rounds (S,).
    large=True serves a centralized problem of 60 < n_x <= 240 states and k <= 20 agents (the four-, six- and twelve-state
    families): every round is ProblemBatch.solve, backward_pass(X, U, policy_mu) with feedback, and one launch of
    ProblemBatch.policy_advance_large, whose K dx is policy_rollout_large's (one fused multiply-add per term).  A problem of
    n_x <= 60 takes the route above whatever `large` says.
    team=True serves the DISTRIBUTED loop (centralized=False) of any lowerable team of up to 64 agents, whatever n_x is (64
    double integrators: n_x = 256): every round is solve_scenarios_distributed(policy=feedback, ...) and one launch of
    ProblemBatch.policy_advance_dec_team -- DistributedPolicy.advance(..., team=True) with feedback, the stitched plan open loop
    without --, whose arithmetic is policy_rollout_dec_team's.  A problem of n_x <= 60 and k <= 20 takes the route above
    whatever `team` says.  It is opt-in: without it a larger distributed problem is refused as before.
    wide=True serves the DISTRIBUTED loop (centralized=False) of any lowerable team of 1 .. 256 agents on the wide entries,
    whatever its size: every round is solve_scenarios_distributed(policy="wide" if feedback else False, ...) and one launch of
    ProblemBatch.policy_advance_dec_wide -- DistributedPolicy.advance(..., wide=True) with feedback, the stitched plan open loop
    without --, and the final state's terminal cost is ProblemBatch.cost_wide.  It is opt-in too: without it every refusal is
    as before, a team of more than 64 agents included.
    max_cluster=m (an integer 1 .. 64; None: no cap) serves every distributed route -- the small one, team=True, wide=True --:
    each round's solve_scenarios_distributed caps the neighbourhoods at their m nearest agents (include/dpilqr_nearest.h), the
    policy's masks are the capped ones and the advance reads them as any others; a dense team (a clique of 64, a swarm whose
    neighbourhoods exceed 64 agents) is planned round by round instead of refused.  With centralized=True it is a ValueError.
    Not built: fp32, shard=, ignore_ids; the wide route as a default.  Device problems only."""
    import torch
    from . import _lib
    from .batch import ROUTES, ProblemBatch, route_refusal, route_serves
    from .device import to_dev
    from .dispatch import device_constants
    from .lowering import describe, is_lowerable
    if not is_lowerable(problem):
        raise NotImplementedError("solve_rhc_closed_loop runs the plant on the device and needs a problem built from the recognised "
                                  "plugin types: this one contains host plugins, whose dynamics and cost only exist as Python "
                                  "callables")
    if (J_converge is None) == (dist_converge is None):
        raise ValueError("Must either specify a convergence cost or distance")
    n_x, n_u = problem.dynamics.n_x, problem.dynamics.n_u
    k = problem.n_agents      # (lowerable: one cost and one (n_s, n_c) per agent)
    n_s, n_c = n_x // k, n_u // k
    if max_cluster is not None:
        from .dispatch import checked_max_cluster
        checked_max_cluster(max_cluster, k)
        if centralized:
            raise ValueError("solve_rhc_closed_loop: max_cluster caps the neighbourhoods of the distributed loop (centralized=False)")
    if wide:      # the wide entries, whatever the size: none of the routes below
        if centralized:
            raise ValueError("solve_rhc_closed_loop: wide=True is the distributed loop (centralized=False) of a team of up to "
                             f"{_lib.MAX_TEAM} agents")
        if k > _lib.MAX_TEAM:
            raise ValueError(f"solve_rhc_closed_loop: wide=True serves teams of up to {_lib.MAX_TEAM} agents (this one has {k})")
        if n_s == 5 and k > ROUTES["team"]["max_k_of_ns"][5]:
            raise ValueError(f"solve_rhc_closed_loop: wide=True serves the five-state family up to 12 agents, this one has k = {k}")
        if kwargs.get("ignore_ids") or kwargs.get("shard") is not None:
            raise ValueError("solve_rhc_closed_loop: wide=True serves neither shard= nor ignore_ids")
    small = not wide and route_serves("small", k, n_s, n_c)      # the routes and their limits: batch.ROUTES
    large = bool(large) and not small and not wide
    if team and centralized:
        raise ValueError("solve_rhc_closed_loop: team=True is the distributed loop (centralized=False); a centralized problem of "
                         "60 < n_x <= 240 is served by large=True")
    team = bool(team) and not large and not small and not wide
    if not (small or large or team or wide):
        raise ValueError(f"solve_rhc_closed_loop serves problems up to n_x = 60, this one has n_x = {n_x} "
                         "(large=True serves a centralized problem of up to n_x = 240, team=True the distributed loop of a team "
                         "of up to 64 agents)")
    if large and not centralized:
        raise ValueError("solve_rhc_closed_loop: large=True serves the centralized loop only, the distributed loop for problems of "
                         f"more than 60 states is not built (this one has n_x = {n_x})")
    if large and n_x > ROUTES["large"]["max_nx"]:
        raise ValueError(f"solve_rhc_closed_loop: large=True serves problems of 60 < n_x <= 240, this one has n_x = {n_x}")
    if not centralized and radius is None:
        raise ValueError("solve_rhc_closed_loop: the distributed solve needs the graph's radius")
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, n_x)
    S = x0.shape[0]
    if W is not None:
        W = np.asarray(W, dtype=np.float64) if not isinstance(W, torch.Tensor) else W
        if W.ndim != 3 or W.shape[0] != S or W.shape[2] != n_x:
            raise ValueError(f"solve_rhc_closed_loop: W has shape {tuple(W.shape)}, expected ({S}, L, {n_x})")
    L = int(max_steps) if max_steps is not None else (int(W.shape[1]) if W is not None else None)
    if L is None:
        raise ValueError("solve_rhc_closed_loop: max_steps (or a disturbance W, whose length it defaults to) bounds the executed steps")
    if L < 1 or (W is not None and W.shape[1] != L):
        raise ValueError(f"solve_rhc_closed_loop: max_steps = {L} with W of shape {None if W is None else tuple(W.shape)}")
    h = int(step_size)
    if not 1 <= h <= N:
        raise ValueError(f"solve_rhc_closed_loop: step_size = {step_size}, a round executes 1 .. N = {N} steps")
    d = describe(problem)
    dt = d["dt"]
    why = route_refusal("team", k, n_s, n_c) if team else None
    if why == "beyond":
        raise ValueError(f"solve_rhc_closed_loop is not built for teams of more than {ROUTES['team']['max_k']} agents (this one has {k})")
    if why == "family":
        raise ValueError(f"solve_rhc_closed_loop: team=True serves the five-state family up to 12 agents, this one has k = {k}")
    if large and not route_serves("large", k, n_s, n_c):      # (n_x lies within the route's bounds: refused above otherwise)
        raise ValueError(f"solve_rhc_closed_loop: large=True serves teams of k <= 20 agents of the four-, six- and twelve-state "
                         f"families, this one has k = {k}, (n_s, n_c) = ({n_s}, {n_c})")
    if not 1 <= n_d <= n_s:
        raise ValueError(f"solve_rhc_closed_loop: n_d = {n_d}, an agent has {n_s} states")
    solve_kw = solve_kwargs(kwargs, "solve_rhc_closed_loop")
    xf_h = np.broadcast_to(d["xf"], (S, n_x)).copy() if xf is None else np.asarray(xf, dtype=np.float64).reshape(S, n_x)
    U_h = np.stack([np.random.rand(N, n_u) * 0.01 for _ in range(S)]) if U0 is None else np.array(U0, dtype=np.float64).reshape(S, N, n_u)
    xf_d = to_dev(xf_h)
    c = device_constants(d)

    def batch(idx):
        return ProblemBatch(c["model"], c["n_dims"], xf_d if idx is None else xf_d[idx], c["Q"], c["R"], c["Qf"], d["radius"], dt, N,
                            w_ref=d["w_ref"], w_prox=d["w_prox"], B=S if idx is None else len(idx), hints=(k, n_s, n_u // k, c["word"]))

    full = batch(None)
    state = full.advance_state(x0, L)
    state["U_next"].copy_(to_dev(U_h))
    W_d = None if W is None else to_dev(W)
    lim_d = None if u_lim is None else to_dev(np.asarray(u_lim, dtype=np.float64) if not isinstance(u_lim, torch.Tensor) else u_lim)
    dev = xf_d.device
    state["dist_left"].copy_(torch.linalg.vector_norm((state["x_cur"] - xf_d).reshape(S, k, n_s)[:, :, :n_d], dim=2))
    J = torch.full((S,), float("inf"), dtype=torch.float64, device=dev)

    def flags(idx):      # one small device -> host read per round: (keeps going, has room) per scenario
        crit = (J[idx] >= J_converge) if J_converge else (state["dist_left"][idx] > dist_converge).any(dim=1)
        return torch.stack([crit, state["n_done"][idx] < L]).cpu().numpy()

    converged = np.ones(S, dtype=bool)
    n_rounds = np.zeros(S, dtype=np.int64)
    go, room = flags(torch.arange(S, device=dev))
    active = np.nonzero(go & room)[0]
    first = True
    while active.size:
        ia = torch.as_tensor(active, device=dev)
        scen = ia.to(torch.int32)
        if centralized:
            pb = batch(ia)
            r = pb.solve(state["x_cur"][ia], state["U_next"][ia], window=window, **solve_kw)
            K = pb.backward_pass(r["X"], r["U"], float(policy_mu))[0] if feedback else None
            advance = pb.policy_advance_large if large else pb.policy_advance
            advance(r["X"], r["U"], K, h, state, scen=scen, W=W_d, u_lim=lim_d, n_d=n_d)
            J[ia] = r["J"]
        else:
            Xin = state["x_cur"][ia][:, None, :] if first else state["X_next"][ia]
            Xa, Ua, Ja, info = solve_scenarios_distributed(problem, Xin, state["U_next"][ia], radius, xf=xf_d[ia], window=window,
                                                           device_out=True, desc=d, policy_mu=float(policy_mu),
                                                           policy="wide" if wide and feedback else bool(feedback),
                                                           max_cluster=max_cluster, **solve_kw)
            if feedback:
                info["policy"].advance(h, state, scen=scen, W=W_d, u_lim=lim_d, n_d=n_d, team=team, wide=wide)
            else:
                pb = batch(ia)
                advance = pb.policy_advance_dec_wide if wide else pb.policy_advance_dec_team if team else pb.policy_advance_dec
                advance(Xa, Ua, None, None, h, state, scen=scen, W=W_d, u_lim=lim_d, n_d=n_d)
            J[ia] = Ja
        first = False
        n_rounds[active] += 1
        go, room = flags(ia)
        converged[active[go & ~room]] = False
        active = active[go & room]
    n_done = state["n_done"].cpu().numpy()
    X_exec, U_exec = state["X_exec"].cpu().numpy(), state["U_exec"].cpu().numpy()
    J_term = (full.cost_wide if wide else full.cost)(state["x_cur"][:, None, :], torch.zeros((S, 1, n_u), dtype=torch.float64, device=dev), terminal=True)[:, 0]
    return dict(X=[X_exec[s, :n_done[s] + 1].copy() for s in range(S)], U=[U_exec[s, :n_done[s]].copy() for s in range(S)],
                J=(state["J_exec"] + J_term).cpu().numpy(), min_sep=state["min_sep"].cpu().numpy(),
                goal_dist=state["dist_left"].cpu().numpy(), converged=converged, n_rounds=n_rounds)
