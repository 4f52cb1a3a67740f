"""The scenarios of the swarm-study tests, shared by tests/test_swarm_study_host.py (which checks their conditions on the first-round
graph in NumPy, without a GPU) and tests/test_gpu_swarm_study.py (which runs them).  Not a test module."""
import numpy as np

RADIUS, DT, STEP_SIZE = 0.5, 0.1, 3
# solve_rhc breaks out after the round in which t >= t_diverge, t = 0, 0.3, 0.6, 0.9 (to rounding): four rounds / two rounds at most
T_DIVERGE_FOUR_ROUNDS, T_DIVERGE_TWO_ROUNDS = 0.85, 0.25
# the loop on a swarm: 65 double integrators, three trials.  SPARSE: every first-round neighbourhood has 1 .. 8 members and at least
# one has two; DENSE: some neighbourhood exceeds the cap of 4, which then bites
LOOP = dict(k=65, N=8, trials=(0, 1, 2), energy_sparse=300.0, energy_dense=150.0, max_cluster=4)
# a two-word mask in the study: 130 double integrators, two trials, capped at 4 (which bites)
STUDY = dict(k=130, N=6, trials=(0, 1), energy=600.0, max_cluster=4)


def model():
    from dpilqr_amd import analysis
    return analysis.DoubleIntDynamics4D


def inputs(k, N, energy, trials):
    """trial_inputs of the study's own seeds: lists of x0, xf (n_x,), U_c, U_d (N, n_u)."""
    from dpilqr_amd import analysis
    drawn = [analysis.trial_inputs(k, 4, 2 * k, N, energy, 2, analysis.seed_of(model(), k, i)) for i in trials]
    return [d[0].ravel() for d in drawn], [d[1].ravel() for d in drawn], [d[2] for d in drawn], [d[3] for d in drawn]


def first_round_sizes(k, N, energy, trials, max_cluster=None):
    """Per trial: the sizes of the first round's neighbourhoods (the graph of x0 alone), uncapped and -- with max_cluster --
    capped."""
    from dpilqr_amd.distributed import define_inter_graph_threshold, nearest_neighbourhoods
    ids = [100 + i for i in range(k)]
    out = []
    for x0 in inputs(k, N, energy, trials)[0]:
        g = define_inter_graph_threshold(x0.reshape(1, -1), RADIUS, [4] * k, ids)
        free = np.array([len(g[i]) for i in ids])
        capped = None
        if max_cluster is not None:
            c = nearest_neighbourhoods(x0.reshape(1, -1), RADIUS, [4] * k, ids, max_cluster)
            capped = np.array([len(c[i]) for i in ids])
        out.append((free, capped))
    return out
