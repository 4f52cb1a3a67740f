"""GPU tests of the reference-style surface: the same objects and calls a dp-ilqr user writes
(ilqrProblem / ilqrSolver / solve_distributed / plugin methods), checked against the golden vectors."""
import numpy as np
import pytest

from tests.golden_util import MODEL_NAMES, relerr
from tests.test_host_logic import MODEL_CLASSES, problem_from

pytestmark = pytest.mark.gpu
TOL_PASS, TOL_SOLVE = 1e-9, 1e-5


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()
    return dpilqr_amd


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_plugin_models(dp, golden, name):
    """Model(dt)(x,u), .f, .linearize and the module-level FFI functions vs bbdynamicswrap (G1)."""
    z = golden("g1_models"); enum_val = int(z[f"{name}_enum"])
    for i in range(4):
        x, u, dt = z[f"{name}_x"][i], z[f"{name}_u"][i], float(z[f"{name}_dt"][i])
        m = MODEL_CLASSES[enum_val](dt, 100)
        assert relerr(m(x, u), z[f"{name}_xn"][i]) < 1e-12 and relerr(m.f(x, u), z[f"{name}_f"][i]) < 1e-13
        A, B = m.linearize(x, u)
        assert relerr(A, z[f"{name}_A"][i]) < 1e-13 and relerr(B, z[f"{name}_B"][i]) < 1e-13
        assert relerr(dp.integrate(x, u, dt, dp.Model(enum_val)), z[f"{name}_xn"][i]) < 1e-12
    with pytest.raises(ValueError):
        dp.integrate(np.zeros(4), np.zeros(2), 0.1, 0)        # not a Model member (pyx:52-54)


def test_plugin_costs(dp, golden):
    z = golden("g2_costs")
    rc = dp.ReferenceCost(z["ref_xf"], z["ref_Q"], z["ref_R"], z["ref_Qf"], 100)
    for term, tag in ((False, "S"), (True, "T")):
        for i in range(2):
            assert abs(rc(z["ref_x"][i], z["ref_u"][i], term) - z[f"ref_cost_{tag}"][i]) < 1e-11
            q = rc.quadraticize(z["ref_x"][i], z["ref_u"][i], term)
            for got, nm in zip(q, ["Lx", "Lu", "Lxx", "Luu", "Lux"]):
                assert np.allclose(got, z[f"ref_{nm}_{tag}"][i], rtol=0, atol=1e-11), (nm, tag)
    # the reference's own (passing) ReferenceCost tests: tests/test_cost.py:52-78
    rc2 = dp.ReferenceCost(np.zeros(3), np.eye(3), np.eye(2), np.diag([1.0, 1, 0]), 101)
    x, u = z["reftest_x"], z["reftest_u"]
    assert abs(rc2(x, u) - (np.sum(x ** 2) + np.sum(u ** 2))) < 1e-12 and abs(rc2(x, u, terminal=True) - np.sum(x[:-1] ** 2)) < 1e-12
    for tag, ns in (("p2", 4), ("p3", 6), ("pm", 6)):
        pc = dp.ProximityCost([ns] * 3, 0.5, [int(v) for v in z[f"{tag}_ndims"]])
        for i in range(2):
            assert abs(pc(z[f"{tag}_x"][i]) - z[f"{tag}_cost"][i]) < 1e-13
            Lx, Lxx = pc.quadraticize(z[f"{tag}_x"][i])
            assert np.allclose(Lx, z[f"{tag}_Lx"][i], rtol=1e-11, atol=1e-12) and np.allclose(Lxx, z[f"{tag}_Lxx"][i], rtol=1e-11, atol=1e-11)
    for i in range(6):
        g, H = dp.quadraticize_distance(dp.Point(*z["qd_pa"][i, :z["qd_nd"][i]]), dp.Point(*z["qd_pb"][i, :z["qd_nd"][i]]),
                                        float(z["qd_radius"]), int(z["qd_nd"][i]))
        nd = int(z["qd_nd"][i])
        assert np.allclose(g, z["qd_Lx"][i, :nd], rtol=1e-12, atol=1e-13) and np.allclose(H, z["qd_Lxx"][i, :nd, :nd], rtol=1e-12, atol=1e-12)
    assert dp.ProximityCost([4], 0.5, [2])(np.zeros(4)) == 0.0
    k = 3
    refs = [dp.ReferenceCost(z["gc3_xf"][i * 4:(i + 1) * 4], np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), 100 + i)
            for i in range(k)]
    gc = dp.GameCost(refs, dp.ProximityCost([4] * k, 0.5, [2] * k))
    assert abs(gc(z["gc3_x"][0], z["gc3_u"][0]) - z["gc3_cost_S"][0]) < 1e-10 * abs(z["gc3_cost_S"][0])
    q = gc.quadraticize(z["gc3_x"][0], z["gc3_u"][0], terminal=True)
    assert np.allclose(q[0], z["gc3_Lx_T"][0], rtol=1e-12, atol=1e-10) and np.allclose(q[2], z["gc3_Lxx_T"][0], rtol=1e-12, atol=1e-10)
    assert not q[1].any() and not q[3].any()


@pytest.mark.parametrize("case", ["cfg1_di4d_k3", "quad6d_k3", "mixed_q6h6"])
def test_solver_passes(dp, golden, case):
    """ilqrSolver._rollout / _backward_pass / _forward_pass as the reference's callers use them (G3)."""
    z = golden(f"g3_passes_{case}")
    s = dp.ilqrSolver(problem_from(z), int(z["T"]))
    X, J = s._rollout(z["x0"].reshape(-1, 1), z["U0"])
    assert relerr(X, z["X_roll"]) < TOL_PASS and abs(J - z["J_roll"]) < TOL_PASS * abs(z["J_roll"])
    s.μ = float(z["mu"])
    K, d = s._backward_pass(z["X"], z["U"])
    assert relerr(K, z["K"]) < TOL_PASS and relerr(d, z["d"]) < TOL_PASS
    Xn, Un, Jn = s._forward_pass(z["X"], z["U"], z["K"], z["d"], np.float32(z["alphas"][2]))
    assert relerr(Xn, z["X_fwd"][2]) < TOL_PASS and relerr(Un, z["U_fwd"][2]) < TOL_PASS and abs(Jn - z["J_fwd"][2]) < TOL_PASS * abs(Jn)


@pytest.mark.parametrize("tag", ["cfg1", "quad_k3", "mixed", "di_k1"])
def test_solver_solve(dp, golden, tag, capsys):
    z = golden("g4_solves_misc")
    s = dp.ilqrSolver(problem_from(z, tag + "_"), int(z[tag + "_T"]))
    X, U, J = s.solve(z[tag + "_x0"].reshape(1, -1), z[tag + "_U0"], verbose=(tag == "cfg1"))
    assert relerr(X, z[tag + "_X"]) < TOL_SOLVE and relerr(U, z[tag + "_U"]) < TOL_SOLVE and abs(J - z[tag + "_J"]) < TOL_SOLVE * abs(J)
    assert s.n_bwd == len(z[tag + "_mu_trace"]) and s.on_device
    n_acc = int((z[tag + "_acc_trace"] >= 0).sum())
    ref = dp.ilqrSolver(s.problem, s.N)
    for _ in range(n_acc):
        ref._decrease_regularization()
    assert s.μ == ref.μ and s.Δ == ref.Δ           # solver object left in the reference's final state
    with pytest.raises(ValueError):
        s.solve(z[tag + "_x0"], np.zeros((3, 3)))  # wrong U shape (control.py:154-155)


def test_host_plugin_path_matches_device_path(dp, golden):
    """A user's DynamicalModel / Cost subclasses with HOST code: the solver calls them and feeds the GPU sweep
    with their tiles; result must equal the all-device solve of the same mathematical problem."""
    z = golden("g4_solves_misc"); tag = "uni_k3"
    prob = problem_from(z, tag + "_")

    class HostUnicycle(dp.DynamicalModel):          # the unicycle restated as a plain NumPy plugin
        def __init__(self, dt, id):
            super().__init__(4, 2, dt, id)

        def f(self, x, u):
            return np.array([x[2] * np.cos(x[3]), x[2] * np.sin(x[3]), u[0], u[1]])

        def __call__(self, x, u):                   # RK4 with 5 sub-steps, like the reference's C++ integrator
            h = self.dt / 5
            x = np.array(x, dtype=float)
            for _ in range(5):
                k0 = self.f(x, u); k1 = self.f(x + h / 2 * k0, u); k2 = self.f(x + h / 2 * k1, u); k3 = self.f(x + h * k2, u)
                x = x + h * (k0 + 2 * k1 + 2 * k2 + k3) / 6.0
            return x

        def linearize(self, x, u):
            A = np.eye(4); B = np.zeros((4, 2))
            A[0, 2] = self.dt * np.cos(x[3]); A[0, 3] = -self.dt * x[2] * np.sin(x[3])
            A[1, 2] = self.dt * np.sin(x[3]); A[1, 3] = self.dt * x[2] * np.cos(x[3])
            B[2, 0] = B[3, 1] = self.dt
            return A, B

    ids = prob.ids
    host_dyn = dp.MultiDynamicalModel([HostUnicycle(0.1, id_) for id_ in ids])
    host_prob = dp.ilqrProblem(host_dyn, prob.game_cost)
    hs = dp.ilqrSolver(host_prob, int(z[tag + "_T"]))
    assert not hs.on_device
    Xh, Uh, Jh = hs.solve(z[tag + "_x0"], z[tag + "_U0"], verbose=False)
    assert relerr(Xh, z[tag + "_X"]) < TOL_SOLVE and relerr(Uh, z[tag + "_U"]) < TOL_SOLVE and abs(Jh - z[tag + "_J"]) < TOL_SOLVE * abs(Jh)


@pytest.mark.parametrize("tag", ["uni5", "uni8", "quad10"])
def test_solve_distributed(dp, golden, tag):
    """solve_distributed(problem, X, U, radius, ignore_ids) vs the reference (G5), incl. the second,
    trajectory-seeded call of the receding-horizon pattern."""
    z = golden("g5_dispatch")
    prob = problem_from(z, tag + "_")
    Xd, Ud, Jf, info = dp.solve_distributed(prob, z[tag + "_x0"].reshape(1, -1), z[tag + "_U0"], 0.5, ignore_ids=[], verbose=False)
    assert relerr(Xd, z[tag + "_X_dec"]) < TOL_SOLVE and relerr(Ud, z[tag + "_U_dec"]) < TOL_SOLVE
    assert abs(Jf - z[tag + "_J_full"]) < TOL_SOLVE * abs(Jf) and set(info) == set(prob.ids)
    if tag + "_X_dec2" in z:
        # the receding-horizon pattern: a second call seeded with the (reference's) first result -> larger clusters
        Xd2, Ud2, Jf2, _ = dp.solve_distributed(prob, z[tag + "_X_dec"], z[tag + "_U_dec"], 0.5, ignore_ids=None,
                                                verbose=False)                                  # None tolerated (Q9)
        ns = prob.game_cost.x_dims[0]
        if tag == "uni5":
            assert relerr(Xd2, z[tag + "_X_dec2"]) < TOL_SOLVE and abs(Jf2 - z[tag + "_J_full2"]) < TOL_SOLVE * abs(Jf2)
        else:
            # uni8's second call has 4..8-agent unicycle clusters, several of which are chaotic in the reference
            # itself: the CPU oracle, which tracks the reference to 1e-15 elsewhere, lands 0.2-0.6 away on agents
            # 0, 2, 3, 4 there.  Agents 1, 6, 7 are well conditioned (oracle error < 1e-12) and are held to parity.
            for i in (1, 6, 7):
                assert relerr(Xd2[:, i * ns:(i + 1) * ns], z[tag + "_X_dec2"][:, i * ns:(i + 1) * ns]) < TOL_SOLVE, i
            assert np.isfinite(Xd2).all() and np.isfinite(Jf2)
    ign = prob.ids[1]
    Xi, Ui, _, info_i = dp.solve_distributed(prob, z[tag + "_x0"].reshape(1, -1), z[tag + "_U0"], 0.5, ignore_ids=[ign], verbose=False)
    ns = prob.game_cost.x_dims[0]
    assert not Xi[:, ns:2 * ns].any() and info_i[ign] == (0.0, [ign])           # ignored agent's columns stay zero
    assert relerr(Xi[:, :ns], z[tag + "_X_dec"][:, :ns]) < TOL_SOLVE


def test_device_graph_kernel(dp, golden):
    z = golden("g5_dispatch")
    for tag in ("uni5", "quad10", "uni8"):
        k, ns = int(z[tag + "_k"]), int(z[tag + "_n_s"])
        adj0 = dp.pairwise_graph(z[tag + "_x0"].reshape(1, 1, -1), 0.5, k, ns).cpu().numpy()[0]
        adj1 = dp.pairwise_graph(z[tag + "_X_dec"][None], 0.5, k, ns).cpu().numpy()[0]
        np.testing.assert_array_equal(adj0, z[tag + "_adj_x0"]); np.testing.assert_array_equal(adj1, z[tag + "_adj_traj"])


def test_selfish_warmstart_and_rhc(dp, golden):
    z = golden("g4_solves_misc"); tag = "cfg1"
    prob = problem_from(z, tag + "_"); T = 20
    Uw = prob.selfish_warmstart(z[tag + "_x0"], T)
    ns, nc = 4, 2
    for i, id_ in enumerate(prob.ids):          # each column block = that agent solving alone
        single = prob.split({id_: [id_]})[0]
        _, Ui, _ = dp.ilqrSolver(single, T).solve(z[tag + "_x0"][i * ns:(i + 1) * ns], verbose=False)
        assert relerr(Uw[:, i * nc:(i + 1) * nc], Ui) < 1e-12
    np.random.seed(0)
    Xf, Uf, Jf = dp.solve_rhc(prob, z[tag + "_x0"], 15, centralized=True, step_size=5, dist_converge=0.5, t_diverge=3.0)
    assert Xf.shape[1] == 12 and Uf.shape[0] == Xf.shape[0] and np.isfinite(Jf)
    goal = z[tag + "_xf"].reshape(3, 4)[:, :2]; start = z[tag + "_x0"].reshape(3, 4)[:, :2]; end = Xf[-1].reshape(3, 4)[:, :2]
    assert np.linalg.norm(end - goal) < np.linalg.norm(start - goal)


@pytest.mark.parametrize("tag", ["uni5", "quad10"])
def test_solve_scenarios_distributed_equals_per_scenario_calls(dp, golden, tag):
    """The Monte-Carlo front end (many scenarios of one problem, array code + one device solve per cluster size)
    must give, scenario by scenario, exactly what solve_distributed gives -- including the golden scenario, which
    is the reference's own answer (G5)."""
    from dpilqr_amd.dispatch import solve_scenarios_distributed
    z = golden("g5_dispatch")
    prob = problem_from(z, tag + "_")
    k = len(prob.ids); ns = prob.game_cost.x_dims[0]
    T = z[tag + "_U0"].shape[0]
    rng = np.random.default_rng(5)
    S = 6
    x0 = np.tile(z[tag + "_x0"].reshape(1, -1), (S, 1))
    jitter = rng.normal(scale=0.15, size=(S, k, ns)); jitter[:, :, 2:] = 0.0; jitter[0] = 0.0     # scenario 0 = golden
    x0 = x0 + jitter.reshape(S, -1)
    U0 = np.tile(z[tag + "_U0"][None], (S, 1, 1))
    Xd, Ud, Jf, info = solve_scenarios_distributed(prob, x0[:, None, :], U0, 0.5)
    assert relerr(Xd[0], z[tag + "_X_dec"]) < TOL_SOLVE and abs(Jf[0] - z[tag + "_J_full"]) < TOL_SOLVE * abs(Jf[0])
    assert info["n_subproblems"] == S * k and info["n_unique"] <= S * k
    for s in range(S):
        Xs, Us, Js, _ = dp.solve_distributed(prob, x0[s].reshape(1, -1), U0[s], 0.5, ignore_ids=[], verbose=False)
        assert (Xd[s] == Xs).all() and (Ud[s] == Us).all() and Jf[s] == Js, s


def test_edge_cases_empty_batch_short_horizon_no_iterations(dp):
    """The corners the reference's API allows: an empty batch, a one-step horizon, n_lqr_iter = 0 (solve() then
    returns the rollout of the warm start, control.py:164-168), a window of one, and a bad argument's error code."""
    from oracle import oracle as orc
    Q, R, Qf = np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4)
    rng = np.random.default_rng(3)
    # empty batch
    pb0 = dp.ProblemBatch([0, 0], [2, 2], np.zeros((0, 8)), Q, R, Qf, 0.5, 0.1, 5, B=0)
    r0 = pb0.solve(np.zeros((0, 8)), np.zeros((0, 5, 4)))
    assert r0["X"].shape == (0, 6, 8) and r0["J"].shape == (0,)
    # one-step horizon, two agents, against the oracle
    B, T, k = 3, 1, 2
    xf = rng.normal(size=(B, 4 * k)); x0 = rng.normal(size=(B, 4 * k))
    pb = dp.ProblemBatch([0] * k, [2] * k, xf, Q, R, Qf, 0.5, 0.1, T)
    r = pb.solve(x0, np.zeros((B, T, 2 * k)), trace=True)
    proto = orc.Problem([0] * k, [2] * k, xf[0], Q, R, Qf, 0.5, 0.1, T)
    o = orc.solve_batch(proto, x0, xf, np.zeros((B, T, 2 * k)))
    assert relerr(r["X"].cpu().numpy(), o["X"]) < TOL_SOLVE and (r["n_bwd"].cpu().numpy() == o["n_bwd"]).all()
    # n_lqr_iter = 0: the rollout of the warm start, no backward pass
    U0 = rng.normal(size=(B, T, 2 * k)) * 0.1
    rz = pb.solve(x0, U0, n_lqr_iter=0)
    Xr, Jr = pb.rollout(x0, U0)
    assert (rz["X"] == Xr).all().item() and (rz["n_bwd"] == 0).all().item() and relerr(rz["J"].cpu().numpy(), Jr.cpu().numpy()) < 1e-14
    # a window of one sub-problem in flight
    r1 = pb.solve(x0, np.zeros((B, T, 2 * k)), window=1)
    assert (r1["X"] == r["X"]).all().item()
    # errors come back as codes + message, never as a crash
    lib = dp._lib.load()
    assert lib.dpilqr_backward_pass_tiles(1, 0, 4, 2, None, None, None, None, None, None, None, None) == -1   # DPILQR_EINVAL
    assert b"bad sizes" in lib.dpilqr_last_error()


@pytest.mark.parametrize("centralized", [True, False])
def test_rhc_scenarios_equal_per_scenario_rhc(dp, golden, centralized):
    """The lock-step receding-horizon loop over several scenarios must reproduce, scenario by scenario, what
    solve_rhc (distributed.py:106-221) gives when run on each alone with the same warm start."""
    z = golden("g4_solves_misc"); tag = "cfg1"
    prob = problem_from(z, tag + "_")
    n_x, n_u, N, S = 12, 6, 12, 3
    rng = np.random.default_rng(11)
    x0 = np.tile(z[tag + "_x0"].reshape(1, -1), (S, 1))
    jit = rng.normal(scale=0.1, size=(S, 3, 4)); jit[:, :, 2:] = 0.0; jit[0] = 0.0
    x0 = x0 + jit.reshape(S, -1)
    U0 = np.zeros((S, N, n_u))
    for s in range(S):
        np.random.seed(40 + s)
        U0[s] = np.random.rand(N, n_u) * 0.01
    args = () if centralized else (0.5,)
    kw = dict(centralized=centralized, step_size=4, dist_converge=0.6, t_diverge=2.0)
    batched = dp.solve_rhc_scenarios(prob, x0, N, 0.5, U0=U0, **kw)
    for s in range(S):
        np.random.seed(40 + s)                      # solve_rhc draws its warm start from the global RNG
        Xs, Us, Js = dp.solve_rhc(prob, x0[s], N, *args, **kw)
        Xb, Ub, Jb, _ = batched[s]
        assert Xb.shape == Xs.shape and (Xb == Xs).all() and (Ub == Us).all() and Jb == Js, s


def _perturbed_scenarios(z, tag, S, seed=9):
    rng = np.random.default_rng(seed)
    k = int(z[tag + "_k"]); ns = int(z[tag + "_n_s"])
    x0 = np.tile(z[tag + "_x0"].reshape(1, -1), (S, 1)); x0[1:, 0::ns] += rng.normal(scale=0.15, size=(S - 1, k))
    U0 = np.tile(z[tag + "_U0"][None], (S, 1, 1))
    return x0, U0


def test_scenarios_sharded_single_rank_equals_front_end(dp, golden):
    """sharding.solve_scenarios_sharded with the real device solver behind it (one rank, gloo for the collective on
    CPU copies is not needed: world 1 gathers in place): the gathered result must be the front end's own."""
    import socket
    import torch.distributed as dist
    from dpilqr_amd.dispatch import solve_scenarios_distributed
    from dpilqr_amd.sharding import solve_scenarios_sharded
    z = golden("g5_dispatch"); tag = "uni5"
    prob = problem_from(z, tag + "_")
    S = 4
    x0, U0 = _perturbed_scenarios(z, tag, S)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        Xg, Ug, Jg, info = solve_scenarios_sharded(prob, x0[:, None, :], U0, 0.5)
        # ... and the batch-sharded form over the same RCCL group: the chunked all-gather issued from inside the solve's
        # progress callback, on a side stream, while the solve's own stream is busy (bench.py's N > 1 path with one rank)
        import torch
        from dpilqr_amd.sharding import ResultBuffers
        from dpilqr_amd.util import random_setup_batch
        from tests.golden_util import cfg2_params
        c = cfg2_params(); Bc = 2500
        xc0, xcf = random_setup_batch((31000, Bc), 5, 4, var=2.5, n_d=2, energy=10.0)
        pbc = dp.ProblemBatch(c["model"], c["n_dims"], xcf, c["Q"], c["R"], c["Qf"], c["radius"], c["dt"], c["T"])
        Uc0 = torch.zeros((Bc, 50, 10), dtype=torch.float64, device="cuda")
        ref = pbc.solve(xc0, Uc0, window=512)
        rb = ResultBuffers(Bc, 50, 20, 10, chunk=512, device=torch.device("cuda"))
        assert rb.collective and rb.world == 1
        rb.warm()
        sent_early = []
        for _ in range(2):
            rb.begin()
            pbc.solve(xc0, Uc0, window=512, out=rb.out, progress=lambda n, tot: (rb.progress(n, tot), sent_early.append(rb._sent)))
            rb.finish()
            torch.cuda.synchronize()
            g = rb.results()
            for key in ("X", "U", "J", "status", "n_bwd", "n_fwd"):
                assert torch.equal(g[key][0], ref[key]), key
        assert max(sent_early) >= 2            # chunks went out while the solve was still running
    finally:
        dist.destroy_process_group()
    Xd, Ud, Jd, _ = solve_scenarios_distributed(prob, x0[:, None, :], U0, 0.5)
    assert (Xg == Xd).all() and (Ug == Ud).all() and (Jg == Jd).all() and info["shard_rows"] == [S * 5]


@pytest.mark.parametrize("tag,world", [("uni5", 2), ("quad10", 3), ("uni8", 8)])
def test_bucket_sharded_rows_of_several_ranks_rebuild_the_unsharded_result(dp, golden, tag, world):
    """The multi-GPU partitioning on ONE GPU, rank after rank: every rank solves its 1 / world share of every size bucket and
    packs one row per (scenario, agent) it owns; the rank-major concatenation of the padded blocks -- what the all-gather
    delivers -- scattered back must be the unsharded front end's result bit for bit, every (scenario, agent) exactly once."""
    import torch
    from dpilqr_amd.dispatch import solve_scenarios_distributed
    z = golden("g5_dispatch")
    prob = problem_from(z, tag + "_")
    S = 7
    x0, U0 = _perturbed_scenarios(z, tag, S)
    Xd, Ud, Jd, info = solve_scenarios_distributed(prob, x0[:, None, :], U0, 0.5, device_out=True)
    blocks, counts = [], []
    for rank in range(world):
        fe, solved, _ = solve_scenarios_distributed(prob, x0[:, None, :], U0, 0.5, shard=(rank, world))
        _, n = fe.pack_rows(solved, count_only=True)
        counts.append(n)
    pad = max(counts + [1])
    for rank in range(world):
        fe, solved, _ = solve_scenarios_distributed(prob, x0[:, None, :], U0, 0.5, shard=(rank, world))
        rows, n = fe.pack_rows(solved, pad_to=pad)
        assert n == counts[rank] and int((rows[:, 0] >= 0).sum()) == n
        blocks.append(rows)
    k = int(z[tag + "_k"])
    assert sum(counts) == S * k
    allrows = torch.cat(blocks, dim=0)
    idx = allrows[:, 0][allrows[:, 0] >= 0].cpu().numpy().astype(int)
    assert sorted(idx.tolist()) == list(range(S * k))
    Xs, Us = fe.scatter_rows(allrows)
    assert torch.equal(Xs, Xd) and torch.equal(Us, Ud)
    # balance: no rank holds more than its share of any bucket plus one
    for kc, n_kc in info["sizes"].items():
        assert n_kc >= 0


def test_front_end_on_device_equals_per_scenario_host_graphs(dp, golden):
    """The device front end (bit masks, de-duplication, size buckets) against the host definitions, scenario by scenario."""
    import torch
    from dpilqr_amd.dispatch import ScenarioFrontEnd
    from dpilqr_amd.lowering import describe
    z = golden("g5_dispatch"); tag = "quad10"
    prob = problem_from(z, tag + "_")
    S = 9
    x0, U0 = _perturbed_scenarios(z, tag, S, seed=3)
    fe = ScenarioFrontEnd(describe(prob), x0[:, None, :], U0, 0.5, None)
    k = fe.k
    bits = fe.bits.cpu().numpy().reshape(S, k); rep = fe.rep.cpu().numpy().reshape(S, k); size = fe.size.cpu().numpy().reshape(S, k)
    order = fe.order.cpu().numpy(); slot = fe.slot.cpu().numpy().reshape(S, k)
    ids = prob.ids
    n_unique = 0
    for s in range(S):
        g = dp.define_inter_graph_threshold(x0[s].reshape(1, -1), 0.5, prob.game_cost.x_dims, ids)
        masks = [sum(1 << ids.index(int(j)) for j in g[id_]) for id_ in ids]
        assert list(bits[s]) == masks
        for i in range(k):
            first = masks.index(masks[i])
            assert rep[s, i] == first and size[s, i] == bin(masks[i]).count("1")
            n_unique += first == i
    assert int(fe.counts.sum()) == n_unique
    # the buckets: representatives sorted by size, (s, i) ascending inside a size, slot = position in the bucket
    pos = 0
    for kc in range(1, k + 1):
        want = [s * k + i for s in range(S) for i in range(k) if rep[s, i] == i and size[s, i] == kc]
        assert list(order[pos:pos + len(want)]) == want and fe.counts[kc] == len(want) and fe.starts[kc] == pos
        for j, e in enumerate(want):
            assert slot.reshape(-1)[e] == j
        pos += len(want)


def test_profile_totals_by_sweep_variant(dp):
    """dpilqr_profile_read_sweep splits the sweep's profile class by the variant that ran (wavefronts per workgroup),
    which is how bench.py's roofline object follows ONE kernel name of a rocprofv3 trace: the variants' launches and
    items add up to the class totals, and the items equal the backward passes the solver counted."""
    from dpilqr_amd import _lib
    rng = np.random.default_rng(5)
    B, k, T = 2500, 5, 8
    xf = rng.normal(size=(B, 4 * k)); x0 = xf + 0.3 * rng.normal(size=(B, 4 * k))
    pb = dp.ProblemBatch([0] * k, [2] * k, xf, np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), 0.5, 0.1, T)
    _lib.profile_enable(True); _lib.profile_read(reset=True)
    for w in (4, 8, 12):
        _lib.profile_read_sweep(w, reset=True)
    try:
        r = pb.solve(x0, np.zeros((B, T, 2 * k)), n_lqr_iter=6, tol=1e-3)
        tot = _lib.profile_read(reset=True)["riccati"]
        var = {w: _lib.profile_read_sweep(w, reset=True) for w in (4, 8, 12)}
    finally:
        _lib.profile_enable(False)
    assert var[12]["launches"] >= 1 and var[12]["items"] >= B            # the first iteration sweeps all 2500 items
    assert sum(v["launches"] for v in var.values()) == tot["launches"]
    assert sum(v["items"] for v in var.values()) == tot["items"] == int(r["n_bwd"].sum().item())
    assert abs(sum(v["ms"] for v in var.values()) - tot["ms"]) < 1e-6 * max(tot["ms"], 1.0)
    with pytest.raises(Exception):
        _lib.profile_read_sweep(5)


def test_solve_workspaces_are_pooled(dp):
    """Solve workspaces come from one process-wide pool (batch._WorkspacePool): a second solve of any ProblemBatch
    reuses the first one's buffer, a larger request gets a new (rounded) one, release_workspaces() empties the pool."""
    from dpilqr_amd import batch
    rng = np.random.default_rng(11)
    dp.release_workspaces()
    pool = batch._workspace_pool

    def solve(B, k):
        xf = rng.normal(size=(B, 4 * k)); x0 = xf + 0.2 * rng.normal(size=(B, 4 * k))
        pb = dp.ProblemBatch([0] * k, [2] * k, xf, np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), 0.5, 0.1, 5)
        return pb.solve(x0, np.zeros((B, 5, 2 * k)), n_lqr_iter=3)

    solve(64, 3)
    assert len(pool._free) == 1
    first = pool._free[0].data_ptr()
    assert pool._free[0].numel() % batch._WorkspacePool.GRANULE == 0
    solve(32, 2)                                   # smaller request: the same buffer serves it
    assert len(pool._free) == 1 and pool._free[0].data_ptr() == first
    big = pool._free[0].numel() + 1
    buf = pool.acquire(big)                        # larger than anything pooled: a new buffer, the old one stays
    assert buf.numel() >= big and len(pool._free) == 1
    pool.release(buf)
    assert len(pool._free) == 2
    dp.release_workspaces()
    assert len(pool._free) == 0


# ---------------------------------------------------------------- G7: the callers, pinned to the reference
class _Rows(__import__("logging").Handler):
    def __init__(self):
        super().__init__()
        self.rows = []

    def emit(self, record):
        self.rows.append(record.getMessage())


@pytest.mark.parametrize("tag", ["rhc_c", "rhc_c2", "rhc_d"])
def test_solve_rhc_vs_reference(dp, golden, tag):
    """solve_rhc (distributed.py:106-221), centralized and distributed branch, against the reference's own run: the
    executed trajectory, the final cost and every logged CSV row (fields that are not wall-clock times: exact for the
    discrete ones, 1e-6 for the floats; the row FORMAT is checked byte for byte in test_host_logic.py)."""
    import logging
    from tests.test_host_logic import _parse_row
    z = golden("g7_callers")
    prob = problem_from(z, tag + "_")
    N = int(z[tag + "_N"]); centralized = bool(z[tag + "_centralized"])
    kw = dict(step_size=int(z[tag + "_kw_step_size"]), dist_converge=float(z[tag + "_kw_dist_converge"]),
              t_diverge=float(z[tag + "_kw_t_diverge"]))
    np.random.seed(int(z[tag + "_np_seed"]))                      # solve_rhc draws its warm start from the global RNG (:152)
    log = logging.getLogger(); old = log.level; log.setLevel(logging.INFO)
    h = _Rows(); log.addHandler(h)
    try:
        args = () if centralized else (0.5, [])
        Xf, Uf, Jf = dp.solve_rhc(prob, z[tag + "_x0"], N, *args, centralized=centralized, i_trial=7, **kw)
    finally:
        log.removeHandler(h); log.setLevel(old)
    assert Xf.shape == z[tag + "_X_full"].shape and Uf.shape == z[tag + "_U_full"].shape
    assert relerr(Xf, z[tag + "_X_full"]) < TOL_SOLVE and relerr(Uf, z[tag + "_U_full"]) < TOL_SOLVE
    assert abs(Jf - float(z[tag + "_J_full"])) < TOL_SOLVE * abs(float(z[tag + "_J_full"]))
    ref_rows = [str(r) for r in z[tag + "_rows"]]
    assert len(h.rows) == len(ref_rows)
    for mine, ref in zip(h.rows, ref_rows):
        a, b = _parse_row(mine), _parse_row(ref)
        for key in ("model_name", "n_agents", "i_trial", "centralized", "last", "N", "dt", "converged", "ids"):
            assert a[key] == b[key], key
        assert repr(a["subgraphs"]) == repr(b["subgraphs"])          # NumPy-int neighbours next to Python-int owners (Q10)
        assert repr(a["t"]) == repr(b["t"])
        assert abs(a["J"] - b["J"]) < 1e-6 * abs(b["J"]) and np.allclose(a["left"], b["left"], rtol=1e-6, atol=1e-9)
        assert len(a["times"]) == len(b["times"])                      # wall-clock seconds: the one field that cannot match


@pytest.mark.parametrize("tag", ["ws_uni", "ws_di"])
def test_selfish_warmstart_vs_reference(dp, golden, tag):
    """ilqrProblem.selfish_warmstart (problem.py:66-91): one k = 1 batch on the device against the reference's loop."""
    z = golden("g7_callers")
    prob = problem_from(z, tag + "_")
    Uw = prob.selfish_warmstart(z[tag + "_x0"], int(z[tag + "_N"]))
    assert Uw.shape == z[tag + "_U_warm"].shape and relerr(Uw, z[tag + "_U_warm"]) < TOL_SOLVE


def test_solve_subproblem_vs_reference(dp, golden):
    """solve_subproblem((subproblem, x0, U, id_, verbose)) (problem.py:97-105) -- the worker the reference's dispatch loop and
    its multiprocessing pool call -- on the sub-problems of a proximity graph, plus its starmap form."""
    from dpilqr_amd.problem import solve_subproblem, solve_subproblem_starmap
    z = golden("g7_callers")
    prob = problem_from(z, "sub_")
    ids = prob.ids; T = int(z["sub_T"])
    graph = dp.define_inter_graph_threshold(z["sub_x0"].reshape(1, -1), 0.5, prob.game_cost.x_dims, ids)
    adj = np.zeros((len(ids), len(ids)), dtype=np.int32)
    for i, id_ in enumerate(ids):
        adj[i, [ids.index(int(j)) for j in graph[id_]]] = 1
    np.testing.assert_array_equal(adj, z["sub_adj"])
    subs = prob.split(graph)
    x0s = dp.split_graph(z["sub_x0"].reshape(1, -1), prob.game_cost.x_dims, graph)
    U0s = dp.split_graph(np.zeros((T, prob.dynamics.n_u)), prob.game_cost.u_dims, graph)
    for i, id_ in enumerate(ids):
        Xi, Ui, rid = solve_subproblem((subs[i], x0s[i], U0s[i], id_, False))
        assert rid == id_ and Xi.shape == z[f"sub_X_{i}"].shape
        assert relerr(Xi, z[f"sub_X_{i}"]) < TOL_SOLVE and relerr(Ui, z[f"sub_U_{i}"]) < TOL_SOLVE
    Xi, Ui, rid = solve_subproblem_starmap(subs[0], x0s[0], U0s[0], ids[0])
    assert rid == ids[0] and relerr(Xi, z["sub_X_0"]) < TOL_SOLVE


@pytest.mark.parametrize("tag,k,ns,nd", [("k5s4", 5, 4, 2), ("k3s4", 3, 4, 2), ("k10s6", 10, 6, 3), ("k15s4", 15, 4, 2)])
def test_scenarios_generated_on_the_device_equal_the_references(dp, golden, tag, k, ns, nd):
    """dpilqr_random_setup against the reference's own np.random.seed(s); random_setup(...) outputs (G6), bit for bit, and
    against the host generator for seeds the fixture does not hold (large seeds, more than one MT19937 block is never
    needed: 4 k n_d <= 624 draws)."""
    from dpilqr_amd.util import random_setup, random_setup_batch
    z = golden("g6_scenarios")
    x0, xf = random_setup_batch(range(0, 8), k, ns, var=k / 2, n_d=nd, energy=10.0)
    np.testing.assert_array_equal(x0.cpu().numpy(), z[tag + "_x0"]); np.testing.assert_array_equal(xf.cpu().numpy(), z[tag + "_xf"])
    for seed0 in (1000, 4_000_000_000):
        a, b = random_setup_batch((seed0, 33), k, ns, var=k / 2, n_d=nd, energy=10.0)
        for i in (0, 7, 32):
            np.random.seed(seed0 + i)
            h0, hf = random_setup(k, ns, is_rotation=False, rel_dist=k, var=k / 2, n_d=nd, random=True, energy=10.0)
            np.testing.assert_array_equal(a[i].cpu().numpy(), h0.ravel()); np.testing.assert_array_equal(b[i].cpu().numpy(), hf.ravel())
    a, b = random_setup_batch((5, 4), k, ns, var=2.0, n_d=nd, energy=None)          # no normalisation
    np.random.seed(5)
    h0, hf = random_setup(k, ns, is_rotation=False, var=2.0, n_d=nd, random=True, energy=None)
    np.testing.assert_array_equal(a[0].cpu().numpy(), h0.ravel())


def test_progress_reports_and_chunked_gather_world1(dp):
    """The solve's progress callback (dpilqr_solver_set_progress) reports a growing finished PREFIX while later items still
    solve, and sharding.ResultBuffers gathers those chunks on a side stream as they complete; with one rank the 'gather'
    is a copy, and the gathered results must be the plain solve's bit for bit."""
    import torch
    from dpilqr_amd.sharding import ResultBuffers
    from dpilqr_amd.util import random_setup_batch
    from tests.golden_util import cfg2_params
    c = cfg2_params(); B = 3000
    x0, xf = random_setup_batch((12000, B), 5, 4, var=2.5, n_d=2, energy=10.0)
    pb = dp.ProblemBatch(c["model"], c["n_dims"], xf, c["Q"], c["R"], c["Qf"], c["radius"], c["dt"], c["T"])
    U0 = torch.zeros((B, 50, 10), dtype=torch.float64, device="cuda")
    ref = pb.solve(x0, U0, window=512)
    rb = ResultBuffers(B, 50, 20, 10, chunk=512, device=torch.device("cuda"))
    rb.warm()
    for _ in range(2):                                   # the buffers are reused job after job
        calls = []

        side = torch.cuda.Stream()

        def prog(n, total):
            # what is reported finished IS final AT CALLBACK TIME: the chunk gather is issued first, with no synchronisation of the
            # solve's stream (which still has look-ahead iterations queued), then the prefix's X, U and status are snapshotted
            # by a side stream that waits for nothing; the snapshots are compared with the plain solve after this one has ended
            rb.progress(n, total)
            with torch.cuda.stream(side):
                lo = calls[-1][0] if calls else 0
                snap = (rb.out["X"][lo:n].clone(), rb.out["U"][lo:n].clone(), rb.out["status"][lo:n].clone())
            calls.append((n, total, lo, snap))

        rb.begin()
        r = pb.solve(x0, U0, window=512, out=rb.out, progress=prog)
        rb.finish()
        torch.cuda.synchronize()
        g = rb.results()
        for key in ("X", "U", "J", "status", "n_bwd", "n_fwd"):
            assert torch.equal(g[key][0], ref[key]), key
            assert torch.equal(r[key], ref[key]), key
        ns = [c_[0] for c_ in calls]
        assert ns == sorted(ns) and ns[-1] == B and all(c_[1] == B for c_ in calls)
        for n, _, lo, (sx, su, ss) in calls:
            assert torch.equal(sx, ref["X"][lo:n]) and torch.equal(su, ref["U"][lo:n]) and torch.equal(ss, ref["status"][lo:n]), \
                f"items {lo}..{n} were reported finished before their results were final"
        assert len([n for n in ns if 0 < n < B]) >= 2    # progress was reported while the solve was still running


def test_bench_two_ranks_on_one_gpu_over_gloo():
    """bench.py's N > 1 path end to end with two processes (torch.distributed.run, backend gloo through
    DPILQR_BENCH_BACKEND, both ranks on the one GPU of the box): per-rank seeds, results written into ResultBuffers, chunks
    all-gathered from the solve's progress callback on a side stream while the solve runs, barrier + MAX over ranks, one JSON
    line from rank 0 -- and bench.py's own check that each rank's block of the gathered results is what that rank solved."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    env = dict(os.environ, DPILQR_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(root / "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--reps", "2",
           "--gather-chunk", "512", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=str(root))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and len(d["repetitions"]["ms_per_step"]) == 2
    assert "all-gather in chunks of 512" in d["config"]["parallelism"]


def _run_bench(args, env_extra, timeout=900):
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, str(root / "bench.py"), *args], env=env, capture_output=True, text=True,
                          timeout=timeout, cwd=str(root))


def test_plain_bench_gpus_2_starts_two_ranks_itself():
    """`python bench.py --gpus 2` with no launcher in front (the driver's command shape for N = 1, extended to N): bench.py
    starts its own two ranks before anything touches the GPU and rank 0's line says n_gpus = 2 (gloo, both ranks on the one GPU
    of this box: the multi-rank path as a diagnostic)."""
    import json
    out = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--reps", "2", "--gather-chunk", "512", "--no-cpu-baseline",
                      "--full"], {"DPILQR_BENCH_BACKEND": "gloo"})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0's)"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["roofline"]["launches"] > 0
    assert "cpu_baseline" not in d                       # N = 1 only
    # the line validates itself: the rank count is the process group's, every rank names its device and its own throughput
    assert d["ranks_seen"] == 2 and d["backend"] == "gloo" and d["n1_path"] is None
    assert [r["rank"] for r in d["ranks"]] == [0, 1] and len({r["pid"] for r in d["ranks"]}) == 2
    assert all(r["value"] > 0 and r["device_name"] and r["pci_bus"] for r in d["ranks"])
    assert d["value"] <= sum(r["value"] for r in d["ranks"]) * 1.0001        # MAX over ranks bounds the job's time
    assert "batch-sharded x2" in d["config"]["parallelism"]


def test_plain_bench_times_its_steps_once_and_dumps_the_last_step(dp, tmp_path):
    """A plain `bench.py` line: --steps steps timed once, none of the --full legs; --dump-outputs writes the last step's items
    (seeds (K-1)*B .. K*B-1 of rank 0) as float64 arrays, equal to a solve of those seeds on their own (the window's schedule
    does not change an item's arithmetic)."""
    import json
    import torch
    from dpilqr_amd.util import random_setup_batch
    K, B = 2, 256
    out = _run_bench(["--gpus", "1", "--steps", str(K), "--warmup", "1", "--batch", str(B), "--dump-outputs", str(tmp_path)], {},
                     timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == K and d["repetitions"]["n"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["metric"] == "ilqr_subproblems_per_sec" and d["unit"] == "subproblems/s" and d["dtype"] == "f64" and d["higher_is_better"]
    assert not {"roofline", "cpu_baseline", "configs", "single_batch_1024"} & set(d)
    x0, xf = random_setup_batch(((K - 1) * B, B), 5, 4, var=2.5, n_d=2, energy=10.0)
    pb = dp.ProblemBatch([0] * 5, [2] * 5, xf, np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), 0.5, 0.1, 50)
    r = pb.solve(x0, torch.zeros((B, 50, 10), dtype=torch.float64, device="cuda"), n_lqr_iter=50, tol=1e-3)
    for k in ("X", "U", "J", "status", "n_bwd", "n_fwd"):
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == tuple(r[k].shape), k
        np.testing.assert_array_equal(a, r[k].cpu().numpy().astype(np.float64), err_msg=k)


def test_plain_bench_gpus_2_on_one_gpu_over_rccl_fails_loudly():
    """Without the diagnostic backend two ranks need two GPUs: on a one-GPU box the run must end non-zero with a message that
    says so -- never a silent one-GPU line."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer than two GPUs")
    out = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "0", "--reps", "1", "--no-cpu-baseline"], {}, timeout=300)
    assert out.returncode != 0
    assert "needs 2 visible GPUs" in out.stderr and not [l for l in out.stdout.splitlines() if l.startswith("{")]
