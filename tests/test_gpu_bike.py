"""BikeDynamics5D on the device (the five-state family), against the real reference's numbers (G11,
tests/golden/make_golden_bike.py): the model FFI, single passes, whole solves with their decision traces through ilqrSolver and
through many-item batches, solve_distributed, the in-sweep production sweep against the record-fed one, and what the family
does not serve (thirteen or more bikes, the fp32 arm)."""
import numpy as np
import pytest
import torch

from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

TOL_PASS, TOL_SOLVE = 1e-9, 1e-5
PASS_KS = [1, 2, 3, 4, 6, 12]


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()
    return dpilqr_amd


def bike_problem(dp, z, pre=""):
    g = lambda k: z[pre + k]
    k = int(g("k"))
    ids = [int(i) for i in g("ids")]
    dyn = dp.MultiDynamicalModel([dp.BikeDynamics5D(float(g("dt")), id_) for id_ in ids])
    refs = [dp.ReferenceCost(g("xf")[5 * i:5 * i + 5], g("Q")[i], g("R")[i], g("Qf")[i], ids[i]) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([5] * k, float(g("radius")), [int(v) for v in g("n_dims")])))


def bike_batch(dp, z, pre="", xf=None):
    g = lambda k: z[pre + k]
    xf = g("xf")[None] if xf is None else xf
    return dp.ProblemBatch(g("model"), g("n_dims"), xf, g("Q"), g("R"), g("Qf"), float(g("radius")), float(g("dt")), int(g("T")))


def test_model_ffi(dp, golden):
    """dpilqr_model_f / integrate (ONE RK4 step of dt) / linearize against the reference's sympy model (G11 (a)): headings
    up to 1e3 rad, phi up to 1.4, dt 0.05 / 0.1 / 0.5; and the plugin methods of BikeDynamics5D on a few of the points."""
    from dpilqr_amd import _lib
    from dpilqr_amd.device import empty, ptr, stream_handle, to_dev
    z = golden("g11_bike_models"); lib = _lib.load()
    x, u, dts = z["x"], z["u"], z["dt"]
    n = len(x)
    model = to_dev(np.full(n, 10), torch.int32); xd, ud = to_dev(x), to_dev(u)
    f = empty((n, 5)); _lib.check(lib.dpilqr_model_f(n, 5, ptr(model), ptr(xd), ptr(ud), ptr(f), stream_handle()))
    f = f.cpu().numpy()
    for i in range(n):
        assert relerr(f[i], z["f"][i]) < 1e-12, i
    for dt in (0.05, 0.1, 0.5):
        sel = np.where(dts == dt)[0]
        xn = empty((n, 5)); A = empty((n, 5, 5)); Bm = empty((n, 5, 2))
        _lib.check(lib.dpilqr_model_integrate(n, 5, ptr(model), ptr(xd), ptr(ud), dt, ptr(xn), stream_handle()))
        _lib.check(lib.dpilqr_model_linearize(n, 5, ptr(model), ptr(xd), ptr(ud), dt, ptr(A), ptr(Bm), stream_handle()))
        xn, A, Bm = xn.cpu().numpy(), A.cpu().numpy(), Bm.cpu().numpy()
        for i in sel:
            assert relerr(xn[i], z["xn"][i]) < 1e-12 and relerr(A[i], z["A"][i]) < 1e-12 and relerr(Bm[i], z["B"][i]) < 1e-12, i
    for i in range(0, n, 37):
        m = dp.BikeDynamics5D(float(dts[i]), 100)
        assert relerr(m(x[i], u[i]), z["xn"][i]) < 1e-12 and relerr(m.f(x[i], u[i]), z["f"][i]) < 1e-12
        A, B = m.linearize(x[i], u[i])
        assert relerr(A, z["A"][i]) < 1e-12 and relerr(B, z["B"][i]) < 1e-12


@pytest.mark.parametrize("k", PASS_KS)
def test_passes(dp, golden, k):
    """rollout, backward pass (K, d at the solver's mu) and the ten-alpha forward pass of k bikes with proximity costs (G11 (b));
    the solver's own route for the backward pass (in-sweep production at k <= 4) where it applies."""
    from dpilqr_amd.device import to_dev
    z = golden(f"g11_bike_passes_k{k}")
    pb = bike_batch(dp, z)
    X, J = pb.rollout(z["x0"][None], z["U0"][None])
    assert relerr(X.cpu().numpy()[0], z["X_roll"]) < TOL_PASS and abs(J.item() - z["J_roll"]) < TOL_PASS * abs(z["J_roll"])
    mu = to_dev(np.array([float(z["mu"])]))
    Xd = to_dev(z["X"][None])
    K, d = pb.backward_pass(Xd, z["U"][None], mu)
    assert relerr(K.cpu().numpy()[0], z["K"]) < TOL_PASS and relerr(d.cpu().numpy()[0], z["d"]) < TOL_PASS
    if k <= 4:
        Kf, df = pb.backward_pass_fused(Xd, z["U"][None], mu)
        assert relerr(Kf.cpu().numpy()[0], z["K"]) < TOL_PASS and relerr(df.cpu().numpy()[0], z["d"]) < TOL_PASS
    Xn, Un, Jn = pb.forward_pass(z["X"][None], z["U"][None], z["K"][None], z["d"][None], z["alphas"])
    Xn, Un, Jn = Xn.cpu().numpy()[0], Un.cpu().numpy()[0], Jn.cpu().numpy()[0]
    for a in range(len(z["alphas"])):
        # A candidate whose steering angles stay inside (-pi/2, pi/2) is held to 1e-9.  The long steps of these operating
        # points steer some bikes through tan's poles (|phi| up to 270 rad at alpha = 1): there one ulp of tan -- the device's
        # against NumPy's, both faithful -- grows to 1e-7 over the horizon in the reference itself (the same recursion in NumPy
        # with tan, sin, cos perturbed by one ulp), and such candidates are held to 1e-4.
        tol = TOL_PASS if float(np.abs(z["X_fwd"][a][:, 4::5]).max()) < np.pi / 2 else 1e-4
        assert relerr(Xn[a], z["X_fwd"][a]) < tol and relerr(Un[a], z["U_fwd"][a]) < tol, a
        assert abs(Jn[a] - z["J_fwd"][a]) < tol * abs(z["J_fwd"][a]), a


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_in_sweep_production_equals_the_record_fed_sweep(dp, k):
    """At most four bikes: the record-free wavefront sweep (tu_bike.hip) evaluates linearize / quadraticize inside the sweep
    where the record-fed padded sweep reads the tile producer's records.  Same expressions, same orders: the gains bit for bit,
    with per-agent Q / R / Q_f, per-item radius and mu, n_dims 2 and 3 mixed, near and far pairs; a 37-item batch (one
    wavefront per SIMD) and the same items as the first 37 of 1300 (two per SIMD)."""
    from dpilqr_amd.device import to_dev
    ns, nc, T, Bbig = 5, 2, 14, 1300
    rng = np.random.default_rng(950 + k)
    xf = rng.normal(size=(Bbig, ns * k)); x0 = rng.normal(size=(Bbig, ns * k)) * 0.7
    x0[:, 0::ns] += 0.8 * np.arange(k)
    x0[:, 3::ns] = rng.uniform(-3, 3, size=(Bbig, k))          # headings
    x0[:, 4::ns] = rng.uniform(-1, 1, size=(Bbig, k))          # steering angles
    U0 = rng.normal(size=(Bbig, T, nc * k)) * 0.2
    Q = np.stack([np.diag(rng.uniform(0.5, 2.0, ns)) + 0.05 * rng.normal(size=(ns, ns)) for _ in range(k)])
    R = np.stack([np.diag(rng.uniform(0.5, 2.0, nc)) + 0.05 * rng.normal(size=(nc, nc)) for _ in range(k)])
    Qf = np.stack([30.0 * np.eye(ns) + rng.normal(size=(ns, ns)) for _ in range(k)])
    n_dims = [3 if a % 2 == 0 else 2 for a in range(k)]
    rad = rng.uniform(0.4, 1.5, size=Bbig); mu_h = rng.choice([0.0, 0.125, 1.0], size=Bbig)
    out = {}
    for B in (37, Bbig):
        pb = dp.ProblemBatch([10] * k, n_dims, xf[:B], Q, R, Qf, rad[:B], 0.1, T)
        X, _ = pb.rollout(x0[:B], U0[:B])
        mu = to_dev(mu_h[:B])
        Kf, df = pb.backward_pass_fused(X, U0[:B], mu)
        Kr, dr = pb.backward_pass(X, U0[:B], mu)
        assert bool(torch.isfinite(Kf).all()) and float(Kf.abs().max()) > 0
        assert torch.equal(Kf, Kr) and torch.equal(df, dr), B
        out[B] = (Kf, df)
    assert torch.equal(out[Bbig][0][:37], out[37][0]) and torch.equal(out[Bbig][1][:37], out[37][1])


def test_fused_pass_is_not_served_beyond_four_bikes(dp):
    from dpilqr_amd import _lib
    from dpilqr_amd.device import to_dev
    k, T, B = 5, 6, 3
    rng = np.random.default_rng(3)
    pb = dp.ProblemBatch([10] * k, [2] * k, rng.normal(size=(B, 5 * k)), np.eye(5), np.eye(2), np.eye(5), 0.5, 0.1, T)
    X, _ = pb.rollout(rng.normal(size=(B, 5 * k)), np.zeros((B, T, 2 * k)))
    with pytest.raises(_lib.DpilqrError) as e:
        pb.backward_pass_fused(X, np.zeros((B, T, 2 * k)), to_dev(np.zeros(B)))
    assert e.value.code == _lib.EUNSUPPORTED


def check_solve(r, i, z, pre):
    nb = len(z[pre + "mu_trace"])
    assert int(r["n_bwd"][i]) == nb, "number of backward passes differs"
    tr = r["trace"][i].cpu().numpy()[:nb]
    np.testing.assert_array_equal(tr[:, 0], z[pre + "mu_trace"])
    np.testing.assert_array_equal(tr[:, 1].astype(int), z[pre + "acc_trace"])     # decision trace
    np.testing.assert_array_equal(tr[:, 4].astype(int), z[pre + "nfwd_trace"])
    assert int(r["n_fwd"][i]) == int(z[pre + "nfwd_trace"].sum())
    assert relerr(tr[:, 2], z[pre + "Jlast_trace"]) < TOL_SOLVE
    assert relerr(r["X"][i].cpu().numpy(), z[pre + "X"]) < TOL_SOLVE
    assert relerr(r["U"][i].cpu().numpy(), z[pre + "U"]) < TOL_SOLVE
    assert abs(r["J"][i].item() - z[pre + "J"]) < TOL_SOLVE * abs(z[pre + "J"])


def _tags(z, k):
    return [str(t) for t in z["tags"] if str(t).startswith(f"k{k}_")]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6])
def test_solver_solve(dp, golden, k):
    """ilqrSolver.solve of bike problems runs on the device and reproduces the reference's solves (G11 (c)): trajectory, cost,
    number of backward passes."""
    z = golden("g11_bike_solves")
    for tag in _tags(z, k):
        pre = tag + "_"
        s = dp.ilqrSolver(bike_problem(dp, z, pre), int(z[pre + "T"]))
        assert s.on_device
        X, U, J = s.solve(z[pre + "x0"].reshape(1, -1), z[pre + "U0"], verbose=False)
        assert relerr(X, z[pre + "X"]) < TOL_SOLVE and relerr(U, z[pre + "U"]) < TOL_SOLVE, tag
        assert abs(J - z[pre + "J"]) < TOL_SOLVE * abs(J), tag
        assert s.n_bwd == len(z[pre + "mu_trace"]), tag


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6])
def test_batch_solve(dp, golden, k):
    """The same solves as many-item batches (every golden seed of k, each repeated to 1300 items: two wavefronts per SIMD in
    the sweeps), with the decision trace; every copy of an item equal to its first copy bit for bit."""
    z = golden("g11_bike_solves")
    tags = _tags(z, k)
    reps = 1300 // len(tags)
    x0 = np.concatenate([np.tile(z[t + "_x0"], (reps, 1)) for t in tags])
    xf = np.concatenate([np.tile(z[t + "_xf"], (reps, 1)) for t in tags])
    U0 = np.concatenate([np.tile(z[t + "_U0"], (reps, 1, 1)) for t in tags])
    pb = bike_batch(dp, z, tags[0] + "_", xf=xf)
    r = pb.solve(x0, U0, trace=True)
    for j, tag in enumerate(tags):
        i0 = j * reps
        check_solve(r, i0, z, tag + "_")
        sl = slice(i0, i0 + reps)
        for key in ("X", "U", "J", "n_bwd", "trace"):
            v = r[key][sl]
            assert torch.equal(v, v[:1].expand_as(v)) if key != "trace" else torch.equal(torch.nan_to_num(v), torch.nan_to_num(v[:1]).expand_as(v)), (tag, key)


def test_solve_distributed(dp, golden):
    """solve_distributed on six bikes (G11 (d)): the interaction graph, the per-cluster device solves, the merged result."""
    z = golden("g11_bike_dispatch")
    prob = bike_problem(dp, z)
    Xd, Ud, Jf, info = dp.solve_distributed(prob, z["x0"].reshape(1, -1), z["U0"], 0.5, ignore_ids=[], verbose=False)
    assert relerr(Xd, z["X_dec"]) < TOL_SOLVE and relerr(Ud, z["U_dec"]) < TOL_SOLVE
    assert abs(Jf - z["J_full"]) < TOL_SOLVE * abs(Jf) and set(info) == set(prob.ids)


def test_what_the_family_does_not_serve(dp):
    """Thirteen or more bikes (n_x > 60: the large-cluster path has no five-state instantiation) and the fp32 arm: a clean
    DpilqrError, no launch."""
    from dpilqr_amd import _lib
    rng = np.random.default_rng(13)
    k, T, B = 13, 5, 2
    pb = dp.ProblemBatch([10] * k, [2] * k, rng.normal(size=(B, 5 * k)), np.eye(5), np.eye(2), np.eye(5), 0.5, 0.1, T)
    with pytest.raises(_lib.DpilqrError) as e:
        pb.rollout(rng.normal(size=(B, 5 * k)), np.zeros((B, T, 2 * k)))
    assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(_lib.DpilqrError) as e:
        pb.solve(rng.normal(size=(B, 5 * k)), np.zeros((B, T, 2 * k)))
    assert e.value.code == _lib.EUNSUPPORTED
    k = 3
    pb = dp.ProblemBatch([10] * k, [2] * k, rng.normal(size=(B, 5 * k)), np.eye(5), np.eye(2), np.eye(5), 0.5, 0.1, T)
    with pytest.raises(_lib.DpilqrError) as e:
        pb.solve(rng.normal(size=(B, 5 * k)), np.zeros((B, T, 2 * k)), dtype=torch.float32)
    assert e.value.code == _lib.EUNSUPPORTED
    # the library is still usable afterwards
    X, J = pb.rollout(rng.normal(size=(B, 5 * k)), np.zeros((B, T, 2 * k)))
    assert bool(torch.isfinite(X).all())
