"""Every rollout route (kModeRollout) and every route of the stand-alone forward pass (kModeCandidates) against the oracle, per item.

Rollouts: k_rollout_wave<MODEL, KA> (75 instantiations; every solve starts with it, dpilqr_rollout takes the same route), the
LDS-staged k_forward four items to a workgroup and one, and the large-cluster k_forward.  Candidates: ProblemBatch.forward_pass,
the public single-pass API and what ilqrSolver._forward_pass calls with ONE alpha -- the LDS-staged k_forward packed and at 128,
192 and 256 threads, the large-cluster form on the matrix pipe and OFF it (k_forward<double, NS, NC, true, false> with gains, which
no test reached before: at the solve loop's ten candidates every served size is on the pipe, with one alpha and 64 threads every
cluster with n_u > 32 is off it).  The cases, the route mirror, the reference and the bounds are tests/forward_cases.py's;
tests/test_forward_cases.py holds the cases to their conditions without a GPU.

Candidates: nominal and gains are the ORACLE's (its rollout of (x0, U0), its backward pass there at mu = 1); the GPU sweep plays no
part.  The bit-for-bit statement at alpha = 0 (Xn == X, Un == U: dx is exactly zero at every step) holds for a nominal the device
itself rolled out -- the oracle's X differs from the device's integrator in the last bit, after which dx is no longer zero -- so it
is checked in a second launch on pb.rollout's X, which also holds k_rollout_wave's compile-time model to k_forward's run-time one,
bit for bit.

Which kernel ran: derived from what launch_forward and launch_forward_big_t branch on (forward_cases.expected_route), with every
route switch of the environment required to be unset and the descriptor's model hint held to the route.

profiles/forward_checks.txt holds the FWD_RESULT lines of an MI355X run; profiles/forward_sensitivity.txt the mutants of the kernels
each of these tests is there to catch."""
import os

import numpy as np
import pytest

from tests import forward_cases as fc
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu

ROUTE_SWITCHES = ("DPILQR_FORWARD_GENERIC", "DPILQR_FORWARD_NO_PACK", "DPILQR_FORCE_BIG")
GUARD = 5
SENTINEL = -777.25


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()   # loud failure if the HIP library or the GPU is missing
    return dpilqr_amd


def _problem_batch(dp, case, b, sel=None):
    """The ProblemBatch of a case's host arrays; sel: a selection / permutation of its items."""
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    Q, R, Qf = ((pick(M) if b["per_item"] else M) for M in (b["Q"], b["R"], b["Qf"]))
    radius = float(b["radius"][0]) if case.weights == "shared" else pick(b["radius"])
    return dp.ProblemBatch(b["models"], b["n_dims"], pick(b["xf"]), Q, R, Qf, radius, b["dt"], b["T"])


def _assert_route(pb, case):
    assert not [v for v in ROUTE_SWITCHES if v in os.environ]
    assert case.expected_route() == case.route
    hint = (pb.desc.uniform_model & 0xff) - 1
    assert hint == (case.models[0] if case.uniform else -1)
    assert pb.fused_sweep == (pb.n_x > 60)
    if case.route == "wave":
        assert (hint, pb.k) in fc.RO_TABLE and case.mode == "rollout"
    elif case.mode == "rollout" and case.route in ("staged-packed", "staged"):
        assert hint < 0 or (hint, pb.k) not in fc.RO_TABLE


def _result_line(case, n, unchecked, worst, worst_bound, min_margin):
    print(f"FWD_RESULT {case.id} route={case.route} checked={n} unchecked={unchecked} worst_err={worst:.3e} its_bound={worst_bound:.3e} "
          f"min_margin={min_margin:.3g}")


class _Worst:
    """The error with the smallest margin to its bound."""

    def __init__(self):
        self.err, self.bound, self.margin = 0.0, 0.0, np.inf

    def add(self, err, bound):
        margin = bound / err if err > 0 else np.inf
        if margin < self.margin or self.bound == 0.0:
            self.err, self.bound, self.margin = err, bound, margin


@pytest.mark.parametrize("case", fc.ROLLOUT_CASES, ids=[c.id for c in fc.ROLLOUT_CASES])
def test_rollout_against_oracle(dp, case):
    r = fc.case_ref(case)
    b = r.batch
    pb = _problem_batch(dp, case, b)
    _assert_route(pb, case)
    X, J = pb.rollout(b["x0"], b["U0"])
    Xh, Jh = X.cpu().numpy(), J.cpu().numpy()
    assert np.isfinite(Xh).all() and np.isfinite(Jh).all()
    w, unchecked, bad = _Worst(), 0, []
    for i in r.idx:
        if r.bound[i] is None:
            unchecked += 1
            continue
        err = max(relerr(Xh[i], r.X[i]), fc.rel(float(Jh[i]), r.J[i]))
        w.add(err, r.bound[i])
        if not err < r.bound[i]:
            bad.append((i, err, r.bound[i]))
    _result_line(case, len(r.idx), unchecked, w.err, w.bound, w.margin)
    assert not bad, bad[:5]
    assert unchecked <= fc.MAX_UNCHECKED * len(r.idx)


def _forward(pb, r, X=None):
    Xn, Un, Jn = pb.forward_pass(r.X if X is None else X, r.U, r.K, r.d, r.alphas)
    return Xn.cpu().numpy(), Un.cpu().numpy(), Jn.cpu().numpy()


@pytest.mark.parametrize("case", fc.CANDIDATES_CASES, ids=[c.id for c in fc.CANDIDATES_CASES])
def test_candidates_against_oracle(dp, case):
    r = fc.case_ref(case)
    b = r.batch
    pb = _problem_batch(dp, case, b)
    _assert_route(pb, case)
    Xn, Un, Jn = _forward(pb, r)
    w, unchecked, bad, pairs = _Worst(), 0, [], 0
    for i in r.idx:
        for g in range(len(r.alphas)):
            Xr, Ur, Jr = r.ref(i, g)
            pairs += 1
            if not np.isfinite(Jr):      # a non-finite reference cost is non-finite on the device (and rejected: control.py:183)
                assert not np.isfinite(Jn[i, g]), (i, g, Jn[i, g])
            if r.bound[i, g] is None:
                unchecked += 1
                continue
            err = max(relerr(Xn[i, g], Xr), relerr(Un[i, g], Ur), fc.rel(float(Jn[i, g]), Jr))
            w.add(err, r.bound[i, g])
            if not err < r.bound[i, g]:
                bad.append((i, g, err, r.bound[i, g]))
    _result_line(case, pairs, unchecked, w.err, w.bound, w.margin)
    assert not bad, bad[:5]
    assert unchecked <= fc.MAX_UNCHECKED * pairs
    if r.alphas[0] == 0.0:      # alpha = 0 on a nominal the device rolled out: the nominal itself, bit for bit
        Xd, _ = pb.rollout(b["x0"], b["U0"])
        Xd = Xd.cpu().numpy()
        Xz, Uz, Jz = _forward(pb, r, Xd)
        assert np.array_equal(Xz[:, 0], Xd) and np.array_equal(Uz[:, 0], r.U)
        assert np.isfinite(Jz[:, 0]).all()


PUBLIC = [fc.by_id(s) for s in fc.PUBLIC_PATH_CASES]


@pytest.mark.parametrize("case", PUBLIC, ids=[c.id for c in PUBLIC])
def test_public_one_candidate_path(dp, case):
    """ilqrSolver._forward_pass -- ONE alpha, 64 threads -- against the oracle, on problems built from the plugin classes:
    seventeen unicycles (n_u = 34: three row tiles of sixteen controls, off the matrix pipe) and config 5's cluster (fourteen
    twelve-state quadcopters and six padded humans, n_u = 80: more controls than the launch has threads)."""
    assert case.route == "big-nopipe" and case.expected_route() == "big-nopipe" and case.alphas == "P1" and case.weights == "shared"
    r = fc.case_ref(case)
    b = r.batch
    assert not [v for v in ROUTE_SWITCHES if v in os.environ]
    cls = {0: dp.DoubleIntDynamics4D, 3: dp.UnicycleDynamics4D, 7: dp.QuadcopterDynamics12D, 8: dp.HumanDynamics6DPadded12}
    k, ns, nc = case.k, case.ns, case.nc
    for i in (0, case.B - 1):
        dyn = dp.MultiDynamicalModel([cls[m](b["dt"], a) for a, m in enumerate(case.models)])
        refs = [dp.ReferenceCost(b["xf"][i, a * ns:(a + 1) * ns], b["Q"], b["R"], b["Qf"], a) for a in range(k)]
        prob = dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([ns] * k, float(b["radius"][i]), list(b["n_dims"]))))
        s = dp.ilqrSolver(prob, b["T"])
        assert s.on_device
        Xn, Un, Jn = s._forward_pass(r.X[i], r.U[i], r.K[i], r.d[i], float(r.alphas[0]))
        pb = s._pb(b["T"])
        assert (pb.k, pb.n_x, pb.n_u, pb.B) == (k, k * ns, k * nc, 1)
        assert (pb.desc.uniform_model & 0xff) - 1 == (case.models[0] if case.uniform else -1)
        Xr, Ur, Jr = r.ref(i, 0)
        bound = r.bound[i, 0]
        assert bound is not None
        err = max(relerr(Xn, Xr), relerr(Un, Ur), fc.rel(Jn, Jr))
        print(f"FWD_RESULT public-{case.id} item={i} err={err:.3e} bound={bound:.3e}")
        assert err < bound, (i, err, bound)


SAMPLES = [fc.by_id(s) for s in fc.ROUTE_SAMPLES]


def _run(pb, case, r, sel=None):
    """The case's launch on the items `sel` of its batch: (X, J) or (Xn, Un, Jn) as host arrays."""
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    b = r.batch
    if case.mode == "rollout":
        X, J = pb.rollout(pick(b["x0"]), pick(b["U0"]))
        return X.cpu().numpy(), J.cpu().numpy()
    Xn, Un, Jn = pb.forward_pass(pick(r.X), pick(r.U), pick(r.K), pick(r.d), r.alphas)
    return Xn.cpu().numpy(), Un.cpu().numpy(), Jn.cpu().numpy()


@pytest.mark.parametrize("case", SAMPLES, ids=[c.id for c in SAMPLES])
def test_position_independence(dp, case):
    """An item's results do not depend on where in the batch it sits: results of batch[perm] == results[perm], bit for bit."""
    r = fc.case_ref(case)
    perm = np.random.default_rng(31 + case.seed).permutation(case.B)
    if np.array_equal(perm, np.arange(case.B)):
        perm = np.roll(perm, 1)
    base = _run(_problem_batch(dp, case, r.batch), case, r)
    moved = _run(_problem_batch(dp, case, r.batch, perm), case, r, perm)
    for a, c in zip(base, moved):
        assert np.array_equal(a[perm], c, equal_nan=True)


@pytest.mark.parametrize("case", SAMPLES, ids=[c.id for c in SAMPLES])
def test_guard_rows(dp, case):
    """The C entry with output buffers of B + 5 items and a descriptor of B: the five spare items' rows stay untouched, the B
    items' rows are what the API returns."""
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle, to_dev
    r = fc.case_ref(case)
    b = r.batch
    pb = _problem_batch(dp, case, b)
    lib = _lib.load()
    B, T, n, m = case.B, b["T"], pb.n_x, pb.n_u
    assert pb.desc.B == B
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
    base = _run(pb, case, r)
    if case.mode == "rollout":
        x0, U = to_dev(b["x0"]), to_dev(b["U0"])
        outs = [full(B + GUARD, T + 1, n), full(B + GUARD)]
        _lib.check(lib.dpilqr_rollout(pb._d, ptr(x0), ptr(U), ptr(outs[0]), ptr(outs[1]), stream_handle()))
    else:
        A = len(r.alphas)
        X, U, K, d, al = to_dev(r.X), to_dev(r.U), to_dev(r.K), to_dev(r.d), to_dev(np.asarray(r.alphas, dtype=np.float64))
        outs = [full(B + GUARD, A, T + 1, n), full(B + GUARD, A, T, m), full(B + GUARD, A)]
        _lib.check(lib.dpilqr_forward_pass(pb._d, ptr(X), ptr(U), ptr(K), ptr(d), ptr(al), A, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                           stream_handle()))
    torch.cuda.synchronize()
    for o, a in zip(outs, base):
        o = o.cpu().numpy()
        assert (o[B:] == SENTINEL).all()
        assert np.array_equal(o[:B], a, equal_nan=True)


POISONED = [fc.by_id(s) for s in fc.POISON_SAMPLES]


@pytest.mark.parametrize("case", POISONED, ids=[c.id for c in POISONED])
def test_poisoned_item(dp, case):
    """A NaN in x0 of an item in the middle of a wavefront (wave: 64 // k items share one) or of a workgroup (packed: four items
    share one): its neighbours are bit-identical to the clean run, its own cost is non-finite."""
    import copy
    r = fc.case_ref(case)
    per = 64 // case.k if case.route == "wave" else 4
    assert per >= 3 and case.B > per + 2
    victim = per + 1      # the second workgroup's / wavefront's second item: neighbours on both sides share its wavefront or workgroup
    pb = _problem_batch(dp, case, r.batch)
    clean = _run(pb, case, r)
    bad = copy.copy(r)
    if case.mode == "rollout":
        bad.batch = dict(r.batch); bad.batch["x0"] = r.batch["x0"].copy(); bad.batch["x0"][victim, 0] = np.nan
    else:
        bad.X = r.X.copy(); bad.X[victim, 0, 0] = np.nan
    dirty = _run(pb, case, bad)
    others = np.arange(case.B) != victim
    for a, c in zip(clean, dirty):
        assert np.array_equal(a[others], c[others], equal_nan=True)
    assert not np.isfinite(dirty[-1][victim]).any() and np.isfinite(clean[-1][victim]).all()
