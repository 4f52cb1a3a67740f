#!/usr/bin/env python
"""Generate the BikeDynamics5D golden vectors (G11) from the REAL reference.

Like make_golden.py (whose reference import and problem builders it reuses) it runs the reference's own functions on seeded
inputs and stores inputs and outputs as arrays only.

  g11_bike_models.npz     f / integrate (one RK4 step of dt) / linearize at 256 seeded points, |theta| up to 1e3 rad,
                          phi in (-1.4, 1.4), dt in {0.05, 0.1, 0.5}
  g11_bike_passes_k*.npz  rollout, backward pass (K, d at the solver's mu) and the ten-alpha forward pass of k bikes with a
                          GameCost including proximity (the g3_case pattern), k = 1, 2, 3, 4, 6, 12
  g11_bike_solves.npz     whole ilqrSolver.solve runs with the decision trace, k = 1..4 and 6, a few seeds each; only seeds
                          whose trace (and the costs it compares, to 1e-6) the reference itself keeps under a 1e-12 perturbation
                          of x0
  g11_bike_dispatch.npz   one solve_distributed on a six-bike scenario

Run:  python tests/golden/make_golden_bike.py
"""
import io
import sys
from contextlib import redirect_stdout
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402  (imports the reference)

dp = mg.dp
BIKE = dp.BikeDynamics5D
mg.MODEL_ENUM[BIKE] = 10          # the library's enum value for the bike (include/dpilqr_hip.h)
OUT = mg.OUT


def g11_models():
    rng = np.random.default_rng(1101)
    n = 256
    x = np.zeros((n, 5))
    x[:, :2] = rng.normal(size=(n, 2)) * 3.0
    x[:, 2] = rng.uniform(-3.0, 3.0, size=n)
    # headings: a quarter of them large (up to 1e3 rad: the argument reduction), the rest within a few turns
    x[:, 3] = np.where(np.arange(n) % 4 == 0, rng.uniform(-1e3, 1e3, size=n), rng.uniform(-7.0, 7.0, size=n))
    x[:, 4] = rng.uniform(-1.4, 1.4, size=n)
    u = rng.normal(size=(n, 2))
    dt = np.array([0.05, 0.1, 0.5])[np.arange(n) % 3]
    f = np.zeros((n, 5)); xn = np.zeros((n, 5)); A = np.zeros((n, 5, 5)); B = np.zeros((n, 5, 2))
    for i in range(n):
        m = BIKE(float(dt[i]))
        f[i] = np.asarray(m.f(x[i].copy(), u[i].copy()), dtype=np.float64).ravel()
        xn[i] = m(x[i].copy(), u[i].copy())
        A[i], B[i] = m.linearize(x[i].copy(), u[i].copy())
    np.savez_compressed(OUT / "g11_bike_models.npz", x=x, u=u, dt=dt, f=f, xn=xn, A=A, B=B)


def bike_setup(k, seed):
    if k == 1:   # random_setup centres a single agent on the origin and divides by zero
        if seed == 0:
            return np.array([1.5, -0.7, 0.2, 0.3, 0.1]), np.array([-0.8, 1.1, 0.0, 0.0, 0.0])
        rng = np.random.default_rng(seed)
        p0, pf = rng.uniform(-2.0, 2.0, size=2), rng.uniform(-2.0, 2.0, size=2)
        return np.r_[p0, 0.2, rng.uniform(-1.0, 1.0), 0.1], np.r_[pf, 0.0, 0.0, 0.0]
    np.random.seed(seed)
    x0, xf = dp.random_setup(k, 5, is_rotation=False, rel_dist=k, var=k / 2, n_d=2, random=True, energy=10.0)
    return x0.reshape(-1), xf.reshape(-1)


def g11_passes():
    for k, T, seed in ((1, 30, 0), (2, 30, 21), (3, 30, 22), (4, 25, 23), (6, 20, 24), (12, 12, 25)):
        x0, xf = bike_setup(k, seed)
        prob, meta = mg.build_problem([BIKE] * k, x0, xf, 0.5, 0.1, [2] * k)
        U0 = mg.warm_U([BIKE] * k, T)
        s = dp.ilqrSolver(prob, T)
        x0v = meta["x0"]
        Xr, Jr = s._rollout(x0v.reshape(-1, 1), U0)
        out = dict(meta); out.update(T=np.array(T), U0=U0, X_roll=Xr, J_roll=np.array(Jr))
        # operating point: after two iLQR iterations, so that the agents interact
        X, U, _ = s.solve(x0v.copy(), U0.copy(), n_lqr_iter=2, verbose=False)
        mu = s.μ
        K, d = s._backward_pass(X, U)
        alphas = 1.1 ** (-np.arange(10, dtype=np.float32) ** 2)
        Xs, Us, Js = [], [], []
        for a in alphas:
            Xn, Un, Jn = s._forward_pass(X, U, K, d, a)
            Xs.append(Xn); Us.append(Un); Js.append(Jn)
        out.update(X=X, U=U, mu=np.array(mu), K=K, d=d, alphas=alphas.astype(np.float64),
                   X_fwd=np.array(Xs), U_fwd=np.array(Us), J_fwd=np.array(Js))
        np.savez_compressed(OUT / f"g11_bike_passes_k{k}.npz", **out)
        print(f"g11 passes k={k}: mu {mu:.3g}", flush=True)


def _trace_key(r):
    return (r["mu_trace"].tolist(), r["nfwd_trace"].tolist(), r["acc_trace"].tolist())


def g11_solves():
    out, tags = {}, []
    for k, T, seeds, want in ((1, 40, range(1, 11), 2), (2, 40, range(30, 40), 3), (3, 40, range(40, 50), 3),
                              (4, 40, range(50, 80), 3), (6, 30, range(60, 80), 2)):
        kept = 0
        for seed in seeds:
            x0, xf = bike_setup(k, seed)
            prob, meta = mg.build_problem([BIKE] * k, x0, xf, 0.5, 0.1, [2] * k)
            U0 = mg.warm_U([BIKE] * k, T)
            r = mg.traced_solve(prob, meta["x0"], U0, T)
            x0p = meta["x0"] * (1.0 + 1e-12) + 1e-12
            prob_p, _ = mg.build_problem([BIKE] * k, x0p, xf, 0.5, 0.1, [2] * k)
            rp = mg.traced_solve(prob_p, x0p, U0, T)
            # the decision trace must not move, nor the costs it compares (a line search that ends in rejected candidates can
            # keep its trace while their costs move by per cent: steering angles through tan's poles)
            same = _trace_key(r) == _trace_key(rp)
            moved = max(float(np.max(np.abs(r[key] - rp[key]) / np.maximum(np.abs(r[key]), 1e-300)))
                        for key in ("Jlast_trace", "Jstar_trace")) if same else float("inf")
            if moved > 1e-6:
                print(f"g11 solves k={k} seed {seed}: trace moves under a 1e-12 perturbation ({moved:.1e}), dropped", flush=True)
                continue
            r.pop("K_last"); r.pop("d_last")
            tag = f"k{k}_s{seed}"
            for k_, v in {**meta, **r, "U0": U0, "T": np.array(T)}.items():
                out[f"{tag}_{k_}"] = v
            tags.append(tag)
            kept += 1
            print(f"g11 solves {tag}: {len(r['mu_trace'])} backward passes, J {float(r['J']):.6g}", flush=True)
            if kept == want:
                break
        assert kept == want, (k, kept)
    out["tags"] = np.array(tags)
    np.savez_compressed(OUT / "g11_bike_solves.npz", **out)


def g11_dispatch():
    k, T, seed = 6, 40, 3
    x0, xf = bike_setup(k, seed)
    prob, meta = mg.build_problem([BIKE] * k, x0, xf, 0.5, 0.1, [2] * k)
    ids = [int(i) for i in meta["ids"]]
    U0 = mg.warm_U([BIKE] * k, T)
    X0row = meta["x0"].reshape(1, -1)
    g1 = dp.define_inter_graph_threshold(X0row, 0.5, prob.game_cost.x_dims, ids)
    with redirect_stdout(io.StringIO()):
        Xd, Ud, Jf, _ = dp.solve_distributed(prob, X0row, U0, 0.5, ignore_ids=[], verbose=False)
    out = dict(meta)
    out.update(T=np.array(T), U0=U0, adj_x0=mg.graph_to_arrays(g1, ids), X_dec=Xd, U_dec=Ud, J_full=np.array(Jf))
    np.savez_compressed(OUT / "g11_bike_dispatch.npz", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["models", "passes", "solves", "dispatch"]
    for w in which:
        print("generating g11", w, flush=True)
        {"models": g11_models, "passes": g11_passes, "solves": g11_solves, "dispatch": g11_dispatch}[w]()
    for f in sorted(OUT.glob("g11_*.npz")):
        print(f"{f.name:40s} {f.stat().st_size/1024:8.1f} KiB")
