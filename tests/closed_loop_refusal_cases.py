"""A pin of what the closed-loop entry points refuse, and with which words: a CPU-only grid of bad and boundary argument sets
for the eight ProblemBatch methods (policy_rollout, _large, _dec, _dec_team; policy_advance, _large, _dec, _dec_team), for
solve_rhc_closed_loop and for the eight C entries of include/dpilqr_policy.h.

Every case is (id, outcome); an outcome is ["ok", a validator's return value], ["raise", exception type, message] or
["rc", return code, dpilqr_last_error's text].  Run as a program (`python -m tests.closed_loop_refusal_cases`) the module writes
tests/golden/closed_loop_refusals.json; tests/test_closed_loop_refusals_host.py replays the grid against that file.

Nothing here reaches a device.  The Python cases run on a batch object made with ProblemBatch.__new__ (no device state) and host
arrays: a refusal is raised before the first device call, an acceptance is asked of the validator, which makes none.  The C cases
use an EMPTY batch (B = 0) and fake pointers: every check of the arguments is made whatever B is, and an entry that accepts its
arguments returns before any HIP call -- so a refusal that went missing would show as DPILQR_OK, never as a launch on pointers
that do not exist."""
import ctypes as C
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "closed_loop_refusals.json"
P = 1 << 20      # a fake device pointer: non-null, aligned; never dereferenced
B, T, S, L = 2, 3, 4, 5      # items, horizon, samples per item (scenarios of a loop's state), capacity

# method -> (kind, neighbourhood gains?, the (k, n_s, n_c) its bad-argument cases are made at)
METHODS = {"policy_rollout": ("rollout", False, (3, 4, 2)), "policy_rollout_large": ("rollout", False, (16, 4, 2)),
           "policy_rollout_dec": ("rollout", True, (3, 4, 2)), "policy_rollout_dec_team": ("rollout", True, (21, 4, 2)),
           "policy_advance": ("advance", False, (3, 4, 2)), "policy_advance_large": ("advance", False, (16, 4, 2)),
           "policy_advance_dec": ("advance", True, (3, 4, 2)), "policy_advance_dec_team": ("advance", True, (21, 4, 2))}
VALIDATORS = {"policy_rollout": "_policy_shapes", "policy_rollout_large": "_policy_large_shapes",
              "policy_rollout_dec": "_policy_dec_shapes", "policy_rollout_dec_team": "_policy_dec_team_shapes"}
# both sides of every size limit: n_x 60 | 63 .. 66 (61 is no multiple of a family's n_s), n_x 240 | 244, 246, 252, k 20 | 21,
# k 64 | 65, twelve | thirteen bikes -- and the families a route does not serve at a size it would
SIZES = [(1, 4, 2), (15, 4, 2), (16, 4, 2), (20, 4, 2), (21, 4, 2), (60, 4, 2), (61, 4, 2), (64, 4, 2), (65, 4, 2),
         (20, 3, 2), (21, 3, 2), (64, 3, 2), (65, 3, 2), (12, 5, 2), (13, 5, 2), (20, 5, 2), (10, 6, 3), (11, 6, 3), (20, 6, 3),
         (21, 6, 3), (40, 6, 3), (41, 6, 3), (5, 12, 4), (6, 12, 4), (20, 12, 4), (21, 12, 4), (64, 12, 4), (65, 12, 4)]


def jsonable(v):
    if isinstance(v, (tuple, list)):
        return [jsonable(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


def outcome(fn):
    try:
        return ["ok", jsonable(fn())]
    except Exception as e:      # noqa: BLE001 -- the type is part of what is pinned
        return ["raise", type(e).__name__, str(e)]


# ---------------------------------------------------------------------------------------------- the Python wrappers
def bare_batch(k, ns, nc):
    from dpilqr_amd.batch import ProblemBatch
    pb = ProblemBatch.__new__(ProblemBatch)      # no device state at all
    pb.B, pb.T, pb.k, pb.n_s, pb.n_c, pb.n_x, pb.n_u = B, T, k, ns, nc, k * ns, k * nc
    return pb


def own_bits(k):
    return (np.uint64(1) << np.arange(k, dtype=np.uint64))[None].repeat(B, axis=0)


def host_state(k, ns, nc, S=S, L=L, **over):
    import torch
    n, m, f64 = k * ns, k * nc, torch.float64
    st = dict(x_cur=torch.zeros((S, n), dtype=f64), n_done=torch.zeros((S,), dtype=torch.int32), X_exec=torch.zeros((S, L + 1, n), dtype=f64),
              U_exec=torch.zeros((S, L, m), dtype=f64), J_exec=torch.zeros((S,), dtype=f64), min_sep=torch.zeros((S,), dtype=f64),
              dist_left=torch.zeros((S, k), dtype=f64), U_next=torch.zeros((S, T, m), dtype=f64), X_next=torch.zeros((S, T + 1, n), dtype=f64))
    st.update(over)
    return st


def good_args(name, k, ns, nc, kc_max=1):
    """Arguments the method accepts at a shape it serves."""
    kind, dec, _ = METHODS[name]
    n, m = k * ns, k * nc
    a = dict(X=np.zeros((B, T + 1, n)), U=np.zeros((B, T, m)), W=None, u_lim=None, masks_checked=None)
    a["K"] = np.zeros((B, T, k, nc, kc_max * ns)) if dec else np.zeros((B, T, m, n))
    a["bits"] = own_bits(k) if dec else None
    if kind == "rollout":
        a["x0s"] = np.zeros((B, S, n))
    else:
        a.update(h=2, state=host_state(k, ns, nc), scen=None, n_d=2)
    return a


def call_public(pb, name, a):
    kind, dec, _ = METHODS[name]
    f = getattr(pb, name)
    if kind == "rollout":
        if dec:
            return f(a["X"], a["U"], a["K"], a["bits"], a["x0s"], W=a["W"], u_lim=a["u_lim"], masks_checked=a["masks_checked"])
        return f(a["X"], a["U"], a["K"], a["x0s"], W=a["W"], u_lim=a["u_lim"])
    if dec:
        return f(a["X"], a["U"], a["K"], a["bits"], a["h"], a["state"], scen=a["scen"], W=a["W"], u_lim=a["u_lim"], n_d=a["n_d"],
                 masks_checked=a["masks_checked"])
    return f(a["X"], a["U"], a["K"], a["h"], a["state"], scen=a["scen"], W=a["W"], u_lim=a["u_lim"], n_d=a["n_d"])


def call_validator(pb, name, a, **kw):
    """The method's host-side validator, by the private name and positional signature the host tests use."""
    kind, dec, _ = METHODS[name]
    n, m = pb.n_x, pb.n_u
    if kind == "rollout":
        f = getattr(pb, VALIDATORS[name])
        if dec:
            return f(a["X"], a["U"], a["K"], a["bits"], a["x0s"], a["W"], a["u_lim"], **kw)
        return f(a["X"], a["U"], a["K"], a["x0s"], a["W"], a["u_lim"])
    if dec:
        others = (("U_ff", a["U"], (B, T, m)),) + ((("nbr_bits", a["bits"], (B, pb.k)),) if a["K"] is not None else ())
    else:
        others = (("U", a["U"], (B, T, m)), ("K", a["K"], (B, T, m, n)))
    route = dict(large=True) if name.endswith("_large") else dict(team=True) if name.endswith("_team") else {}
    return pb._advance_shapes(name, a["X"], a["h"], a["state"], a["scen"], a["W"], a["u_lim"], a["n_d"], others, **route)


def bad_arguments(name):
    """(label, overrides of good_args) of one method's bad argument sets, at kc_max = 2 for the neighbourhood forms."""
    import torch
    kind, dec, (k, ns, nc) = METHODS[name]
    n, m = k * ns, k * nc
    g = good_args(name, k, ns, nc, kc_max=2)
    bad = [("X-short", dict(X=g["X"][:, :T])), ("X-items", dict(X=np.zeros((B + 1, T + 1, n)))), ("X-tensor", dict(X=torch.zeros((B, T + 1, n + 1)))),
           ("U-narrow", dict(U=g["U"][:, :, :m - 1])), ("U-steps", dict(U=np.zeros((B, T + 1, m)))),
           ("W-shape", dict(W=np.zeros((B, S, T + 1, n)))), ("W-tensor", dict(W=torch.zeros((S, L, n + 1)))),
           ("u_lim-transposed", dict(u_lim=np.zeros((m, 2)))), ("u_lim-crossed", dict(u_lim=np.array([[1.0] * m, [-1.0] * m]))),
           ("u_lim-one-crossed", dict(u_lim=np.array([[0.0] * m, [1.0] * (m - 1) + [-1e-9]])))]
    if dec:
        bad += [("Kc-dense", dict(K=np.zeros((B, T, m, n)))), ("Kc-ragged", dict(K=np.zeros((B, T, k, nc, 2 * ns + 1)))),
                ("Kc-beyond-k", dict(K=np.zeros((B, T, k, nc, (k + 1) * ns)))), ("Kc-empty", dict(K=np.zeros((B, T, k, nc, 0)))),
                ("Kc-items", dict(K=np.zeros((B + 1, T, k, nc, 2 * ns)))), ("Kc-tensor", dict(K=torch.zeros((B, T, k, nc + 1, 2 * ns)))),
                ("bits-narrow", dict(bits=g["bits"][:, :k - 1])), ("bits-float", dict(bits=g["bits"].astype(np.float64))),
                ("bits-no-own", dict(bits=g["bits"] ^ np.uint64(1))), ("bits-four-members", dict(bits=g["bits"] | np.uint64(7))),
                ("bits-no-own-int64", dict(bits=(g["bits"] ^ np.uint64(2)).view(np.int64)))]
    else:
        bad += [("K-transposed", dict(K=np.zeros((B, T, n, m)))), ("K-steps", dict(K=np.zeros((B, T + 1, m, n))))]
    if kind == "rollout":
        bad += [("x0s-2d", dict(x0s=np.zeros((B, n)))), ("x0s-no-sample", dict(x0s=np.zeros((B, 0, n)))), ("x0s-width", dict(x0s=np.zeros((B, S, n + 1)))),
                ("x0s-items", dict(x0s=np.zeros((B + 1, S, n)))), ("x0s-tensor", dict(x0s=torch.zeros((B, S, n - 1)))),
                ("W-samples", dict(W=np.zeros((B, S + 1, T, n))))]
        return bad
    st = lambda **kw: host_state(k, ns, nc, **kw)
    f64 = torch.float64

    class Fields:      # a state given as an object: its fields are read with getattr
        pass

    partial = Fields()
    for f, t in st().items():
        if f != "J_exec":
            setattr(partial, f, t)
    bad += [("h-zero", dict(h=0)), ("h-beyond-T", dict(h=T + 1)), ("h-fraction", dict(h=1.5)), ("h-negative", dict(h=-1)),
            ("n_d-zero", dict(n_d=0)), ("n_d-beyond", dict(n_d=ns + 1)), ("n_d-fraction", dict(n_d=1.5)),
            ("state-empty", dict(state={})), ("state-no-U_next", dict(state={f: t for f, t in st().items() if f != "U_next"})),
            ("state-numpy-field", dict(state=st(min_sep=np.zeros(S)))), ("state-object-lacks-J_exec", dict(state=partial)),
            ("state-too-few", dict(state=st(S=1))), ("state-x_cur-1d", dict(state=st(x_cur=torch.zeros((n,), dtype=f64)))),
            ("state-x_cur-width", dict(state=st(x_cur=torch.zeros((S, n + 1), dtype=f64)))),
            ("state-L-zero", dict(state=st(L=0))), ("state-U_exec-2d", dict(state=st(U_exec=torch.zeros((S, m), dtype=f64)))),
            ("state-n_done-int64", dict(state=st(n_done=torch.zeros((S,), dtype=torch.int64)))),
            ("state-n_done-shape", dict(state=st(n_done=torch.zeros((S, 1), dtype=torch.int32)))),
            ("state-X_exec-short", dict(state=st(X_exec=torch.zeros((S, L, n), dtype=f64)))),
            ("state-U_exec-width", dict(state=st(U_exec=torch.zeros((S, L, m + 1), dtype=f64)))),
            ("state-J_exec-shape", dict(state=st(J_exec=torch.zeros((S + 1,), dtype=f64)))),
            ("state-min_sep-float32", dict(state=st(min_sep=torch.zeros((S,), dtype=torch.float32)))),
            ("state-dist_left-width", dict(state=st(dist_left=torch.zeros((S, k + 1), dtype=f64)))),
            ("state-U_next-steps", dict(state=st(U_next=torch.zeros((S, T + 1, m), dtype=f64)))),
            ("state-X_next-strided", dict(state=st(X_next=torch.zeros((S, n, T + 1), dtype=f64).transpose(1, 2)))),
            ("state-x_cur-strided", dict(state=st(x_cur=torch.zeros((n, S), dtype=f64).t()))),
            ("scen-short", dict(scen=[0])), ("scen-beyond-S", dict(scen=[0, S])), ("scen-negative", dict(scen=[-1, 0])),
            ("scen-repeated", dict(scen=[1, 1])), ("scen-float", dict(scen=np.array([0.0, 1.0]))),
            ("scen-float-tensor", dict(scen=torch.tensor([0.0, 1.0]))), ("scen-tensor-shape", dict(scen=torch.zeros((B, 1), dtype=torch.int32))),
            ("W-capacity", dict(W=np.zeros((S, L + 1, n)))), ("W-scenarios", dict(W=np.zeros((B, L, n))))]
    bad = [c for c in bad if c[0] != "W-shape"]      # (that one is the rollouts' layout)
    if dec:
        bad += [("gains-without-masks", dict(bits=None)), ("open-loop-h-beyond-T", dict(K=None, bits=None, h=T + 1)),
                ("open-loop-U-narrow", dict(K=None, bits=None, U=g["U"][:, :, :m - 1]))]
    else:
        bad += [("open-loop-h-beyond-T", dict(K=None, h=T + 1))]
    return bad


def python_cases():
    for name, (kind, dec, home) in METHODS.items():
        pb = bare_batch(*home)
        g = good_args(name, *home, kc_max=2)
        yield f"py/{name}/good", outcome(lambda: call_validator(pb, name, g))
        for label, over in bad_arguments(name):
            a = dict(g); a.update(over)
            yield f"py/{name}/{label}", outcome(lambda: call_public(pb, name, a))
            if not (kind == "advance" and dec and label.startswith(("Kc-", "bits-", "gains-"))):      # (checked outside _advance_shapes)
                yield f"py/{name}/{label}/validator", outcome(lambda: call_validator(pb, name, a))
        if dec and kind == "rollout":      # a trusted call reads no mask: these are never looked at
            a = dict(g); a["bits"] = g["bits"] ^ np.uint64(1)
            yield f"py/{name}/trusted-masks-unread", outcome(lambda: call_validator(pb, name, a, check_masks=False))
        if kind == "advance":
            lim = np.array([[-1.0] * pb.n_u, [1.0] * pb.n_u])
            a = dict(g); a.update(scen=[3, 1], W=np.zeros((S, L, pb.n_x)), u_lim=lim, h=T, n_d=home[1])
            yield f"py/{name}/good-all-optional", outcome(lambda: call_validator(pb, name, a))
        for k, ns, nc in SIZES:
            pb = bare_batch(k, ns, nc)
            a = good_args(name, k, ns, nc)
            v = outcome(lambda: call_validator(pb, name, a))
            yield f"py/{name}/size-k{k}-{ns}x{nc}/validator", v
            if v[0] == "raise":      # an accepted size would go on to the device
                yield f"py/{name}/size-k{k}-{ns}x{nc}", outcome(lambda: call_public(pb, name, a))
                if kind == "advance":
                    a = dict(a); a["K"] = a["bits"] = None
                    yield f"py/{name}/size-k{k}-{ns}x{nc}/open-loop", outcome(lambda: call_public(pb, name, a))


# ---------------------------------------------------------------------------------------------- the loop
def problem(k, model="DoubleIntDynamics4D"):
    import dpilqr_amd as dp
    dp._reset_ids()
    cls = getattr(dp, model)
    ns, nc = cls(0.1).n_x, cls(0.1).n_u
    dyn = dp.MultiDynamicalModel([cls(0.1) for _ in range(k)])
    costs = [dp.ReferenceCost(np.zeros(ns), np.eye(ns), np.eye(nc), 100.0 * np.eye(ns), i) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([ns] * k, 0.5, [2] * k))), k * ns


def loop_cases():
    """solve_rhc_closed_loop's refusals that are raised before any device work."""
    import dpilqr_amd as dp
    D, U, Q6, BIKE, CAR = "DoubleIntDynamics4D", "UnicycleDynamics4D", "QuadcopterDynamics6D", "BikeDynamics5D", "CarDynamics3D"
    ok = dict(dist_converge=0.1, max_steps=4)
    cases = [("both-criteria", 3, D, dict(dist_converge=0.1, J_converge=1.0, max_steps=4)), ("no-criterion", 3, D, dict(max_steps=4)),
             ("team-centralized", 16, D, dict(ok, radius=1.0, team=True)), ("team-centralized-small", 3, D, dict(ok, radius=1.0, team=True)),
             ("n_x-64-default", 16, D, ok), ("n_x-64-distributed", 16, D, dict(ok, radius=1.0, centralized=False)),
             ("n_x-63-default", 21, CAR, ok), ("n_x-66-default", 11, Q6, ok), ("n_x-65-default", 13, BIKE, ok),
             ("large-distributed", 16, D, dict(ok, radius=1.0, centralized=False, large=True)),
             ("large-n_x-244", 61, D, dict(ok, large=True)), ("large-n_x-246", 41, Q6, dict(ok, large=True)),
             ("large-k-21", 21, U, dict(ok, large=True)), ("large-k-21-cars", 21, CAR, dict(ok, large=True)),
             ("large-bikes", 13, BIKE, dict(ok, large=True)), ("large-n_d", 16, D, dict(ok, large=True, n_d=5)),
             ("large-no-capacity", 16, D, dict(dist_converge=0.1, large=True)),
             ("large-step_size", 16, D, dict(ok, large=True, step_size=11)),
             ("small-distributed-no-radius", 3, D, dict(ok, centralized=False, large=True)),
             ("team-no-radius", 16, D, dict(ok, team=True, centralized=False)),
             ("team-k-65", 65, D, dict(ok, radius=1.0, team=True, centralized=False)),
             ("team-k-65-cars", 65, CAR, dict(ok, radius=1.0, team=True, centralized=False)),
             ("team-13-bikes", 13, BIKE, dict(ok, radius=1.0, team=True, centralized=False)),
             ("team-n_d", 21, D, dict(ok, radius=1.0, team=True, centralized=False, n_d=0)),
             ("W-2d", 3, D, dict(dist_converge=0.1, W=np.zeros((2, 12)))), ("W-scenarios", 3, D, dict(dist_converge=0.1, W=np.zeros((3, 4, 12)))),
             ("W-width", 3, D, dict(dist_converge=0.1, W=np.zeros((2, 4, 13)))), ("no-capacity", 3, D, dict(dist_converge=0.1)),
             ("capacity-zero", 3, D, dict(dist_converge=0.1, max_steps=0)),
             ("capacity-against-W", 3, D, dict(dist_converge=0.1, max_steps=5, W=np.zeros((2, 4, 12)))),
             ("step_size-zero", 3, D, dict(ok, step_size=0)), ("step_size-beyond-N", 3, D, dict(ok, step_size=11)),
             ("n_d-zero", 3, D, dict(ok, n_d=0)), ("n_d-beyond", 3, D, dict(ok, n_d=5))]
    for label, k, model, kw in cases:
        prob, n_x = problem(k, model)
        yield f"loop/{label}", outcome(lambda: dp.solve_rhc_closed_loop(prob, np.zeros((2, n_x)), 10, **kw))


# ---------------------------------------------------------------------------------------------- the C entries
ROLLOUT_TAIL = ("n_samples", "x0s", "W", "u_lim", "Xs", "Us", "J", "min_sep", "goal_dist")
ADVANCE_TAIL = ("h", "scen", "n_scen", "L", "n_d", "W", "u_lim", "x_cur", "n_done", "X_exec", "U_exec", "J_exec", "min_sep", "dist_left",
                "U_next", "X_next")
SCALARS = ("kc_max", "n_samples", "h", "n_scen", "L", "n_d")
INT_POINTERS = ("scen", "n_done")


def c_arguments(name):
    kind, dec, _ = METHODS[name]
    return ("X", "U", "K") + (("kc_max", "nbr_bits") if dec else ()) + (ROLLOUT_TAIL if kind == "rollout" else ADVANCE_TAIL)


def c_call(lib, name, desc, **over):
    """-> ["rc", return code, error text]: every pointer the fake one, an empty batch's scalars, `over` on top."""
    a = dict(kc_max=1, n_samples=4, h=1, n_scen=0, L=5, n_d=2)
    L = lib.load()
    args = [over.get(f, a.get(f, P)) for f in c_arguments(name)]
    rc = getattr(L, "dpilqr_" + name)(None if desc is None else C.byref(desc), *args, None)
    return ["rc", rc, L.dpilqr_last_error().decode() if rc else ""]


def empty_desc(lib, k, ns, nc, T=10):
    return lib.BatchDesc(0, k, ns, nc, T, 0, 0.1, 1.0, 200.0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0)


def c_cases(lib):
    for name, (kind, dec, home) in METHODS.items():
        d = empty_desc(lib, *home)
        yield f"c/{name}/good", c_call(lib, name, d)
        yield f"c/{name}/desc-null", c_call(lib, name, None)
        yield f"c/{name}/no-such-family", c_call(lib, name, empty_desc(lib, 3, 7, 2))
        yield f"c/{name}/no-agent", c_call(lib, name, empty_desc(lib, 0, 4, 2))
        yield f"c/{name}/no-step", c_call(lib, name, empty_desc(lib, *home, T=0))
        for f in c_arguments(name):
            if f in SCALARS:
                continue
            yield f"c/{name}/{f}-null", c_call(lib, name, d, **{f: None})
            yield f"c/{name}/{f}-misaligned", c_call(lib, name, d, **{f: P + (2 if f in INT_POINTERS else 4)})
        if dec:
            for kc in (0, -1, home[0], home[0] + 1):
                yield f"c/{name}/kc_max={kc}", c_call(lib, name, d, kc_max=kc)
        if kind == "rollout":
            scalars = [dict(n_samples=0), dict(n_samples=-3)]
        else:
            scalars = [dict(h=0), dict(h=-1), dict(h=10), dict(h=11), dict(L=0), dict(L=-2), dict(n_d=0), dict(n_d=home[1]), dict(n_d=home[1] + 1),
                       dict(n_scen=-1), dict(K=None, nbr_bits=None), dict(K=None, nbr_bits=None, kc_max=0), dict(K=None, h=0)]
        for kw in scalars:
            yield f"c/{name}/" + ",".join(f"{f}={v}" for f, v in kw.items()), c_call(lib, name, d, **kw)
        for k, ns, nc in SIZES:
            yield f"c/{name}/size-k{k}-{ns}x{nc}", c_call(lib, name, empty_desc(lib, k, ns, nc))
            yield f"c/{name}/size-k{k}-{ns}x{nc}/bad-argument", c_call(lib, name, empty_desc(lib, k, ns, nc), X=None)


def all_cases():
    import __graft_entry__ as g
    g.build(verbose=False)
    from dpilqr_amd import _lib
    out = {}
    for gen in (python_cases(), loop_cases(), c_cases(_lib)):
        for cid, v in gen:
            assert cid not in out, cid
            out[cid] = v
    return out


if __name__ == "__main__":
    cases = all_cases()
    GOLDEN.write_text(json.dumps(cases, indent=0, sort_keys=True) + "\n")
    print(f"{len(cases)} cases -> {GOLDEN}")
