"""Diagnostic behind profiles/cost_order_model.txt: what predicts a fused sweep wavefront's time, and which order of the active
list (csrc/admit_order.hpp) a full cfg2 window wants.  Needs the stamp build (`python scripts/phase_stamps.py --build`, no GPU);
then, on the GPU box, `python scripts/cost_order_model.py [B] [out.txt]`.

One window of B = 6144 real cfg2 iterates (two iLQR iterations in) at the real radius:
  * predictor: per-item sweep time (in-kernel stamps) against the item's near-step count (dpilqr_cost_keys), and the key of the
    previous iterate against the current one's (staleness);
  * measured orders: the same sweep launched on the items permuted as the spread and the grouped order would list them;
  * replayed orders: the launch rebuilt offline from a per-item cost a + b key under two machine models -- a SIMD's time is the
    SUM of its wavefronts' work (issue-bound), or a wavefront's time is its OWN -- with workgroups placed on CUs greedily."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from dpilqr_amd import _lib  # noqa: E402
_lib.LIB_PATH = ROOT / "dpilqr_amd" / "variants" / "libdpilqr_stamps.so"
import dpilqr_amd as dp  # noqa: E402
from dpilqr_amd.device import empty, ptr, stream_handle, to_dev  # noqa: E402
from dpilqr_amd.util import random_setup_batch  # noqa: E402
from bench import K_AGENTS, N_U, N_X, T  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args else 6144
out_path = Path(args[1]) if len(args) > 1 else None
N_CUS, WAVES = 256, 12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


lib = _lib.load()
x0, xf = random_setup_batch((0, B), K_AGENTS, 4, var=K_AGENTS / 2, n_d=2, energy=10.0)
pb = dp.ProblemBatch([0] * K_AGENTS, [2] * K_AGENTS, xf.cpu().numpy(), np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), 0.5, 0.1, T)
U0 = np.zeros((B, T, N_U))
prev = pb.solve(x0, U0, n_lqr_iter=1)
cur = pb.solve(x0, U0, n_lqr_iter=2)


def keys_of(X):
    k = torch.zeros((B,), dtype=torch.int32, device=X.device)
    _lib.check(lib.dpilqr_cost_keys(pb._d, ptr(X), None, None, ptr(k), stream_handle()))
    torch.cuda.synchronize()
    return k.cpu().numpy().astype(np.int64)


key, key_prev = keys_of(cur["X"]), keys_of(prev["X"])
mu = to_dev(np.full(B, 0.125)); K = empty((B, T, N_U, N_X)); d = empty((B, T, N_U))
buf = torch.zeros((B * 12,), dtype=torch.int64, device="cuda")
_lib.check(lib.dpilqr_debug_stamps(ptr(buf)))


def sweep(X, U):
    """-> per-slot durations (us) and the launch's span (us), third of three launches"""
    for _ in range(3):
        _lib.check(lib.dpilqr_backward_pass_fused(pb._d, ptr(X), ptr(U), ptr(mu), ptr(K), ptr(d), None, stream_handle()))
    torch.cuda.synchronize()
    s = buf.cpu().numpy()[:4 * B].reshape(B, 4)
    return (s[:, 1] - s[:, 0]) / 100.0, (s[:, 1].max() - s[:, 0].min()) / 100.0


def listing(order):
    """list position -> item, as k_order_list would leave it (ties by item index)"""
    if not order:
        return np.arange(B)
    ranked = np.argsort(-key, kind="stable")
    pos = np.array([lib.dpilqr_order_position(r, B, N_CUS, WAVES, order) for r in range(B)])
    at = np.empty(B, dtype=np.int64)
    at[pos] = ranked
    return at


dur, span_id = sweep(cur["X"], cur["U"])
say(f"cfg2, one window of {B} items two iterations in, radius 0.5, fused sweep at {WAVES} wavefronts per workgroup, {N_CUS} CUs")
say(f"near-step key: mean {key.mean():.2f} of {T + 1} steps, {100 * (key > 0).mean():.1f} % of items have one, "
    f"{100 * key.sum() / (B * (T + 1)):.1f} % of (item, step)s are near")
say("")
say("1. predictor: per-wavefront sweep time against the near-step count")
a_fit, b_fit = np.polyfit(key, dur, 1)[::-1]
resid = dur - (a_fit + b_fit * key)
say(f"   Pearson r = {np.corrcoef(key, dur)[0, 1]:.3f};  fit  t = {a_fit:.1f} us + {b_fit:.2f} us x key;  residual sd {resid.std():.1f} us "
    f"(sd of t {dur.std():.1f} us)")
for lo, hi in ((0, 0), (1, 5), (6, 15), (16, 30), (31, T + 1)):
    m = (key >= lo) & (key <= hi)
    if m.any():
        say(f"   key {lo:2d}..{hi:2d}: {m.sum():5d} items, mean {dur[m].mean():6.1f} us, max {dur[m].max():6.1f} us")
say(f"   what the key leaves unexplained is the residual above: the co-resident wavefronts' load (a wavefront's time depends on "
    f"its SIMD's other two) and everything else, the LU pivot searches included")
say("")
say("2. staleness: the previous iterate's key against the current one's")
say(f"   Pearson r = {np.corrcoef(key_prev, key)[0, 1]:.3f}; equal for {100 * (key_prev == key).mean():.1f} % of items, "
    f"|difference| mean {np.abs(key_prev - key).mean():.2f}, max {np.abs(key_prev - key).max()}; "
    f"r(previous key, time) = {np.corrcoef(key_prev, dur)[0, 1]:.3f}")
say("")
say("3. measured: the same sweep on the items listed in each order (launch span, first start to last end)")
spans = {"as listed (arbitrary)": span_id}
stats = {"as listed (arbitrary)": dur}
for name, order in (("spread", 1), ("grouped", 2)):
    at = torch.tensor(listing(order), device="cuda")
    dd, sp = sweep(cur["X"][at].contiguous(), cur["U"][at].contiguous())
    spans[name], stats[name] = sp, dd
dd, sp = sweep(cur["X"], cur["U"])
spans["as listed, again"], stats["as listed, again"] = sp, dd
for name in spans:
    say(f"   {name:24s} span {spans[name]:7.1f} us   wavefront mean {stats[name].mean():6.1f} max {stats[name].max():6.1f} us")
say("")
say("4. replayed offline from c = a + b key (the fit above), workgroups placed on the first free CU in launch order")
cost = a_fit + b_fit * key


def replay(at, model):
    per_layer = 4 * N_CUS
    layers = -(-B // per_layer)
    rounds = -(-layers // (WAVES // 4))
    lo, extra = divmod(layers, rounds)
    free = np.zeros(N_CUS)
    for rnd in range(rounds):
        my_layers, first = lo + (1 if rnd < extra else 0), rnd * lo + min(rnd, extra)
        for cu in range(N_CUS):
            simd = np.zeros(4); own = 0.0
            for wave in range(4 * my_layers):
                slot = (first + (wave >> 2)) * per_layer + (wave & 3) * N_CUS + cu
                if slot < B:
                    c = cost[at[slot]]
                    simd[wave & 3] += c / my_layers      # three co-resident wavefronts share the SIMD's issue slots
                    own = max(own, c)
            t = simd.max() if model == "sum" else own
            i = int(np.argmin(free))
            free[i] += t
    return free.max()


for model, text in (("sum", "SIMD time = sum of its wavefronts' work"), ("own", "a wavefront's time is its own")):
    say(f"   {text}: " + ", ".join(f"{name} {replay(listing(order), model):.0f} us" for name, order in (("as listed", 0), ("spread", 1), ("grouped", 2))))
if out_path:
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
