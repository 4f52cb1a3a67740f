"""Child process of tests/test_gpu_cost_order.py: the library's route switches are read once per process, so every order variant
(default, DPILQR_NO_COST_ORDER, DPILQR_COST_ORDER=1 / 2 behind DPILQR_DEBUG_ROUTES=1) solves the same batches in a process of its
own and reports what it got:  python tests/cost_order_child.py OUT.json
Per shape (B, window, n_lqr_iter) of cfg2's model (k = 5, T = 50): a synchronous solve with the gains by item, and the same solve
through dpilqr_solve_enqueue split into two calls (resume = 1).  Large arrays travel as SHA-256 of their bytes plus a wrapping
int64 sum per item (to name the items that differ); the counters travel whole."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SHAPES = [(1100, 1100, 3), (3000, 2100, 3), (40, 7, 3)]


def digest(t):
    import torch
    t = t.contiguous()
    bits = t.view(torch.int64) if t.dtype == torch.float64 else t.to(torch.int64)
    per_item = bits.reshape(t.shape[0], -1).sum(1).cpu().numpy()
    return dict(sha=hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest(), per_item=[int(v) for v in per_item])


def main(out_path):
    import torch
    import dpilqr_amd as dp
    from dpilqr_amd import _lib
    from dpilqr_amd.util import random_setup_batch
    from tests.golden_util import cfg2_params
    _lib.require_gpu()
    c = cfg2_params()
    out = {}
    for B, window, n_iter in SHAPES:
        x0, xf = random_setup_batch((31000, B), 5, 4, var=2.5, n_d=2, energy=10.0)
        pb = dp.ProblemBatch(c["model"], c["n_dims"], xf.cpu().numpy(), c["Q"], c["R"], c["Qf"], c["radius"], c["dt"], c["T"])
        U0 = np.zeros((B, c["T"], 10))
        r = pb.solve(x0, U0, n_lqr_iter=n_iter, gains=True, window=window)
        res = {key: digest(r[key]) for key in ("X", "U", "J", "K", "d")}
        for key in ("status", "n_bwd", "n_fwd"):
            res[key] = r[key].cpu().numpy().tolist()
        # the same solve, enqueue only, in two calls: two iterations, then the rest of the bound
        bound = pb.iterations_bound(n_iter, window=window)
        q, state = pb.solve_enqueue(x0, U0, 2, n_lqr_iter=n_iter, window=window)
        q, state = pb.solve_enqueue(None, None, bound, state=state)
        torch.cuda.synchronize()
        res["resumed_equal"] = {key: bool(torch.equal(q[key], r[key])) for key in ("X", "U", "J", "status", "n_bwd", "n_fwd")}
        out[f"{B}/{window}/{n_iter}"] = res
    Path(out_path).write_text(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
