"""BikeDynamics5D, the five-state family, without a GPU: the public names, the C ABI's model table and argument checks, the
lowering of bike problems, and the SymbolicModel host mix-in against the reference's own numbers (G11 (a))."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import dpilqr_amd as dp
from dpilqr_amd import _lib
from tests.golden_util import relerr

ROOT = Path(__file__).resolve().parent.parent


def test_public_names():
    from dpilqr_amd import BikeDynamics5D, SymbolicModel  # noqa: F401
    from dpilqr_amd.batch import MODEL_DIMS
    from dpilqr_amd.bbdynamics import MODEL_DIMS as FFI_DIMS
    from dpilqr_amd.dynamics import DEVICE_MODEL_CLASSES, is_device_model
    assert dp.Model.Bike5D.value == 10 and FFI_DIMS[dp.Model.Bike5D] == (5, 2) and MODEL_DIMS[10] == (5, 2)
    bike = dp.BikeDynamics5D(0.1, 100)
    assert (bike.n_x, bike.n_u, bike.dt, bike.id) == (5, 2, 0.1, 100) and bike.model is dp.Model.Bike5D
    assert dp.BikeDynamics5D in DEVICE_MODEL_CLASSES and is_device_model(bike)
    assert issubclass(dp.SymbolicModel, dp.DynamicalModel)


def test_package_does_not_import_sympy():
    import subprocess
    import sys
    code = "import sys, dpilqr_amd; print('sympy' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    assert out == "False"


def test_header_defines_the_model():
    h = (ROOT / "include" / "dpilqr_hip.h").read_text()
    assert re.search(r"^#define DPILQR_MODEL_BIKE_5D 10\b", h, flags=re.M)
    assert not re.search(r"^#define DPILQR_MODEL_\w+ 9\b", h, flags=re.M)      # 9 stays unassigned
    assert re.search(r"^#define DPILQR_ABI_VERSION 4\b", h, flags=re.M)


def test_model_dims():
    L = _lib.load()
    ns, nc = C.c_int32(), C.c_int32()
    assert L.dpilqr_model_dims(10, C.byref(ns), C.byref(nc)) == 0 and (ns.value, nc.value) == (5, 2)
    assert L.dpilqr_model_dims(9, C.byref(ns), C.byref(nc)) == _lib.EINVAL          # the hole below the bike
    assert L.dpilqr_model_dims(11, C.byref(ns), C.byref(nc)) == _lib.EINVAL


def _desc(k, n_s, n_c, addr):
    return _lib.BatchDesc(1, k, n_s, n_c, 10, 0, 0.1, 1.0, 200.0, addr, 0, addr, 0, addr, 0, addr, 0, addr, 0, addr, 0, addr, 0)


def test_descriptor_checks():
    """(5, 2) is a family now; what is not: other pairs, thirteen or more bikes (n_x > 60), the fp32 arm, and device pointers
    that are not aligned to their element type.  Every call here fails in the argument checks, before any launch (and the
    buffers are NULL besides)."""
    L = _lib.load()
    assert L.dpilqr_rollout(C.byref(_desc(2, 5, 3, 64)), None, None, None, None, None) == _lib.EINVAL
    assert b"(5,2)" in L.dpilqr_last_error()
    assert L.dpilqr_rollout(C.byref(_desc(2, 5, 2, 1)), None, None, None, None, None) == _lib.EINVAL
    assert b"aligned" in L.dpilqr_last_error()
    assert L.dpilqr_rollout(C.byref(_desc(2, 5, 2, 64)), None, None, None, None, None) == _lib.EINVAL    # NULL buffers
    assert L.dpilqr_rollout(C.byref(_desc(13, 5, 2, 64)), None, None, None, None, None) == _lib.EUNSUPPORTED
    assert b"12 agents" in L.dpilqr_last_error()
    assert L.dpilqr_rollout_f32(C.byref(_desc(2, 5, 2, 64)), None, None, None, None, None) == _lib.EUNSUPPORTED
    assert b"fp32" in L.dpilqr_last_error()


def _bike_problem(k=3, dt=0.1):
    ids = [100 + i for i in range(k)]
    rng = np.random.default_rng(5)
    xf = rng.normal(size=5 * k)
    dyn = dp.MultiDynamicalModel([dp.BikeDynamics5D(dt, i) for i in ids])
    refs = [dp.ReferenceCost(xf[5 * i:5 * i + 5], np.eye(5), np.eye(2), 1000.0 * np.eye(5), ids[i]) for i in range(k)]
    return dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([5] * k, 0.5, [2] * k)))


def test_bike_problems_lower():
    from dpilqr_amd import lowering
    from dpilqr_amd.batch import ProblemBatch
    prob = _bike_problem(3)
    assert lowering.is_lowerable(prob)
    d = lowering.describe(prob)
    assert d["model"].tolist() == [10, 10, 10] and d["n_dims"].tolist() == [2, 2, 2] and d["k"] == 3
    assert d["Q"].shape == (3, 5, 5) and d["R"].shape == (3, 2, 2) and d["xf"].shape == (15,)
    # the descriptor's hints: bits 0..7 = 1 + model, bits 8..15 = 1 + n_dims, bit 16 shared weights, NOT bit 17 (planar 4-state)
    w = ProblemBatch.hint_word(d["model"], d["n_dims"], d["Q"], d["R"], d["Qf"])
    assert w & 0xff == 11 and (w >> 8) & 0xff == 3 and (w >> 16) & 1 == 1 and (w >> 17) & 1 == 0
    # a bike among other families cannot be stacked (the reference's uniform-dims assumption)
    mixed = dp.ilqrProblem(dp.MultiDynamicalModel([dp.BikeDynamics5D(0.1, 1), dp.UnicycleDynamics4D(0.1, 2)]),
                           prob.game_cost)
    assert not lowering.is_lowerable(mixed)


class SympyBike(dp.SymbolicModel):
    """dynamics.py:253-278 as a user would write it against this package (sympy imported by the subclass only)."""

    def __init__(self, dt, *args, **kwargs):
        import sympy as sym
        super().__init__(5, 2, dt, *args, **kwargs)
        p_x, p_y, theta, v, phi, a, rho = sym.symbols("p_x p_y theta v phi a rho")
        x = sym.Matrix([p_x, p_y, v, theta, phi])
        u = sym.Matrix([a, rho])
        x_dot = sym.Matrix([x[2] * sym.cos(x[3]), x[2] * sym.sin(x[3]), u[0], x[2] * sym.tan(x[4]), u[1]])
        self._f = sym.lambdify((x, u), sym.Array(x_dot)[:, 0])
        self.A_num = sym.lambdify((x, u), x_dot.jacobian(x))
        self.B_num = sym.lambdify((x, u), x_dot.jacobian(u))


def test_symbolic_model_matches_the_reference(golden):
    """The reference's own BikeDynamics5D, a sympy SymbolicModel, restated as a user subclass of this package's SymbolicModel:
    f, linearize and the one-step RK4 of DynamicalModel.__call__ on G11 (a)'s points."""
    pytest.importorskip("sympy")

    z = golden("g11_bike_models")
    for i in range(0, len(z["x"]), 5):
        m = SympyBike(float(z["dt"][i]), 7)
        x, u = z["x"][i].copy(), z["u"][i].copy()
        assert relerr(np.asarray(m.f(x, u), dtype=np.float64), z["f"][i]) < 1e-12
        A, B = m.linearize(x, u)
        assert relerr(A, z["A"][i]) < 1e-12 and relerr(B, z["B"][i]) < 1e-12
        assert relerr(m(x, u), z["xn"][i]) < 1e-12
    # pickling drops the lambdified functions and rebuilds them through __init__(dt) (the reference's __getstate__ /
    # __setstate__; like there, that __init__ call also gives the copy a fresh id)
    import pickle
    m2 = pickle.loads(pickle.dumps(SympyBike(0.5, 9)))
    assert m2.dt == 0.5 and relerr(np.asarray(m2.f(z["x"][0], z["u"][0]), dtype=np.float64), z["f"][0]) < 1e-12
