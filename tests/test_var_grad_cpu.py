"""The gradient of the predictive variance without a GPU: the formula against central differences of the 80-bit
variance, the numpy branch ``GaussianProcess.variance_gradient(is_gpu=False)`` against the 80-bit truth inside the
gates of ``var_grad_cases``, the A + A^T identity on a non-symmetric invQ, the launch plan's new op and the new symbols.
"""
import numpy as np
import pytest

import trained_cases as tc
import var_grad_cases as vg
from trained_cases import F32, F64, LD, N_ROWS, RECIPES, UNIT

from gp_emulator_amd import GaussianProcess, _lib


def gp_of(em):
    gp = GaussianProcess(em["inputs"], [])
    gp.theta, gp.invQ, gp.invQt = em["theta_host"], em["invQ"], em["invQt"]
    return gp


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("n,d", vg.SHAPES_CPU, ids=["%dx%d" % s for s in vg.SHAPES_CPU])
def test_numpy_branch_within_gate(n, d, recipe):
    em = tc.emulator(n, d, recipe, F64)
    t = tc.rows(em, N_ROWS)
    tr, g = vg.truth(em, t), vg.gates(em, t)
    var, dvar = gp_of(em).variance_gradient(t, is_gpu=False)
    assert var.shape == (N_ROWS,) and dvar.shape == (N_ROWS, d) and dvar.dtype == F64
    err = vg.units(dvar, tr, F64)
    err_var = tc.units(var, tc.truth(em, t), "var", F64)
    print("VAR_GRAD cpu (%d, %d) %-6s dvar %.3g u S (yardsticks a %.3g, b %.3g, gate %.3g)  var %.3g u S (gate %.3g)  "
          "median S_dvar / |dvar| %.3g" % (n, d, recipe, err, g["a"], g["b"], g["gate"], err_var, tc.gates(em, t)["var"]["gate"],
                                         float(np.median(tr["S_dvar"] / np.abs(tr["dvar"])))))
    assert g["raw"] <= tc.CAP, g
    assert err <= g["gate"], (err, g)
    assert err_var <= tc.gates(em, t)["var"]["gate"]
    # the two definitions of the variance agree: b - k^T A k and b - 1/2 sum_j W_j
    assert float(np.max(np.abs(tr["var"] - tc.truth(em, t)["var"]) / tc.truth(em, t)["S_var"])) < 1e-17


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("n,d", vg.SHAPES_CPU, ids=["%dx%d" % s for s in vg.SHAPES_CPU])
def test_formula_against_central_differences(n, d, recipe):
    """Central differences of the longdouble variance agree with the truth to 1e-8 S_dvar on the first 12 rows (near
    training points, outside the box): the formula, not a kernel.  The quotient is taken of k^T invQ k, the variance
    without its constant b (``var_grad_cases.quadratic_ld``), with step 1e-6."""
    em = tc.emulator(n, d, recipe, F64)
    t = tc.rows(em, N_ROWS)
    tr = vg.truth(em, t)
    m, h = 12, LD(1e-6)
    T = t[:m].astype(LD)
    worst = 0.0
    for q in range(d):
        step = np.zeros(d, LD)
        step[q] = h
        fd = -(vg.quadratic_ld(em, T + step) - vg.quadratic_ld(em, T - step)) / (2 * h)
        worst = max(worst, float(np.max(np.abs(fd - tr["dvar"][:m, q]) / tr["S_dvar"][:m, q])))
    print("VAR_GRAD central differences (%d, %d) %-6s %.3g S_dvar" % (n, d, recipe, worst))
    assert worst <= 1e-8


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_nonsymmetric_invq(dtype):
    """A random non-symmetric invQ (37, 3): the truth agrees with central differences of b - k^T invQ k with invQ as
    given, and the numpy branch (float64 arithmetic on the case's arrays) with the truth, inside the gate."""
    em = vg.nonsymmetric_emulator(dtype)
    assert np.max(np.abs(em["invQ"] - em["invQ"].T)) > 0.5
    t = tc.rows(em, N_ROWS)
    tr, g = vg.truth(em, t), vg.gates(em, t)
    h = LD(1e-6)
    T = t.astype(LD)
    for q in range(em["d"]):
        step = np.zeros(em["d"], LD)
        step[q] = h
        fd = -(vg.quadratic_ld(em, T + step) - vg.quadratic_ld(em, T - step)) / (2 * h)
        assert float(np.max(np.abs(fd - tr["dvar"][:, q]) / tr["S_dvar"][:, q])) <= 1e-8
    var, dvar = gp_of(em).variance_gradient(t.astype(F64), is_gpu=False)
    err = vg.units(dvar, tr, F64)
    print("VAR_GRAD cpu nonsymmetric %s numpy branch %.3g u64 S (yardsticks of the dtype: a %.3g, b %.3g)" %
          (tc.name(dtype), err, g["a"], g["b"]))
    assert g["raw"] <= tc.CAP
    assert err <= vg.MARGIN * max(vg.units(vg.difference_f64(em, t.astype(F64))[1], tr, F64), 1.0)
    assert float(np.max(np.abs(var.astype(LD) - tr["var"]) / tc.truth(em, t)["S_var"])) <= 16 * UNIT[F64]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("n,d", vg.SHAPES_GPU, ids=["%dx%d" % s for s in vg.SHAPES_GPU])
def test_every_gate_is_bounded(n, d, recipe, dtype):
    """The gates the GPU test applies, from the numpy yardsticks alone, are inside CAP before the cap is applied."""
    em = tc.emulator(n, d, recipe, dtype)
    g = vg.gates(em, tc.rows(em, N_ROWS))
    print("VAR_GRAD gate (%d, %d) %-6s %s a %.3g b %.3g gate %.3g" % (n, d, recipe, tc.name(dtype), g["a"], g["b"], g["gate"]))
    assert vg.MARGIN <= g["raw"] <= tc.CAP and g["gate"] == g["raw"]


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_launch_plan_op(prec):
    """The op of the launch plan: predict_kernel's item and grid arithmetic, whatever the call's size, and several
    items per workgroup at the row counts the GPU test's multi-round case uses."""
    assert _lib.PLAN_KERNELS[12] == "var_grad" and _lib._PLAN_OPS["var_grad"] == _lib.GP_OP_VAR_GRAD == 6
    plan = lambda rows, **kw: _lib.launch_plan("var_grad", prec, rows, n_train=250, n_inputs=10, compute_units=256, **kw)
    ref = _lib.launch_plan("predict", prec, 10 ** 6, n_train=250, n_inputs=10, compute_units=256)
    p = plan(10 ** 6)
    assert p["kernel"] == "var_grad" and p["rows_per_item"] == ref["rows_per_item"] == (128 if prec == F64 else 192)
    assert (p["items"], p["workgroups"]) == (ref["items"], ref["workgroups"]) and p["rest_items"] == 0
    r, W = p["rows_per_item"], p["workgroups"]
    q = plan(2 * W * r + 37)
    assert q["items"] == 2 * W + 1 > q["workgroups"] == W
    few = plan(53)                     # never the few-rows kernel
    assert few["kernel"] == "var_grad" and few["items"] == few["workgroups"] == 1
    assert plan(53, n_emulators=3)["items"] == 3
    for n, d in ((321, 16), (100, 17)):
        with pytest.raises(_lib.GpuPredictError, match="general-shape"):
            _lib.launch_plan("var_grad", prec, 1000, n_train=n, n_inputs=d)


def test_abi_symbols():
    lib = _lib.load()
    for name, nargs in (("gp_predict_var_grad_device", 7), ("gp_model_var_grad_bytes", 2)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    for attr in ("predict_var_grad_device", "predict_var_grad"):
        assert callable(getattr(_lib.Model, attr)) and getattr(_lib.BatchModel, attr) is getattr(_lib.Model, attr)
    from gp_emulator_amd import perband
    assert callable(perband.variance_gradient_bands)
