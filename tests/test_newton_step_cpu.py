"""Damped Newton step and LM update without a GPU: the numpy branch of the step against a longdouble Cholesky solve
(the a-priori bound of newton_cases.py, without the store-rounding term: the branch returns float64), the argument
checks of the two C entries, and the logic of perband.retrieve_bands' loop with an injected step on a quadratic
problem."""
import ctypes
import os
import re

import numpy as np
import pytest

import newton_cases as nc
from conftest import ROOT

from gp_emulator_amd import _lib, perband

GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4
NEW_SYMBOLS = ("gp_newton_step_device", "gp_lm_update_device")


# ---- the numpy branch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("full_rank", [True, False])
@pytest.mark.parametrize("D", nc.DIMS)
def test_numpy_branch_within_the_residual_bound(D, full_rank, dtype):
    """|A' step + g'| within the bound for the seeded matrices of the GPU test (inputs of either dtype, arithmetic
    and result in float64), both damping modes, every lambda, with and without a prior; no row fails, in the
    branch or in the longdouble factorisation."""
    worst = 0.0
    for prior in (False, True):
        case = nc.seeded(D, 65, full_rank, dtype, prior=prior)
        for damping in ("diagonal", "identity"):
            for lam in nc.LAMBDAS:
                step, trial, status = _lib.newton_step_numpy(case["x"], case["grad"], case["A"], lam, damping, case["prior"])
                assert step.dtype == trial.dtype == np.float64 and status.dtype == np.int32
                prep = nc.prepare(case, lam, damping)
                res, bound = nc.residual_and_bound(case, prep, step, stored_f32=False)
                assert prep[3].all() and not status.any(), (prior, damping, lam)
                assert np.all(res <= bound), (prior, damping, lam, float(np.max(res / bound)))
                worst = max(worst, float(np.max(res / np.maximum(bound, nc.LD(1e-300)))))
                assert np.array_equal(trial, case["x"].astype(np.float64) + step)
    print("D = %d, E = %d, %s: worst residual / bound %.3g" % (D, nc.n_terms(D, full_rank), np.dtype(dtype).name, worst))


def test_numpy_branch_agrees_with_numpy_solve_and_clamps():
    case = nc.seeded(11, 40, True, np.float64, prior=True, bounds=True)
    lam = np.linspace(0.1, 2.0, 40)
    step, trial, status = _lib.newton_step_numpy(case["x"], case["grad"], case["A"], lam, "diagonal", case["prior"], case["bounds"])
    x0, P = case["prior"]
    A = case["A"] + P
    idx = np.arange(11)
    A[:, idx, idx] *= 1.0 + lam[:, None]
    g = case["grad"] + (case["x"] - x0) @ P.T
    ref = -np.linalg.solve(A, g[:, :, None])[:, :, 0]
    assert np.max(np.abs(step - ref)) <= 1e-8 * np.max(np.abs(ref))
    lo, hi = case["bounds"]
    assert np.array_equal(trial, np.clip(case["x"] + step, lo, hi))
    assert np.any(trial == lo) and np.any(trial == hi) and not status.any()
    # the upper triangle is never read
    broken = case["A"].copy()
    broken[:, np.triu_indices(11, 1)[0], np.triu_indices(11, 1)[1]] = np.nan
    again = _lib.newton_step_numpy(case["x"], case["grad"], broken, lam, "diagonal", case["prior"], case["bounds"])
    assert all(np.array_equal(a, b) for a, b in zip(again, (step, trial, status)))


def test_numpy_branch_reports_the_failed_pivot():
    D, M = 7, 9
    case = nc.seeded(D, M, True, np.float64)
    A, k_bad = case["A"].copy(), {2: 0, 4: 3, 7: 6}            # row -> pivot
    for m, k in k_bad.items():
        A[m, k:, :] = 0.0
        A[m, :, k:] = 0.0
        A[m, k, k] = -1.0
    step, trial, status = _lib.newton_step_numpy(case["x"], case["grad"], A, 1.0, "identity")
    good = _lib.newton_step_numpy(case["x"], case["grad"], case["A"], 1.0, "identity")
    for m in range(M):
        if m in k_bad:
            assert status[m] == k_bad[m] + 1 and not step[m].any() and np.array_equal(trial[m], case["x"][m])
        else:
            assert status[m] == 0 and np.array_equal(step[m], good[0][m]) and np.array_equal(trial[m], good[1][m])
    with pytest.raises(ValueError):
        _lib.newton_step_numpy(case["x"], case["grad"], A, 1.0, "marquardt")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", nc.DIMS)
def test_numpy_branch_carries_a_nan_through_the_clamp(D, dtype):
    """newton_cases.check_nan_into_the_clamp, both damping modes, without and with prior + bounds: a NaN gradient or
    state under a sound matrix gives status 0 and a NaN trial, as the kernel does."""
    for extras in (False, True):
        case = nc.seeded(D, 65, True, dtype, prior=extras, bounds=extras)
        lam = np.array(nc.LAMBDAS, dtype)[np.arange(65) % 3]
        for damping in ("diagonal", "identity"):
            nc.check_nan_into_the_clamp(lambda c: _lib.newton_step_numpy(c["x"], c["grad"], c["A"], lam, damping, c["prior"],
                                                                          c["bounds"]), case)


# ---- the C entries ---------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in gp_predict_hip.h" % name
        assert hasattr(lib, name), "libgp_predict_hip.so does not export %s" % name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(args) == len(m.group(1).split(","))
    assert re.search(r"#define\s+GP_DAMP_DIAGONAL\s+0\b", text) and re.search(r"#define\s+GP_DAMP_IDENTITY\s+1\b", text)
    assert (_lib.GP_DAMP_DIAGONAL, _lib.GP_DAMP_IDENTITY) == (0, 1)
    for name in ("newton_step_device", "lm_update_device", "newton_step"):
        assert hasattr(_lib.Context, name)


def newton_args(**kw):
    """Arguments of gp_newton_step_device that pass every check; ``x`` stands for any non-null pointer."""
    x = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    a = dict(ctx=x, dtype=_lib.GP_F64, d_x=x, d_grad=x, d_A=x, d_lambda=x, damping=0, d_prior_mean=None, d_prior_prec=None,
             d_lo=None, d_hi=None, d_step=x, d_trial=x, d_status=x, n_rows=1, n_inputs=3)
    for k, v in kw.items():
        a[k] = x if v == "set" else v
    return list(a.values())


def update_args(**kw):
    x = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    a = dict(ctx=x, dtype=_lib.GP_F64, d_x=x, d_trial=x, d_cost=x, d_cost_trial=x, d_grad=x, d_grad_trial=x, d_A=x,
             d_A_trial=x, d_lambda=x, d_status=x, d_state=x, d_accepted=None, d_prior_mean=None, d_prior_prec=None,
             down=1 / 3.0, up=4.0, lambda_min=1e-12, lambda_max=1e12, ftol=1e-10, xtol=0.0, n_rows=1, n_inputs=3)
    for k, v in kw.items():
        a[k] = x if v == "set" else v
    return list(a.values())


# The checks run before the context is used, so a stand-in for it reaches the later ones without a GPU; no case
# here passes them all.
ARGUMENT_CASES = [
    ("gp_newton_step_device", newton_args(ctx=None), GP_ERR_INVALID, "null context"),
    ("gp_newton_step_device", [None, _lib.GP_F64] + [None] * 4 + [0] + [None] * 7 + [1, 1], GP_ERR_INVALID, "null context"),
    ("gp_newton_step_device", newton_args(d_A=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_newton_step_device", newton_args(d_status=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_newton_step_device", newton_args(d_step=None, d_trial=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_newton_step_device", newton_args(dtype=7), GP_ERR_INVALID, "bad dtype 7"),
    ("gp_newton_step_device", newton_args(n_rows=0), GP_ERR_INVALID, "bad sizes"),
    ("gp_newton_step_device", newton_args(n_inputs=0), GP_ERR_INVALID, "bad sizes"),
    ("gp_newton_step_device", newton_args(n_inputs=33), GP_ERR_UNSUPPORTED, "the Newton step kernels serve n_inputs <= 32"),
    ("gp_newton_step_device", newton_args(damping=2), GP_ERR_INVALID, "bad damping 2"),
    ("gp_newton_step_device", newton_args(d_prior_mean="set"), GP_ERR_INVALID, "prior mean and prior precision go together"),
    ("gp_newton_step_device", newton_args(d_prior_prec="set"), GP_ERR_INVALID, "prior mean and prior precision go together"),
    ("gp_newton_step_device", newton_args(d_lo="set"), GP_ERR_INVALID, "lower and upper bounds go together"),
    ("gp_newton_step_device", newton_args(d_hi="set"), GP_ERR_INVALID, "lower and upper bounds go together"),
    ("gp_lm_update_device", update_args(ctx=None), GP_ERR_INVALID, "null context"),
    ("gp_lm_update_device", [None, _lib.GP_F64] + [None] * 14 + [0.5, 2.0, 0.0, 1.0, 0.0, 0.0, 1, 1], GP_ERR_INVALID, "null context"),
    ("gp_lm_update_device", update_args(d_cost_trial=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_lm_update_device", update_args(d_state=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_lm_update_device", update_args(n_rows=-1), GP_ERR_INVALID, "bad sizes"),
    ("gp_lm_update_device", update_args(n_inputs=40), GP_ERR_UNSUPPORTED, "the Newton step kernels serve n_inputs <= 32"),
    ("gp_lm_update_device", update_args(d_grad=None), GP_ERR_INVALID,
     "grad / grad_trial and A / A_trial are given or left out as pairs"),
    ("gp_lm_update_device", update_args(d_A_trial=None), GP_ERR_INVALID,
     "grad / grad_trial and A / A_trial are given or left out as pairs"),
    ("gp_lm_update_device", update_args(d_prior_mean="set"), GP_ERR_INVALID, "prior mean and prior precision go together"),
]


@pytest.mark.parametrize("name,args,code,message", ARGUMENT_CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(ARGUMENT_CASES)])
def test_argument_errors_go_through_the_one_error_buffer(name, args, code, message):
    lib = _lib.load()
    i32, i64 = ctypes.c_int(), ctypes.c_int64()
    ref = ctypes.byref
    # a different message first (another unit's), so that a buffer of the new code's own would leave it behind
    rc = lib.gp_launch_plan(99, _lib.GP_F64, 10, 2, 1, 1, 0, 1, 0, ref(i32), ref(i64), ref(i32), ref(i64), ref(i32), ref(i32))
    assert (rc, lib.gp_last_error_string().decode()) == (GP_ERR_INVALID, "bad op 99")
    rc = getattr(lib, name)(*args)
    assert (rc, lib.gp_last_error_string().decode()) == (code, message)


# ---- the loop of retrieve_bands --------------------------------------------------------------------------
class LinearBand:
    """An 'emulator' whose mean is linear in x, so that the misfit is quadratic and Gauss-Newton exact."""

    def __init__(self, inputs, a, b):
        self.inputs, self.a, self.b = inputs, a, b

    def cpu_predict(self, X, do_unc=False):
        return X @ self.a + self.b, np.broadcast_to(self.a, X.shape).copy()

    def hessian(self, X):
        return np.zeros((X.shape[0], X.shape[1], X.shape[1]))


def toy(D=4, E=9, M=6, seed=3):
    rs = np.random.RandomState(seed)
    inputs = rs.random_sample((5, D))
    gps = [LinearBand(inputs, rs.standard_normal(D), rs.standard_normal()) for _ in range(E)]
    obs = rs.standard_normal(E)                                   # inconsistent: the minimum cost is > 0
    Amat = np.stack([g.a for g in gps])
    x_star = np.linalg.lstsq(Amat, obs - np.array([g.b for g in gps]), rcond=None)[0]
    X0 = x_star + rs.uniform(0.5, 1.0, (M, D))
    return gps, obs, x_star, X0


def cost_of(gps, obs, X):
    return perband.misfit_bands(gps, X, obs, is_gpu=False)[0]


def test_loop_rejects_accepts_clamps_and_freezes():
    """Rows 0-1 are offered uphill trials (row 1 a downhill one with a failed status): rejected, x kept, lambda times
    up per iteration up to LAMBDA_MAX.  Rows 2-3 are offered half the way to the minimum: accepted every time,
    lambda times down, down to LAMBDA_MIN.  Rows 4-5 are offered a move below xtol: accepted once, converged, and
    frozen whatever is offered afterwards."""
    gps, obs, x_star, X0 = toy()
    M, iters, up, down = X0.shape[0], 6, 4.0, 1.0 / 3.0
    calls = []

    def step_fn(x, grad, A, lam):
        calls.append((x.copy(), lam.copy()))
        trial, status = x.copy(), np.zeros(M, np.int32)
        trial[0] = x[0] + (x[0] - x_star)                  # away from the minimum
        trial[1] = x[1] + 0.5 * (x_star - x[1])            # good, but its factorisation 'failed'
        status[1] = 2
        trial[2:4] = x[2:4] + 0.5 * (x_star - x[2:4])
        trial[4:6] = x[4:6] + 1e-9 * (x_star - x[4:6]) if len(calls) == 1 else x_star     # (the minimum itself, later)
        return trial - x, trial, status

    for lam0 in (1e-10, 1e11):
        del calls[:]
        X, cost, state, n_acc, lam = perband.retrieve_bands(gps, X0, obs, lam0=lam0, max_iter=iters, down=down, up=up,
                                                            ftol=1e-30, xtol=1e-6, step_fn=step_fn)
        assert len(calls) == iters and X.dtype == np.float64 and state.dtype == n_acc.dtype == np.int32
        lam_rej = lam_acc = lam0
        for _ in range(iters):
            lam_rej, lam_acc = min(lam_rej * up, perband.LAMBDA_MAX), max(lam_acc * down, perband.LAMBDA_MIN)
        assert (lam_rej == perband.LAMBDA_MAX) == (lam0 == 1e11) and (lam_acc == perband.LAMBDA_MIN) == (lam0 == 1e-10)
        assert np.array_equal(X[:2], X0[:2]) and np.all(lam[:2] == lam_rej)
        assert np.array_equal(n_acc, [0, 0, iters, iters, 1, 1]) and np.array_equal(state, [0, 0, 0, 0, 1, 1])
        x = X0[2:4].copy()
        for _ in range(iters):
            x = x + 0.5 * (x_star - x)
        assert np.array_equal(X[2:4], x) and np.all(lam[2:4] == lam_acc)
        assert np.array_equal(X[4:6], X0[4:6] + 1e-9 * (x_star - X0[4:6])) and np.all(lam[4:6] == max(lam0 * down, perband.LAMBDA_MIN))
        assert np.array_equal(cost, cost_of(gps, obs, X)) and np.all(cost[2:] < cost_of(gps, obs, X0)[2:])
        # the step sees the rows and the damping the update left
        assert np.array_equal(calls[-1][0][:2], X0[:2]) and np.array_equal(calls[0][1], np.full(M, lam0))
        assert np.array_equal(calls[1][1][:2], np.full(2, min(lam0 * up, perband.LAMBDA_MAX)))

    # ftol: the first accepted step gains less than 0.9 F, so every accepting row converges at once
    del calls[:]
    X, cost, state, n_acc, lam = perband.retrieve_bands(gps, X0, obs, lam0=1.0, max_iter=iters, ftol=0.9, xtol=0.0,
                                                        step_fn=step_fn)
    assert np.array_equal(state, [0, 0, 1, 1, 1, 1]) and np.array_equal(n_acc, [0, 0, 1, 1, 1, 1])
    assert len(calls) == iters                             # (rows 0 and 1 never converge)
    # every row converged: looked for after each fourth iteration, and the loop ends there
    del calls[:]

    def halfway(x, grad, A, lam):
        calls.append(None)
        return 0.5 * (x_star - x), x + 0.5 * (x_star - x), np.zeros(len(x), np.int32)
    X, cost, state, n_acc, lam = perband.retrieve_bands(gps, X0[2:], obs, lam0=1.0, max_iter=11, ftol=0.9, step_fn=halfway)
    assert np.all(state == 1) and np.all(n_acc == 1) and len(calls) == 4


def test_numpy_branch_of_the_loop_finds_the_minimum():
    gps, obs, x_star, X0 = toy()
    X, cost, state, n_acc, lam = perband.retrieve_bands(gps, X0, obs, is_gpu=False, max_iter=12)
    assert np.max(np.abs(X - x_star)) <= 1e-6 and np.all(n_acc >= 1)
    assert np.all(cost <= cost_of(gps, obs, X0)) and np.array_equal(cost, cost_of(gps, obs, X))
    costs = [perband.retrieve_bands(gps, X0, obs, is_gpu=False, max_iter=k)[1] for k in range(5)]
    assert np.array_equal(costs[0], cost_of(gps, obs, X0))
    assert all(np.all(b <= a) for a, b in zip(costs, costs[1:]))
    # prior and bounds: the minimiser of the sum, clipped
    D = X0.shape[1]
    prior = (np.full(D, 0.5), 4.0 * np.eye(D))
    Xp = perband.retrieve_bands(gps, X0, obs, prior=prior, is_gpu=False, max_iter=12)[0]
    Amat, b = np.stack([g.a for g in gps]), np.array([g.b for g in gps])
    ref = np.linalg.solve(Amat.T @ Amat + prior[1], Amat.T @ (obs - b) + prior[1] @ prior[0])
    assert np.max(np.abs(Xp - ref)) <= 1e-6
    Xb = perband.retrieve_bands(gps, X0, obs, bounds=(x_star + 0.25, x_star + 2.0), is_gpu=False, max_iter=12)[0]
    assert np.all(Xb >= x_star + 0.25) and np.all(Xb <= x_star + 2.0)
    for bad in (dict(second_order=None), dict(second_order="newton")):
        with pytest.raises(ValueError):
            perband.retrieve_bands(gps, X0, obs, is_gpu=False, **bad)
    with pytest.raises(ValueError):
        perband.retrieve_bands(gps, X0[:, :2], obs, is_gpu=False)
