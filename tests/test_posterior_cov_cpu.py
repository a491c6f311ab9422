"""Posterior covariance without a GPU: the numpy branch against the a-priori bound of posterior_cases.py (no free
tolerance; the branch returns float64, so the bound carries no store-rounding term), planted failed pivots, the
argument checks of the C entry, and perband.retrieve_bands(return_cov=True) on its numpy branch."""
import ctypes
import os
import re

import numpy as np
import pytest

import newton_cases as nc
import posterior_cases as pc
from conftest import ROOT

from gp_emulator_amd import _lib, perband

GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


# ---- the numpy branch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", nc.DIMS)
def test_numpy_branch_within_the_bound(D, dtype):
    """|C^ - C| and |sigma^ - sqrt(C_dd)| within the bound for the seeded matrices of the GPU test (inputs of either
    dtype, arithmetic and result in float64): full rank without and with a prior, rank deficient with a prior, 65 rows.
    No row fails, in the branch or in longdouble; cov is symmetric bit for bit; sigma^2 is its diagonal."""
    worst = [0.0, 0.0]
    idx = np.arange(D)
    for full_rank, prior in pc.KINDS:
        case = nc.seeded(D, 65, full_rank, dtype, prior=prior)
        P = case["prior"][1] if prior else None
        cov, sigma, status = _lib.posterior_cov_numpy(case["A"], P)
        assert cov.dtype == sigma.dtype == np.float64 and status.dtype == np.int32
        assert cov.shape == (65, D, D) and sigma.shape == (65, D) and status.shape == (65,)
        C, R, ok = pc.truth(case)
        assert ok.all() and not status.any(), (full_rank, prior)
        same(cov, np.ascontiguousarray(np.transpose(cov, (0, 2, 1))))
        same(sigma, np.sqrt(cov[:, idx, idx]))
        assert np.all(np.abs(sigma * sigma - cov[:, idx, idx]) <= 2.0 ** -51 * cov[:, idx, idx])   # (sqrt and the square: 3 roundings)
        ratios = pc.check(C, pc.gram(R), cov, sigma, stored_f32=False)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
    print("D = %d %s: worst error / bound cov %.3g, sigma %.3g" % (D, np.dtype(dtype).name, worst[0], worst[1]))


def test_numpy_branch_agrees_with_numpy_inv_and_never_reads_the_upper_triangle():
    case = nc.seeded(11, 40, True, np.float64, prior=True)
    P = case["prior"][1]
    cov, sigma, status = _lib.posterior_cov_numpy(case["A"], P)
    low = np.tril(case["A"] + P)
    ref = np.linalg.inv(low + np.transpose(np.tril(low, -1), (0, 2, 1)))
    assert np.max(np.abs(cov - ref) / np.sqrt(np.einsum("mi,mj->mij", sigma ** 2, sigma ** 2))) <= 1e-6 and not status.any()
    broken = case["A"].copy()
    broken[:, np.triu_indices(11, 1)[0], np.triu_indices(11, 1)[1]] = np.nan
    for a, b in zip(_lib.posterior_cov_numpy(broken, P), (cov, sigma, status)):
        same(a, b)
    with pytest.raises(ValueError):
        _lib.posterior_cov_numpy(case["A"][:, :5, :], None)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 3, 16, 17])
def test_numpy_branch_names_the_failed_pivot(D, dtype):
    """A negative, NaN or infinite diagonal entry behind k sound pivots: status k + 1, cov and sigma of the row NaN
    throughout; the other rows are bitwise those of a call without the bad rows."""
    M = 65
    case = nc.seeded(D, M, True, dtype)
    planted = pc.planted(D)
    A = case["A"].copy()
    for m, (k, v) in planted.items():
        A[m, k, k] = v
    cov, sigma, status = _lib.posterior_cov_numpy(A)
    keep = np.array([m not in planted for m in range(M)])
    for m, (k, _) in planted.items():
        assert status[m] == k + 1, (m, k, status[m])
        assert np.isnan(cov[m]).all() and np.isnan(sigma[m]).all()
    ref = _lib.posterior_cov_numpy(np.ascontiguousarray(case["A"][keep]))
    assert not ref[2].any() and np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for a, b in zip((cov, sigma, status), ref):
        same(a[keep], b)


def test_context_numpy_branch_is_posterior_cov_numpy():
    """``Context.posterior_cov(..., is_gpu=False)`` needs no context: called on the class."""
    case = nc.seeded(5, 9, True, np.float32, prior=True)
    for P in (None, case["prior"][1]):
        got = _lib.Context.posterior_cov(None, case["A"], P, is_gpu=False)
        for a, b in zip(got, _lib.posterior_cov_numpy(case["A"], P)):
            same(a, b)


# ---- the C entry -----------------------------------------------------------------------------------------
def test_new_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "gp_posterior_cov_device"
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in gp_predict_hip.h" % name
    assert hasattr(lib, name), "libgp_predict_hip.so does not export %s" % name
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_int and len(args) == len(m.group(1).split(",")) == 9
    for attr in ("posterior_cov_device", "posterior_cov"):
        assert hasattr(_lib.Context, attr)
    assert callable(_lib.posterior_cov_numpy)


def cov_args(**kw):
    """Arguments of gp_posterior_cov_device that pass every check; ``x`` stands for any non-null pointer."""
    x = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    a = dict(ctx=x, dtype=_lib.GP_F64, d_A=x, d_prior_prec=None, d_cov=x, d_sigma=x, d_status=x, n_rows=1, n_inputs=3)
    a.update(kw)
    return list(a.values())


# The checks run before the context is used, so a stand-in for it reaches the later ones without a GPU; no case here
# passes them all.
ARGUMENT_CASES = [
    (cov_args(ctx=None), GP_ERR_INVALID, "null context"),
    (cov_args(d_A=None), GP_ERR_INVALID, "null device pointer"),
    (cov_args(d_status=None), GP_ERR_INVALID, "null device pointer"),
    (cov_args(d_cov=None, d_sigma=None), GP_ERR_INVALID, "null device pointer"),
    (cov_args(dtype=7), GP_ERR_INVALID, "bad dtype 7"),
    (cov_args(n_rows=0), GP_ERR_INVALID, "bad sizes"),
    (cov_args(n_rows=-3), GP_ERR_INVALID, "bad sizes"),
    (cov_args(n_inputs=0), GP_ERR_INVALID, "bad sizes"),
    (cov_args(n_inputs=33), GP_ERR_UNSUPPORTED, "the Newton step kernels serve n_inputs <= 32"),
]


@pytest.mark.parametrize("args,code,message", ARGUMENT_CASES, ids=[str(i) for i in range(len(ARGUMENT_CASES))])
def test_argument_errors_go_through_the_one_error_buffer(args, code, message):
    lib = _lib.load()
    i32, i64 = ctypes.c_int(), ctypes.c_int64()
    ref = ctypes.byref
    rc = lib.gp_launch_plan(99, _lib.GP_F64, 10, 2, 1, 1, 0, 1, 0, ref(i32), ref(i64), ref(i32), ref(i64), ref(i32), ref(i32))
    assert (rc, lib.gp_last_error_string().decode()) == (GP_ERR_INVALID, "bad op 99")
    rc = lib.gp_posterior_cov_device(*args)
    assert (rc, lib.gp_last_error_string().decode()) == (code, message)


# ---- retrieve_bands --------------------------------------------------------------------------------------
@pytest.mark.parametrize("second_order", ["gauss_newton", "full"])
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("max_iter", [0, 6])
def test_retrieve_bands_numpy_branch_returns_the_covariance(max_iter, with_prior, second_order):
    """Shapes and dtypes; the first five outputs bitwise those of the call without the flag; cov, sigma and cov_status
    bitwise posterior_cov_numpy of _misfit_numpy's matrix at the returned X (plus P); the same through step_fn."""
    gps, obs, X0 = pc.quadratic_problem()
    M, D = X0.shape
    prior = (np.full(D, 0.5), 3.0 * np.eye(D) + 0.5) if with_prior else None
    kw = dict(second_order=second_order, prior=prior, max_iter=max_iter, is_gpu=False)
    plain = perband.retrieve_bands(gps, X0, obs, **kw)
    out = perband.retrieve_bands(gps, X0, obs, return_cov=True, **kw)
    assert len(plain) == 5 and len(out) == 8
    for a, b in zip(plain, out):
        same(a, b)
    X, cov, sigma, cstat = out[0], out[5], out[6], out[7]
    assert cov.shape == (M, D, D) and sigma.shape == (M, D) and cstat.shape == (M,)
    assert cov.dtype == sigma.dtype == np.float64 and cstat.dtype == np.int32
    if max_iter:
        assert out[3].min() >= 1 and not np.array_equal(X, X0)          # the matrix is not the one at X0
    A = perband.misfit_bands(gps, X, obs, second_order=second_order, is_gpu=False)[2]        # (_misfit_numpy's)
    ref = _lib.posterior_cov_numpy(A, prior[1] if with_prior else None)
    for a, b in zip((cov, sigma, cstat), ref):
        same(a, b)
    assert not cstat.any() and np.isfinite(cov).all()
    # through step_fn (the loop runs on the host whatever is_gpu says)
    calls = []

    def step_fn(x, grad, A_, lam):
        calls.append(None)
        return _lib.newton_step_numpy(x, grad, A_, lam, "diagonal", prior, None)
    kw.pop("is_gpu")
    injected = perband.retrieve_bands(gps, X0, obs, return_cov=True, step_fn=step_fn, **kw)
    assert (len(calls) > 0) == (max_iter > 0) and len(injected) == 8
    for a, b in zip(out, injected):
        same(a, b)
    five = perband.retrieve_bands(gps, X0, obs, step_fn=step_fn, **kw)
    assert len(five) == 5
    for a, b in zip(plain, five):
        same(a, b)
