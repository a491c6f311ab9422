"""Prior propagation without a GPU: prior_propagate_numpy against the longdouble truth and the bound of
prior_cases.py, its status codes, gp_prior_propagate_device's declaration and argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest

import newton_cases as nc
import posterior_cases as pc
import prior_cases as prc
from conftest import ROOT

from gp_emulator_amd import _lib

GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def kind_case(D, M, full_rank, prior, dtype, row_prior):
    case = nc.seeded(D, M, full_rank, dtype, prior=prior)
    return prc.row_priors(case) if prior and row_prior else case


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", nc.DIMS)
def test_numpy_branch_within_the_bound(D, dtype):
    """Inputs of either dtype, arithmetic and result in float64; full rank without and with a prior, rank deficient
    with a prior, 65 rows; priors and noise shared and per row.  No row fails; next_prec is symmetric bit for bit."""
    M = 65
    worst = 0.0
    for full_rank, prior in pc.KINDS:
        for per_row in (False, True):
            case = kind_case(D, M, full_rank, prior, dtype, per_row)
            Q = prc.noise(D, full_rank, dtype, M if per_row else None)
            P = case["prior"][1] if prior else None
            got, status = _lib.prior_propagate_numpy(case["A"], P, Q)
            assert got.dtype == np.float64 and got.shape == (M, D, D) and status.dtype == np.int32 and status.shape == (M,)
            t = prc.propagate_truth(case, Q)
            assert t["ok"].all() and not status.any(), (full_rank, prior, per_row)
            same(got, np.ascontiguousarray(np.transpose(got, (0, 2, 1))))
            worst = max(worst, prc.propagate_check(t, got, stored_f32=False))
    print("D = %d %s: worst error / bound %.3g" % (D, np.dtype(dtype).name, worst))


def test_numpy_branch_agrees_with_numpy_inv_and_reads_lower_triangles_only():
    D, M = 11, 40
    case = prc.row_priors(nc.seeded(D, M, True, np.float64, prior=True))
    P, Q = case["prior"][1], prc.noise(D, True, np.float64)
    got, status = _lib.prior_propagate_numpy(case["A"], P, Q)
    ref = np.linalg.inv(np.linalg.inv(case["A"] + P) + Q)
    scale = np.sqrt(np.einsum("mi,mj->mij", np.einsum("mii->mi", ref), np.einsum("mii->mi", ref)))
    assert np.max(np.abs(got - ref) / scale) <= 1e-6 and not status.any()
    iu = np.triu_indices(D, 1)
    A, Pn, Qn = case["A"].copy(), P.copy(), Q.copy()
    A[:, iu[0], iu[1]], Pn[:, iu[0], iu[1]], Qn[iu] = np.nan, np.nan, np.nan
    for a, b in zip(_lib.prior_propagate_numpy(A, Pn, Qn), (got, status)):
        same(a, b)
    with pytest.raises(ValueError):
        _lib.prior_propagate_numpy(case["A"][:, :5, :], None, Q)


def test_repeated_arrays_equal_the_shared_call_exactly():
    D, M = 17, 65
    case = nc.seeded(D, M, False, np.float64, prior=True)
    P, Q = case["prior"][1], prc.noise(D, False, np.float64)
    ref = _lib.prior_propagate_numpy(case["A"], P, Q)
    Pm, Qm = (np.ascontiguousarray(np.broadcast_to(a, (M, D, D))) for a in (P, Q))
    for p, q in ((Pm, Qm), (P, Qm), (Pm, Q)):
        for a, b in zip(ref, _lib.prior_propagate_numpy(case["A"], p, q)):
            same(a, b)
    # and Context.prior_propagate's numpy branch needs no context: called on the class
    for a, b in zip(ref, _lib.Context.prior_propagate(None, case["A"], P, Q, is_gpu=False)):
        same(a, b)


def test_it_is_the_two_inversions_of_posterior_cov_numpy():
    D, M = 11, 9
    case = nc.seeded(D, M, True, np.float64, prior=True)
    P, Q = case["prior"][1], prc.noise(D, True, np.float64)
    cov = _lib.posterior_cov_numpy(case["A"], P)[0]
    same(_lib.prior_propagate_numpy(case["A"], P, Q)[0], _lib.posterior_cov_numpy(cov, Q)[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 3, 16, 17])
def test_status_names_the_failed_pivot_of_either_inversion(D, dtype):
    """A bad diagonal entry of A behind k sound pivots: k + 1.  A large negative (k, k) entry of the row's process noise:
    D + k + 1.  Failed rows are NaN throughout; the others are bitwise those of a call without the bad rows."""
    M = 65
    case = nc.seeded(D, M, True, dtype)
    Q = prc.noise(D, True, dtype)
    first = pc.planted(D)
    A = case["A"].copy()
    for m, (k, v) in first.items():
        A[m, k, k] = v
    Qm, second = prc.planted_noise(D, Q, M)
    got, status = _lib.prior_propagate_numpy(A, None, Qm)
    for m, (k, _) in first.items():
        assert status[m] == k + 1, (m, k, status[m])
    for m, k in second.items():
        assert status[m] == D + k + 1, (m, k, status[m])
    bad = np.array([m in first or m in second for m in range(M)])
    assert np.isnan(got[bad]).all() and not status[~bad].any()
    ref = _lib.prior_propagate_numpy(np.ascontiguousarray(case["A"][~bad]), None, Q)
    assert not ref[1].any() and np.isfinite(ref[0]).all()
    same(got[~bad], ref[0])


# ---- the C entry -----------------------------------------------------------------------------------------
def test_new_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "gp_prior_propagate_device"
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in gp_predict_hip.h" % name
    assert hasattr(lib, name), "libgp_predict_hip.so does not export %s" % name
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_int and len(args) == len(m.group(1).split(",")) == 11
    for attr in ("prior_propagate_device", "prior_propagate"):
        assert hasattr(_lib.Context, attr)
    assert callable(_lib.prior_propagate_numpy)


def prop_args(**kw):
    """Arguments of gp_prior_propagate_device that pass every check; ``x`` stands for any non-null pointer."""
    x = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    a = dict(ctx=x, dtype=_lib.GP_F64, d_A=x, d_prior_prec=x, prec_stride=9, d_noise=x, noise_stride=9, d_next=x, d_status=x,
             n_rows=1, n_inputs=3)
    a.update(kw)
    return list(a.values())


ARGUMENT_CASES = [
    (prop_args(ctx=None), GP_ERR_INVALID, "null context"),
    (prop_args(d_A=None), GP_ERR_INVALID, "null device pointer"),
    (prop_args(d_noise=None), GP_ERR_INVALID, "null device pointer"),
    (prop_args(d_noise=None, noise_stride=0), GP_ERR_INVALID, "null device pointer"),
    (prop_args(d_next=None), GP_ERR_INVALID, "null device pointer"),
    (prop_args(d_status=None), GP_ERR_INVALID, "null device pointer"),
    (prop_args(dtype=7), GP_ERR_INVALID, "bad dtype 7"),
    (prop_args(n_rows=0), GP_ERR_INVALID, "bad sizes"),
    (prop_args(n_inputs=0), GP_ERR_INVALID, "bad sizes"),
    (prop_args(prec_stride=2), GP_ERR_INVALID, "prior precision stride 2 is neither 0 nor >= 9"),
    (prop_args(noise_stride=8), GP_ERR_INVALID, "process noise stride 8 is neither 0 nor >= 9"),
    (prop_args(noise_stride=-9), GP_ERR_INVALID, "process noise stride -9 is neither 0 nor >= 9"),
    (prop_args(d_prior_prec=None), GP_ERR_INVALID, "prior precision stride without a pointer"),
    (prop_args(n_inputs=33), GP_ERR_UNSUPPORTED, "the Newton step kernels serve n_inputs <= 32"),
]


@pytest.mark.parametrize("args,code,message", ARGUMENT_CASES, ids=[str(i) for i in range(len(ARGUMENT_CASES))])
def test_argument_errors_go_through_the_one_error_buffer(args, code, message):
    lib = _lib.load()
    i32, i64 = ctypes.c_int(), ctypes.c_int64()
    ref = ctypes.byref
    rc = lib.gp_launch_plan(99, _lib.GP_F64, 10, 2, 1, 1, 0, 1, 0, ref(i32), ref(i64), ref(i32), ref(i64), ref(i32), ref(i32))
    assert (rc, lib.gp_last_error_string().decode()) == (GP_ERR_INVALID, "bad op 99")
    rc = lib.gp_prior_propagate_device(*args)
    assert (rc, lib.gp_last_error_string().decode()) == (code, message)
