"""The multivariate retrieval without a GPU: the C entries' argument checks, the launch plan of the Gram kernel, the
numpy branches of MultivariateEmulator.weight_gram / gauss_newton_many on the PROSAIL fixture and the loop of
retrieve_many(is_gpu=False) on a synthetic emulator.

Gates: 1e-14 (max-norm) for the row-by-row float64 Gram matrix against a longdouble one (2101-term sums of
like-signed-or-not products: measured 3e-16); 1e-12 between two float64 orders of the Gauss-Newton contraction,
test_misfit_cpu.py's gate for gn."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import mv_retrieve_cases as mc

from gp_emulator_amd import MultivariateEmulator, _lib

GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gp_predict_hip.h")


def test_new_symbols_are_declared_and_exported():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in ("gp_mv_weight_gram_device", "gp_mv_gauss_newton_rows_device"):
        assert re.search(r"\bint %s\(" % name, text)
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"#define GP_OP_MV_GRAM %d\b" % _lib.GP_OP_MV_GRAM, text)
    plan = [int(v) for v in re.findall(r"#define GP_PLAN_MV_GRAM (\d+)", text)]
    assert len(plan) == 1 and _lib.PLAN_KERNELS[plan[0]] == "mv_gram"


def gram_args(**kw):
    """Arguments of gp_mv_weight_gram_device that pass every check; ``x`` stands for any non-null pointer."""
    x = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    a = dict(ctx=x, dtype=_lib.GP_F64, d_basis=x, d_weights=x, weights_stride=33, d_gram=x, n_rows=1, n_pcs=3, n_bands=33)
    a.update(kw)
    return list(a.values())


def gn_rows_args(**kw):
    x = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    a = dict(ctx=x, dtype=_lib.GP_F64, d_deriv=x, d_gram=x, gram_stride=9, d_gn=x, n_rows=1, n_pcs=3, n_inputs=4)
    a.update(kw)
    return list(a.values())


# The checks run before the context is used, so a stand-in for it reaches the later ones without a GPU; no case
# here passes them all.
GRAM, ROWS = "gp_mv_weight_gram_device", "gp_mv_gauss_newton_rows_device"
STRIDE_W = "weights_stride is 0 (one vector for all rows) or >= n_bands"
STRIDE_G = "gram_stride is 0 (one matrix for all rows) or >= n_pcs^2"
ARGUMENT_CASES = [
    (GRAM, gram_args(ctx=None), GP_ERR_INVALID, "null context"),
    (GRAM, [None, _lib.GP_F64, None, None, 0, None, 1, 1, 1], GP_ERR_INVALID, "null context"),
    (GRAM, gram_args(d_basis=None), GP_ERR_INVALID, "null device pointer"),
    (GRAM, gram_args(d_weights=None), GP_ERR_INVALID, "null device pointer"),
    (GRAM, gram_args(d_gram=None), GP_ERR_INVALID, "null device pointer"),
    (GRAM, gram_args(dtype=7), GP_ERR_INVALID, "bad dtype 7"),
    (GRAM, gram_args(n_rows=0), GP_ERR_INVALID, "bad sizes"),
    (GRAM, gram_args(n_rows=-3), GP_ERR_INVALID, "bad sizes"),
    (GRAM, gram_args(n_pcs=0), GP_ERR_INVALID, "bad sizes"),
    (GRAM, gram_args(n_bands=0), GP_ERR_INVALID, "bad sizes"),
    (GRAM, gram_args(weights_stride=1), GP_ERR_INVALID, STRIDE_W),
    (GRAM, gram_args(weights_stride=32), GP_ERR_INVALID, STRIDE_W),
    (GRAM, gram_args(weights_stride=-33), GP_ERR_INVALID, STRIDE_W),
    (GRAM, gram_args(n_pcs=17), GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= 16"),
    (ROWS, gn_rows_args(ctx=None), GP_ERR_INVALID, "null context"),
    (ROWS, [None, _lib.GP_F64, None, None, 0, None, 1, 1, 1], GP_ERR_INVALID, "null context"),
    (ROWS, gn_rows_args(d_deriv=None), GP_ERR_INVALID, "null device pointer"),
    (ROWS, gn_rows_args(d_gram=None), GP_ERR_INVALID, "null device pointer"),
    (ROWS, gn_rows_args(d_gn=None), GP_ERR_INVALID, "null device pointer"),
    (ROWS, gn_rows_args(dtype=-1), GP_ERR_INVALID, "bad dtype -1"),
    (ROWS, gn_rows_args(n_rows=0), GP_ERR_INVALID, "bad sizes"),
    (ROWS, gn_rows_args(n_pcs=0), GP_ERR_INVALID, "bad sizes"),
    (ROWS, gn_rows_args(n_inputs=0), GP_ERR_INVALID, "bad sizes"),
    (ROWS, gn_rows_args(n_pcs=17, gram_stride=289), GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= 16"),
    (ROWS, gn_rows_args(n_inputs=65), GP_ERR_UNSUPPORTED, "misfit kernels serve n_inputs <= 64"),
    (ROWS, gn_rows_args(gram_stride=1), GP_ERR_INVALID, STRIDE_G),
    (ROWS, gn_rows_args(gram_stride=8), GP_ERR_INVALID, STRIDE_G),
    (ROWS, gn_rows_args(gram_stride=-9), GP_ERR_INVALID, STRIDE_G),
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


def blocks_of(P):
    return -(-(P * (P + 1) // 2) // 16)


# workgroups per CU of instance NPB (index NPB - 1): what the accumulators (8 reals per block and lane) leave room for
WGS_PER_CU = {np.float64: [4, 4, 3, 2, 2, 2, 2, 1, 1], np.float32: [4, 4, 4, 4, 3, 3, 3, 2, 2]}


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("cu", [256, 8])
def test_launch_plan(prec, cu):
    """weight_gram_kernel: 4 waves x 16 rows = 64 rows per item over all bands; rounds balanced as misfit_kernel's."""
    first = _lib.launch_plan("mv_gram", prec, 1, n_pcs=12, n_bands=2101, compute_units=cu)
    assert first == dict(kernel="mv_gram", rows_per_item=64, items=1, workgroups=1, rest_items=0, rest_workgroups=0)
    for P in (3, 12, 16):
        cap, rpi = WGS_PER_CU[prec][blocks_of(P) - 1] * cu, 64
        one_round = cap * rpi
        for rows in (1, one_round - 1, one_round, one_round + 1, 3 * one_round, 3 * one_round + 1):
            p = _lib.launch_plan("mv_gram", prec, rows, n_pcs=P, n_bands=33, compute_units=cu)
            assert p["kernel"] == "mv_gram" and p["rows_per_item"] == rpi
            assert p["items"] == -(-rows // rpi)
            assert 1 <= p["workgroups"] <= min(p["items"], cap)
            assert p["rest_items"] == 0 and p["rest_workgroups"] == 0
        assert _lib.launch_plan("mv_gram", prec, one_round, n_pcs=P, n_bands=33, compute_units=cu)["workgroups"] == cap
        past = _lib.launch_plan("mv_gram", prec, one_round + 1, n_pcs=P, n_bands=33, compute_units=cu)
        assert past["items"] == cap + 1 > past["workgroups"]
        # balanced rounds: no workgroup is left with a whole extra round
        assert -(-past["items"] // past["workgroups"]) == 2
        three = _lib.launch_plan("mv_gram", prec, 3 * one_round + 1, n_pcs=P, n_bands=33, compute_units=cu)
        assert three["items"] == 3 * cap + 1 and -(-three["items"] // three["workgroups"]) == 4
        assert three["workgroups"] == -(-three["items"] // 4)
    with pytest.raises(_lib.GpuPredictError):          # as gp_mv_weight_gram_device
        _lib.launch_plan("mv_gram", prec, 1000, n_pcs=17, n_bands=33, compute_units=cu)
    with pytest.raises(_lib.GpuPredictError):
        _lib.launch_plan("mv_gram", prec, 1000, n_pcs=3, n_bands=0, compute_units=cu)


# ---- the numpy branches on PROSAIL ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mv_case():
    g = load_golden("prosail_mv")
    basis = np.array(g["basis_functions"], copy=True)
    X = g["train_data"].T @ basis
    mv = MultivariateEmulator(X=X, y=g["y_train"], hyperparams=g["hyperparams"], basis_functions=basis,
                              n_pcs=int(g["n_pcs"]))
    lo, hi = g["y_train"].min(0), g["y_train"].max(0)
    rs = np.random.RandomState(11)
    Y = lo + (hi - lo) * rs.random_sample((7, lo.size))
    w = rs.uniform(0.5, 2.0, (7, basis.shape[1]))
    w[rs.random_sample(w.shape) < 0.3] = 0.0                    # masked bands
    return mv, Y, w


def test_weight_gram_numpy_branch(mv_case):
    mv, Y, w = mv_case
    P, B = mv.n_pcs, mv.basis_functions.shape[1]
    G = mv.weight_gram(w, is_gpu=False)
    assert G.shape == (7, P, P) and G.dtype == np.float64
    b = np.asarray(mv.basis_functions, dtype=mc.LD)
    ref = np.einsum("pb,mb,qb->mpq", b, w.astype(mc.LD), b)
    e = mc.err(ref, G)
    print("weight_gram numpy branch against longdouble: %.3g" % e)
    assert e <= 1e-14
    # a row's matrix does not depend on how many rows the call has
    for m in (0, 3, 6):
        mc.same(mv.weight_gram(w[m:m + 1], is_gpu=False)[0], G[m])
    assert mv.weight_gram(np.zeros((0, B)), is_gpu=False).shape == (0, P, P)
    for bad in (w[0], w[:, :-1], np.ones((2, 3, B))):
        for is_gpu in (False, True):          # the shapes are checked before anything touches a device
            with pytest.raises(ValueError):
                mv.weight_gram(bad, is_gpu=is_gpu)


def test_gauss_newton_many_numpy_branch(mv_case):
    mv, Y, w = mv_case
    M, D = Y.shape
    jac = mv.predict_many(Y, is_gpu=False, do_deriv=True)[1]
    gn = mv.gauss_newton_many(Y, weights=w, is_gpu=False)
    assert gn.shape == (M, D, D) and gn.dtype == np.float64
    e = mc.err(np.einsum("mdb,mb,meb->mde", jac, w, jac), gn)
    print("gauss_newton_many numpy branch, per-row weights, against the full Jacobian: %.3g" % e)
    assert e <= 1e-12
    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))            # exactly symmetric
    # None and shared weights: misfit_many's gn, bit for bit
    obs = np.zeros(jac.shape[2])
    for ws in (None, w[2]):
        mc.same(mv.gauss_newton_many(Y, weights=ws, is_gpu=False),
                mv.misfit_many(Y, obs, weights=ws, is_gpu=False, do_deriv=False, gauss_newton=True)[1])
    # every row with the same weights: the shared form to rounding
    tiled = mv.gauss_newton_many(Y, weights=np.tile(w[2], (M, 1)), is_gpu=False)
    assert mc.err(mv.gauss_newton_many(Y, weights=w[2], is_gpu=False), tiled) <= 1e-12
    for is_gpu in (False, True):
        with pytest.raises(ValueError):
            mv.gauss_newton_many(Y, weights=w[:3], is_gpu=is_gpu)
        with pytest.raises(ValueError):
            mv.gauss_newton_many(Y, weights=w[:, :-1], is_gpu=is_gpu)
    # misfit_many itself still refuses per-row weights for its own Gauss-Newton term
    with pytest.raises(ValueError):
        mv.misfit_many(Y, np.zeros((M, jac.shape[2])), weights=w, is_gpu=False, gauss_newton=True)


# ---- the loop of retrieve_many ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.RETRIEVAL_SHAPES)
def test_retrieve_many_numpy_branch(shape):
    c = mc.retrieval_case(*shape)
    mv, obs, Y0, w, bounds = c["mv"], c["obs"], c["Y0"], c["w"], c["bounds"]
    M, D = Y0.shape
    kw = dict(weights=w, bounds=bounds, is_gpu=False)
    runs = [mv.retrieve_many(Y0, obs, max_iter=k, **kw) for k in (0, 1, 2, 3, 4)]
    # max_iter = 0: the start and its cost
    mc.same(runs[0][0], Y0)
    mc.same(runs[0][1], c["cost0"])
    assert not runs[0][2].any() and not runs[0][3].any() and np.all(runs[0][4] == 1e-2)
    for a, b in zip(runs, runs[1:]):
        assert np.all(b[1] <= a[1]) and np.all(b[3] >= a[3])
    assert np.all(runs[1][3] <= 1) and np.all(runs[-1][3] <= 4)
    for r in runs + [c["ref"]]:
        assert np.all(r[0] >= 0.0) and np.all(r[0] <= 1.0)
    X, cost, state, n_acc, lam = c["ref"]
    assert X.shape == (M, D) and cost.shape == state.shape == n_acc.shape == lam.shape == (M,)
    assert X.dtype == cost.dtype == lam.dtype == np.float64 and state.dtype == n_acc.dtype == np.int32
    assert np.all(cost <= runs[-1][1]) and n_acc.min() >= 2
    print("retrieve_many numpy %s: cost max %.3g -> %.3g, accepted %d..%d" % (shape, c["cost0"].max(), cost.max(),
                                                                             n_acc.min(), n_acc.max()))
    assert cost.max() <= 1e-5 * c["cost0"].max()
    # the returned cost is the data term at the returned rows
    assert mc.err(mv.misfit_many(X, obs, weights=w, is_gpu=False, do_deriv=False), cost) <= 1e-12
    # shared weights and none drive the other contraction
    for ws in (w[0], None):
        r = mv.retrieve_many(Y0, obs, weights=ws, bounds=bounds, is_gpu=False)
        r0 = mv.retrieve_many(Y0, obs, weights=ws, bounds=bounds, is_gpu=False, max_iter=0)
        assert np.all(r[1] <= r0[1]) and r[3].min() >= 2
    # the covariance does not change the five
    prior = (np.full(D, 0.5), 32.0 * np.eye(D))
    for pr in (None, prior):
        for extra in (dict(max_iter=0), dict()):
            plain = mv.retrieve_many(Y0, obs, prior=pr, **extra, **kw)
            out = mv.retrieve_many(Y0, obs, prior=pr, return_cov=True, **extra, **kw)
            assert len(plain) == 5 and len(out) == 8
            for a, b in zip(plain, out):
                mc.same(a, b)
            assert out[5].shape == (M, D, D) and out[6].shape == (M, D) and out[7].shape == (M,)
            gn = mv.gauss_newton_many(out[0], weights=w, is_gpu=False)
            cov, sigma, cstat = _lib.posterior_cov_numpy(gn, pr[1] if pr else None)
            mc.same(out[7], cstat)
            assert mc.err(cov, out[5]) <= 1e-9 and mc.err(sigma, out[6]) <= 1e-9


def test_retrieve_many_bad_arguments():
    c = mc.retrieval_case(*mc.RETRIEVAL_SHAPES[1])
    mv, obs, Y0, w = c["mv"], c["obs"], c["Y0"], c["w"]
    M, D = Y0.shape
    B = obs.shape[1]
    for is_gpu in (False, True):             # the shapes are checked before anything touches a device
        for bad in (dict(Y0=Y0[0]), dict(Y0=Y0[:, :-1]), dict(obs=obs[:3]), dict(obs=obs[0, :-1]), dict(weights=w[:3]),
                    dict(weights=np.ones(B + 1)), dict(prior=(np.zeros(D + 1), np.eye(D))), dict(bounds=(np.zeros(D), np.ones(D - 1)))):
            kw = dict(dict(Y0=Y0, obs=obs, weights=w), **bad)
            with pytest.raises(ValueError):
                mv.retrieve_many(kw.pop("Y0"), kw.pop("obs"), is_gpu=is_gpu, **kw)
        with pytest.raises(TypeError):       # Gauss-Newton only
            mv.retrieve_many(Y0, obs, weights=w, second_order="full", is_gpu=is_gpu)
