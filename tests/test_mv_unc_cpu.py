"""The MultivariateEmulator misfit with the per-PC emulators' variance in the data term, without a GPU: the 80-bit truth
of mv_unc_cases against the dense N_full x N_full Gaussian, central differences and the dense Fisher trace formula; its
P = B = 1 reduction to the per-band term; the numpy branch against the truth; the preconditions of the GPU rules; the
argument errors of the new entry and keywords; and the retrieval's covariance."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
import band_unc_cases
import far_rows_cases
import mv_unc_cases as uc

from gp_emulator_amd import _lib

LD = np.longdouble
GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gp_predict_hip.h")
SMALL = [c for c in uc.CASES if c[4] == 33]
CASE_IDS = ["n%d-d%d-P%d-%g-B%d" % c for c in uc.CASES]
SMALL_IDS = ["n%d-d%d-P%d-%g-B%d" % c for c in SMALL]


def some_rows(c, k=8):
    """The first k rows of the case (in the unit box) and its last four (outside it)."""
    sel = np.r_[np.arange(k), np.arange(uc.M_MAX - 4, uc.M_MAX)]
    return c["t"][sel], c["obs"][sel]


@pytest.mark.parametrize("shape", SMALL, ids=SMALL_IDS)
def test_truth_is_the_dense_gaussian(shape):
    """cost = 1/2 r^T C^-1 r + 1/2 log det(C diag(w)), ceff = B C^-1 r, Geff = B C^-1 B^T and gn = J^T C^-1 J + 1/2
    tr(C^-1 dC C^-1 dC) with the dense C (33 x 33), all in longdouble: 1e-14 is 2e5 of its roundings, for sums of 33
    terms and matrices whose condition stays below 1e3."""
    c = uc.case(*shape)
    X, obs = some_rows(c)
    basis, w = c["mv"].basis_functions.astype(LD), c["w"]
    mu, dmu, v, dv = band_unc_cases.terms_ld(c["gps"], X)
    got = uc.truth_at(c, X, w, obs)
    cost, Cinv = uc.dense_cost(mu, v, basis, obs, w)
    assert np.all(got["cost"] > 0)
    assert uc.err(cost, got["cost"]) <= 1e-14
    r = mu.T @ basis - obs.astype(LD)
    assert uc.err(np.einsum("pb,mbc,mc->pm", basis, Cinv, r), got["ceff"]) <= 1e-14
    assert uc.err(np.einsum("pb,mbc,qc->mpq", basis, Cinv, basis), got["geff"]) <= 1e-14
    dvp = np.where((v <= 0)[:, :, None], LD(0), dv)
    J = np.einsum("pmd,pb->mdb", dmu, basis)                             # d f_b / d x_d
    dC = np.einsum("pb,pmd,pc->mdbc", basis, dvp, basis)
    CdC = np.einsum("mab,mdbc->mdac", Cinv, dC)
    fisher = np.einsum("mdb,mbc,mec->mde", J, Cinv, J) + LD(0.5) * np.einsum("mdac,meca->mde", CdC, CdC)
    assert uc.err(fisher, got["gn"]) <= 1e-14
    assert np.all(np.linalg.eigvalsh(got["gn"].astype(np.float64)) >= -1e-12 * np.abs(got["gn"]).max())


@pytest.mark.parametrize("shape", SMALL, ids=SMALL_IDS)
def test_gradient_is_the_derivative_of_the_cost(shape):
    """Central differences of the 80-bit cost with h = 1e-5: the truncation is h^2 / 6 times a third derivative (the
    length scales are >= 0.25, so at most a few hundred times the gradient), the rounding 2^-63 cost / h: 1e-6 of the
    largest gradient element bounds both."""
    c = uc.case(*shape)
    X, obs = some_rows(c, 4)
    w = c["w"]
    grad = uc.truth_at(c, X, w, obs)["grad"]
    h = LD(1e-5)
    num = np.zeros_like(grad)
    for d in range(X.shape[1]):
        e = np.zeros(X.shape[1], LD)
        e[d] = h
        num[:, d] = (uc.truth_at(c, X.astype(LD) + e, w, obs)["cost"] - uc.truth_at(c, X.astype(LD) - e, w, obs)["cost"]) / (2 * h)
    assert uc.err(grad, num) <= 1e-6


def test_one_pc_and_one_band_is_the_per_band_term():
    n, d, nugget = 40, 3, 1e-1
    gps, b = band_unc_cases.emulators(n, d, 1, nugget)
    X = band_unc_cases.rows(d, 9, 77)
    mu, dmu, v, dv = band_unc_cases.terms_ld(gps, X)
    rs = np.random.RandomState(1)
    obs, w = rs.standard_normal((1, 9)), rs.uniform(0.5, 1.5, (1, 9)) / (nugget * b[0])
    v = v.copy()
    v[0, 2] = -v[0, 2]                                           # one clamped pair
    ref = band_unc_cases.truth(mu, dmu, v, dv, obs, w)
    J0, c, G = uc.plain_terms(mu, np.ones((1, 1)), obs.T, w.T)
    got = uc.term(J0, c, G, v, dmu, dv)
    for k in ("cost", "grad", "gn"):
        assert uc.err(ref[k][0], got[k]) <= 1e-17, k


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("shape", uc.CASES, ids=CASE_IDS)
def test_numpy_branch_against_the_truth(shape, per_row):
    c = uc.case(*shape)
    M = 24
    X = np.r_[c["t"][:M - 4], c["t"][-4:]]
    obs = np.r_[c["obs"][:M - 4], c["obs"][-4:]]
    w = np.r_[c["w_rows"][:M - 4], c["w_rows"][-4:]] if per_row else c["w"]
    ref = uc.truth_at(c, X, w, obs)
    cost, grad, gn = c["mv"].misfit_many(X, obs, weights=w, is_gpu=False, gauss_newton=True, emulator_unc=True)
    assert cost.dtype == grad.dtype == gn.dtype == np.float64
    for k, got in (("cost", cost), ("grad", grad), ("gn", gn)):
        assert uc.err(ref[k], got) <= uc.PLAIN_TOL, k
    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))
    assert np.array_equal(cost, c["mv"].misfit_many(X, obs, weights=w, is_gpu=False, do_deriv=False, emulator_unc=True))
    one = c["mv"].misfit(X[3], obs[3], weights=w[3] if per_row else w, is_gpu=False, gauss_newton=True, emulator_unc=True)
    for a, b in zip(one, (cost[3], grad[3], gn[3])):             # (numpy's products round differently per shape)
        assert uc.err(b, a) <= uc.PLAIN_TOL


def test_zero_weights_drop_the_band():
    """30 % of the shared weights 0: the call equals the call on the surviving bands only, to the plain gate."""
    c = uc.case(*uc.CASES[1])
    X, obs = some_rows(c)
    w = c["w"].copy()
    w[np.random.RandomState(2).random_sample(w.size) < 0.3] = 0.0
    keep = w > 0
    assert 0 < keep.sum() < w.size
    sub = uc.shell(c["gps"], c["mv"].basis_functions[:, keep])
    a = c["mv"].misfit_many(X, obs, weights=w, is_gpu=False, gauss_newton=True, emulator_unc=True)
    b = sub.misfit_many(X, obs[:, keep], weights=w[keep], is_gpu=False, gauss_newton=True, emulator_unc=True)
    for x, y in zip(a, b):
        assert uc.err(y, x) <= uc.PLAIN_TOL


@pytest.mark.parametrize("shape", uc.CASES, ids=CASE_IDS)
def test_clamped_case_precondition(shape):
    """invQ = 1e6 I: the numpy branch clamps every (PC, row) pair of the rows the GPU rule uses, and is the plain term."""
    c = uc.case(*shape)
    mv = uc.clamped_emulator(c)
    X, obs, w = c["t"][:65], c["obs"][:65], c["w_rows"][:65]
    v = np.stack([gp.cpu_predict(X, do_unc=True)[1] for gp in mv.emulators])
    assert np.all(v <= 0)
    assert np.array_equal(mv.predict_many(X, is_gpu=False), c["mv"].predict_many(X, is_gpu=False))
    cost, grad, gn = mv.misfit_many(X, obs, weights=w, is_gpu=False, gauss_newton=True, emulator_unc=True)
    cost0, grad0 = mv.misfit_many(X, obs, weights=w, is_gpu=False)
    gn0 = mv.gauss_newton_many(X, weights=w, is_gpu=False)
    assert uc.err(cost0, cost) <= 1e-14 and uc.err(grad0, grad) <= 1e-13 and uc.err(gn0, gn) <= 1e-13


def test_far_rows_precondition():
    """A finite far row has mu = 0, v = b, dmu = dv = 0 exactly on the numpy branch: grad = 0 and gn = 0 exactly, and the
    cost is the formula at mu = 0, v = b; a NaN row is NaN throughout."""
    n, d, P, nugget, B = uc.CASES[3]
    c = uc.case(n, d, P, nugget, B)
    far = far_rows_cases.put_special_rows(c["t"][:far_rows_cases.M])
    zero_rows, nan_rows, others = far_rows_cases.classify(far, np.float64)
    obs, w = c["obs"][:far_rows_cases.M], c["w_rows"][:far_rows_cases.M]
    cost, grad, gn = c["mv"].misfit_many(far, obs, weights=w, is_gpu=False, gauss_newton=True, emulator_unc=True)
    assert np.all(grad[zero_rows] == 0) and np.all(gn[zero_rows] == 0)
    k = len(zero_rows)
    J0, cf, G = uc.plain_terms(np.zeros((P, k)), c["mv"].basis_functions, obs[zero_rows], w[zero_rows])
    ref = uc.term(J0, cf, G, np.repeat(c["b"][:, None], k, 1), np.zeros((P, k, d)), np.zeros((P, k, d)))
    assert uc.err(ref["cost"], cost[zero_rows]) <= uc.PLAIN_TOL
    for a in (cost, grad, gn):                                   # (numpy answers a row holding an infinity: not asserted)
        assert np.isnan(a[list(far_rows_cases.NAN_ROWS)]).all() and np.isfinite(a[others]).all()
    plain = c["mv"].misfit_many(c["t"][:far_rows_cases.M], obs, weights=w, is_gpu=False, gauss_newton=True, emulator_unc=True)
    for a, b in zip((cost, grad, gn), plain):
        assert uc.err(b[others], a[others]) <= 1e-13


def test_float32_yardstick_stays_under_the_cap():
    """The all-float32 evaluation of the term against the truth: 16 x its error is the float32 end-to-end gate, capped at
    1e-2; the nuggets of F32_CASES keep the yardstick alone under the cap."""
    for shape in uc.F32_CASES:
        c = uc.case(*shape)
        sel = np.r_[np.arange(61), np.arange(uc.M_MAX - 4, uc.M_MAX)]          # the GPU tests' rows
        X, obs = c["t"][sel], c["obs"][sel]
        for w in (c["w"], c["w_rows"][sel]):
            ref = uc.truth_at(c, X, w, obs)
            f32 = uc.truth_at(c, X, w, obs, work=np.float32)
            for k in ("cost", "grad", "gn"):
                e = uc.err(ref[k], f32[k])
                print("%s %s float32 yardstick %.3g" % (shape, k, e))
                assert e <= 1e-2, (shape, k)


# ---- argument errors ------------------------------------------------------------------------------------------------
def unc_args(**kw):
    """Arguments of gp_mv_misfit_unc_device that pass every check; ``x`` stands for any non-null pointer."""
    x = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    a = dict(ctx=x, dtype=_lib.GP_F64, d_cost0=x, d_coef=x, d_gram=x, gram_stride=9, d_var=x, d_deriv=x, d_dvar=x, d_cost=x,
             d_grad=x, d_gn=x, d_ceff=None, d_geff=None, n_rows=1, n_pcs=3, n_inputs=4)
    a.update(kw)
    return list(a.values())


UNC = "gp_mv_misfit_unc_device"
STRIDE_G = "gram_stride is 0 (one matrix for all rows) or >= n_pcs^2"
# The checks run before the context is used, so a stand-in for it reaches the later ones without a GPU; no case here
# passes them all.
ARGUMENT_CASES = [
    (unc_args(ctx=None), GP_ERR_INVALID, "null context"),
    (unc_args(d_cost0=None), GP_ERR_INVALID, "null device pointer"),
    (unc_args(d_coef=None), GP_ERR_INVALID, "null device pointer"),
    (unc_args(d_gram=None), GP_ERR_INVALID, "null device pointer"),
    (unc_args(d_var=None), GP_ERR_INVALID, "null device pointer"),
    (unc_args(d_cost=None), GP_ERR_INVALID, "null device pointer"),
    (unc_args(d_deriv=None), GP_ERR_INVALID, "the gradient and gn need d_deriv and d_dvar"),
    (unc_args(d_dvar=None, d_grad=None), GP_ERR_INVALID, "the gradient and gn need d_deriv and d_dvar"),
    (unc_args(dtype=7), GP_ERR_INVALID, "bad dtype 7"),
    (unc_args(n_rows=0), GP_ERR_INVALID, "bad sizes"),
    (unc_args(n_rows=-3), GP_ERR_INVALID, "bad sizes"),
    (unc_args(n_pcs=0), GP_ERR_INVALID, "bad sizes"),
    (unc_args(n_inputs=0), GP_ERR_INVALID, "bad sizes"),
    (unc_args(gram_stride=1), GP_ERR_INVALID, STRIDE_G),
    (unc_args(gram_stride=8), GP_ERR_INVALID, STRIDE_G),
    (unc_args(gram_stride=-9), GP_ERR_INVALID, STRIDE_G),
    (unc_args(n_pcs=17, gram_stride=0), GP_ERR_UNSUPPORTED, "the variance term's kernel serves n_pcs <= 16"),
    (unc_args(n_inputs=17), GP_ERR_UNSUPPORTED, "the variance term's kernel serves n_inputs <= 16"),
    (unc_args(n_rows=(2 ** 31 - 1) * 8 + 1, gram_stride=0), GP_ERR_INVALID, "n_rows too large for one launch"),
]


def test_new_symbol_is_declared_and_exported():
    lib = _lib.load()
    assert re.search(r"\bint %s\(" % UNC, open(HEADER).read())
    assert UNC in _lib.SIGNATURES and getattr(lib, UNC) is not None
    assert len(_lib.SIGNATURES[UNC][1]) == 17


@pytest.mark.parametrize("args,code,message", ARGUMENT_CASES, ids=[str(i) for i in range(len(ARGUMENT_CASES))])
def test_argument_errors_of_the_new_entry(args, code, message):
    lib = _lib.load()
    rc = getattr(lib, UNC)(*args)
    assert (rc, lib.gp_last_error_string().decode()) == (code, message)


def test_keyword_errors():
    c = uc.case(*uc.CASES[0])
    mv, X, obs = c["mv"], c["t"][:3], c["obs"][:3]
    for gpu in (False, True):                                    # (raised before any device work)
        with pytest.raises(ValueError, match="Hessian of the variance"):
            mv.misfit_many(X, obs, is_gpu=gpu, return_coef=True, emulator_unc=True)
    with pytest.raises(ValueError, match="obs must be"):
        mv.misfit_many(X, obs[:2], is_gpu=False, emulator_unc=True)
    with pytest.raises(ValueError, match="gauss_newton=True needs weights shared"):
        mv.misfit_many(X, obs, weights=c["w_rows"][:3], is_gpu=False, gauss_newton=True)      # (still the plain rule)


# ---- the retrieval ----------------------------------------------------------------------------------------------------
def test_retrieval_lowers_the_cost_and_widens_sigma():
    """retrieve_many(emulator_unc=True, is_gpu=False) lowers the term it minimises; and at a FIXED x the Fisher matrix's
    mean part dmu^T Geff dmu is below the plain dmu^T G dmu (Geff = G - G N G with N positive semi-definite), so with the
    same prior P -- and with the variance part left out -- sigma can only grow: checked through the matrices."""
    from gp_emulator_amd import _dense_numpy
    c = uc.case(*uc.CASES[1])
    mv, d = c["mv"], 3
    M = 16
    X0, obs, w = np.clip(c["t"][:M], 0.0, 1.0), c["obs"][:M], c["w_rows"][:M]
    prior = (np.full(d, 0.5), 4.0 * np.eye(d))
    bounds = (np.zeros(d), np.ones(d))
    kw = dict(weights=w, prior=prior, bounds=bounds, is_gpu=False, emulator_unc=True)
    start = mv.retrieve_many(X0, obs, max_iter=0, **kw)
    out = mv.retrieve_many(X0, obs, return_cov=True, return_A=True, **kw)
    assert len(out) == 9 and np.array_equal(start[0], X0)
    F0 = start[1] + 0.5 * np.einsum("md,de,me->m", X0 - 0.5, prior[1], X0 - 0.5)
    F1 = out[1] + 0.5 * np.einsum("md,de,me->m", out[0] - 0.5, prior[1], out[0] - 0.5)
    assert np.all(F1 <= F0) and np.any(F1 < F0) and out[3].max() >= 1
    X, cov, sigma, cstat, A = out[0], out[5], out[6], out[7], out[8]
    assert not cstat.any()
    cost, grad, gn = mv.misfit_many(X, obs, weights=w, is_gpu=False, gauss_newton=True, emulator_unc=True)
    assert uc.err(gn, A) <= 1e-12 and uc.err(cost, out[1]) <= 1e-12
    assert uc.err(_dense_numpy.posterior_cov_numpy(gn, prior[1])[0], cov) <= 1e-12
    # at the fixed rows X: the matrices
    mu, dmu, v, dv = band_unc_cases.terms_f64(c["gps"], X)
    J0, cf, G = uc.plain_terms(mu, mv.basis_functions, obs, w, np.float64)
    t = uc.term(J0, cf, G, v, dmu, dv, np.float64)
    assert np.all(v > 0)
    gap = uc.mirror(G) - t["geff"]
    assert np.all(np.linalg.eigvalsh(gap) >= -1e-12 * np.abs(G).max())              # Geff <= G
    A_mean = np.einsum("pmd,mpq,qme->mde", dmu, t["geff"], dmu)
    A_plain = mv.gauss_newton_many(X, weights=w, is_gpu=False)
    s_unc = _dense_numpy.posterior_cov_numpy(A_mean, prior[1])[1]
    s_plain = _dense_numpy.posterior_cov_numpy(A_plain, prior[1])[1]
    assert np.all(s_unc >= s_plain * (1 - 1e-12)) and np.any(s_unc > s_plain * (1 + 1e-6))


def test_series_passes_the_keyword_through():
    c = uc.case(*uc.CASES[1])
    mv, d, M, T = c["mv"], 3, 8, 3
    X0 = np.clip(c["t"][:M], 0.0, 1.0)
    obs = np.stack([c["obs"][k * M:(k + 1) * M] for k in range(T)])
    w = np.stack([c["w_rows"][k * M:(k + 1) * M] for k in range(T)])
    prior = (np.full(d, 0.5), 4.0 * np.eye(d))
    kw = dict(bounds=(np.zeros(d), np.ones(d)), is_gpu=False, max_iter=6)
    plain = mv.retrieve_series(X0, obs, w, prior, 1e-3 * np.eye(d), smooth=True, **kw)
    unc = mv.retrieve_series(X0, obs, w, prior, 1e-3 * np.eye(d), smooth=True, emulator_unc=True, **kw)
    assert len(unc) == len(plain) == 10
    first = mv.retrieve_many(X0, obs[0], w[0], prior=prior, return_cov=True, emulator_unc=True, **kw)
    assert np.array_equal(unc[0][0], first[0]) and np.array_equal(unc[1][0], first[6])
    assert not np.array_equal(unc[0], plain[0])
