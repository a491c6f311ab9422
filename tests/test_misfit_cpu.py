"""Observation misfit of the multivariate emulator without a GPU: the numpy branch of MultivariateEmulator.misfit /
misfit_many (the statement of the formulas that the GPU tests compare against), hessian_many(coef=) and the launch plan
of the misfit kernel.

  cost = 1/2 sum_b w_b (f_b - obs_b)^2,  coef = basis (w * r),  grad = Jac (w * r),  gn = Jac diag(w) Jac^T

Gates: 1e-5 against the reference's own fwd / jac (the gates test_multivariate_emulator_cpu_matches_reference_outputs
uses for them: the misfit is a sum of their products); 1e-5 for central differences (measured 2.8e-7 at a step of 1e-4
of the training range); 1e-12 between two float64 orders of the same contraction."""
import numpy as np
import pytest

from conftest import load_golden

from gp_emulator_amd import MultivariateEmulator, _lib


def maxnorm(ref, got):
    return np.max(np.abs(np.asarray(got) - ref)) / np.max(np.abs(ref))


@pytest.fixture(scope="module")
def mv_case():
    g = load_golden("prosail_mv")
    basis = np.array(g["basis_functions"], copy=True)
    X = g["train_data"].T @ basis
    mv = MultivariateEmulator(X=X, y=g["y_train"], hyperparams=g["hyperparams"], basis_functions=basis,
                              n_pcs=int(g["n_pcs"]))
    lo, hi = g["y_train"].min(0), g["y_train"].max(0)
    rs = np.random.RandomState(11)
    Y = lo + (hi - lo) * rs.random_sample((50, lo.size))
    Y2 = lo + (hi - lo) * rs.random_sample((50, lo.size))
    obs = mv.predict_many(Y2, is_gpu=False)
    return g, mv, Y, obs, hi - lo


def test_numpy_branch_matches_reference_outputs(mv_case):
    """cost and grad from the reference's own fwd and jac at its points, obs = a training spectrum, w = 1."""
    g, mv = mv_case[:2]
    obs = g["x_train_row17"]
    r = g["fwd"] - obs
    ref_cost = 0.5 * np.sum(r * r, axis=1)
    ref_grad = np.einsum("mdb,mb->md", g["jac"], r)
    cost, grad = mv.misfit_many(g["points"], obs, is_gpu=False)
    assert cost.shape == (4,) and grad.shape == (4, 10)
    e_c, e_g = maxnorm(ref_cost, cost), maxnorm(ref_grad, grad)
    print("misfit numpy branch against the reference's outputs: cost %.3g grad %.3g" % (e_c, e_g))
    assert e_c <= 1e-5 and e_g <= 1e-5


def test_gradient_against_central_differences(mv_case):
    _, mv, Y, obs, rng = mv_case
    cost, grad = mv.misfit_many(Y, obs, is_gpu=False)
    fd = np.empty_like(grad)
    for d in range(Y.shape[1]):
        h = 1e-4 * rng[d]
        Yp, Ym = Y.copy(), Y.copy()
        Yp[:, d] += h
        Ym[:, d] -= h
        fd[:, d] = (mv.misfit_many(Yp, obs, is_gpu=False, do_deriv=False)
                    - mv.misfit_many(Ym, obs, is_gpu=False, do_deriv=False)) / (2 * h)
    err = maxnorm(fd, grad)
    print("misfit gradient against central differences: %.3g" % err)
    assert err <= 1e-5


def test_shapes_broadcasting_and_gauss_newton(mv_case):
    _, mv, Y, obs, _ = mv_case
    Y, obs = Y[:7], obs[:7]
    M, D = Y.shape
    P, B = mv.n_pcs, mv.basis_functions.shape[1]
    rs = np.random.RandomState(3)
    w = rs.uniform(0.5, 2.0, B)
    fwd, jac = mv.predict_many(Y, is_gpu=False, do_deriv=True)
    # the formulas, the long way round: through the reconstructed spectra and the full Jacobian
    r = fwd - obs
    cost, grad, gn, coef = mv.misfit_many(Y, obs, weights=w, is_gpu=False, gauss_newton=True, return_coef=True)
    assert cost.shape == (M,) and grad.shape == (M, D) and gn.shape == (M, D, D) and coef.shape == (M, P)
    assert maxnorm(0.5 * np.sum(w * r * r, axis=1), cost) <= 1e-12
    assert maxnorm(np.einsum("mdb,mb->md", jac, w * r), grad) <= 1e-12
    assert maxnorm((w * r) @ mv.basis_functions.T, coef) <= 1e-12
    assert maxnorm(np.einsum("mdb,b,meb->mde", jac, w, jac), gn) <= 1e-12
    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))            # exactly symmetric
    gn1 = mv.misfit_many(Y, obs, is_gpu=False, do_deriv=False, gauss_newton=True)[1]
    assert maxnorm(np.einsum("mdb,meb->mde", jac, jac), gn1) <= 1e-12
    assert np.array_equal(gn1, np.transpose(gn1, (0, 2, 1)))
    # what is returned, and in which order
    only = mv.misfit_many(Y, obs, is_gpu=False, do_deriv=False)
    assert isinstance(only, np.ndarray) and only.shape == (M,)
    c2, k2 = mv.misfit_many(Y, obs, weights=w, is_gpu=False, do_deriv=False, return_coef=True)
    assert np.array_equal(c2, cost) and np.array_equal(k2, coef)
    # shared against per-row observations and weights
    a = mv.misfit_many(Y, obs[3], weights=w, is_gpu=False, return_coef=True)
    b = mv.misfit_many(Y, np.tile(obs[3], (M, 1)), weights=np.tile(w, (M, 1)), is_gpu=False, return_coef=True)
    for x, y in zip(a, b):
        assert x.shape == y.shape and maxnorm(x, y) <= 1e-12
    wm = rs.uniform(0.5, 2.0, (M, B))
    c3, g3 = mv.misfit_many(Y, obs, weights=wm, is_gpu=False)
    assert maxnorm(0.5 * np.sum(wm * r * r, axis=1), c3) <= 1e-12
    assert maxnorm(np.einsum("mdb,mb->md", jac, wm * r), g3) <= 1e-12
    # one state vector: row 0 of misfit_many
    one = mv.misfit(Y[0], obs[0], weights=w, gauss_newton=True, return_coef=True)
    many = mv.misfit_many(Y[:1], obs[0], weights=w, is_gpu=False, gauss_newton=True, return_coef=True)
    assert len(one) == 4 and np.ndim(one[0]) == 0
    assert one[1].shape == (D,) and one[2].shape == (D, D) and one[3].shape == (P,)
    for x, y in zip(one, many):
        assert np.array_equal(x, y[0])
    assert np.ndim(mv.misfit(Y[0], obs[0], do_deriv=False)) == 0


def test_hessian_many_takes_the_projected_coefficients(mv_case):
    _, mv, Y, obs, _ = mv_case
    Y, obs = Y[:5], obs[:5]
    w = np.random.RandomState(5).uniform(0.5, 2.0, obs.shape)
    fwd = mv.predict_many(Y, is_gpu=False)
    coef = mv.misfit_many(Y, obs, weights=w, is_gpu=False, do_deriv=False, return_coef=True)[1]
    ref = mv.hessian_many(Y, is_gpu=False, weights=w * (fwd - obs))
    got = mv.hessian_many(Y, is_gpu=False, coef=coef)
    assert got.shape == ref.shape == (5, 10, 10)
    assert maxnorm(ref, got) <= 1e-12


def test_bad_arguments_raise(mv_case):
    _, mv, Y, obs, _ = mv_case
    Y, obs = Y[:4], obs[:4]
    B = obs.shape[1]
    for is_gpu in (False, True):             # the shapes are checked before anything touches a device
        with pytest.raises(ValueError):
            mv.misfit_many(Y, obs[:3], is_gpu=is_gpu)
        with pytest.raises(ValueError):
            mv.misfit_many(Y, obs[0, :-1], is_gpu=is_gpu)
        with pytest.raises(ValueError):
            mv.misfit_many(Y, obs, weights=np.ones(B + 1), is_gpu=is_gpu)
        with pytest.raises(ValueError):
            mv.misfit_many(Y, obs, weights=np.ones((3, B)), is_gpu=is_gpu)
        with pytest.raises(ValueError):
            mv.misfit_many(Y, obs, weights=np.ones((4, B)), is_gpu=is_gpu, gauss_newton=True)
    with pytest.raises(ValueError):
        mv.misfit(Y[:2], obs[0])
    with pytest.raises(ValueError):
        mv.misfit(Y[0], obs[:1])
    with pytest.raises(ValueError):
        mv.hessian_many(Y, is_gpu=False, weights=np.ones((4, B)), coef=np.ones((4, mv.n_pcs)))
    with pytest.raises(ValueError):
        mv.hessian_many(Y, is_gpu=False, coef=np.ones((4, mv.n_pcs + 1)))


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("cu", [256, 8])
def test_launch_plan(prec, cu):
    """misfit_kernel: 4 waves x 16 rows = 64 rows per item over all bands, 4 workgroups per CU."""
    first = _lib.launch_plan("misfit", prec, 1, n_pcs=12, n_bands=2101, compute_units=cu)
    assert first == dict(kernel="misfit", rows_per_item=64, items=1, workgroups=1, rest_items=0, rest_workgroups=0)
    cap, rpi = 4 * cu, 64
    one_round = cap * rpi
    for rows in (1, one_round - 1, one_round, one_round + 1, 3 * one_round, 3 * one_round + 1):
        p = _lib.launch_plan("misfit", prec, rows, n_pcs=3, n_bands=33, compute_units=cu)
        assert p["kernel"] == "misfit" and p["rows_per_item"] == rpi
        assert p["items"] == -(-rows // rpi)
        assert 1 <= p["workgroups"] <= min(p["items"], cap)
        assert p["rest_items"] == 0 and p["rest_workgroups"] == 0
    assert _lib.launch_plan("misfit", prec, one_round, n_pcs=3, n_bands=33, compute_units=cu)["workgroups"] == cap
    past = _lib.launch_plan("misfit", prec, one_round + 1, n_pcs=3, n_bands=33, compute_units=cu)
    assert past["items"] == cap + 1 > past["workgroups"]
    # balanced rounds: no workgroup is left with a whole extra round
    assert -(-past["items"] // past["workgroups"]) == 2
    with pytest.raises(_lib.GpuPredictError):          # as gp_mv_misfit_device
        _lib.launch_plan("misfit", prec, 1000, n_pcs=17, n_bands=33, compute_units=cu)
    with pytest.raises(_lib.GpuPredictError):
        _lib.launch_plan("misfit", prec, 1000, n_pcs=3, n_bands=0, compute_units=cu)
