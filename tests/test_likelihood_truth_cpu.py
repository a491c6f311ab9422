"""The 80-bit truth of likelihood_cases.py and its case list, validated without a GPU.

The truth reproduces the committed results of the reference (training_objective.npz); for EVERY case of the list the
reference's numpy route (oracle/gp_oracle.py) and a plain float64 Gauss-Jordan elimination without pivoting (the
kernels' algorithm, a dozen lines of numpy here) meet the bound K kappa u with K = 8 that test_likelihood_gpu.py holds
the kernels to.  A case the reference itself cannot meet may not be in the list; a GPU failure on a case that passes
here is the kernel's, not the algorithm's.  Measured on the CPU: the numpy route's worst ratios are 1.37 kappa u (gradient,
N = 1), 1.32 (invQt), 0.73 (invQ), 0.44 (cost); below 0.53 from N = 7 up."""
import numpy as np
import pytest

import likelihood_cases as lc
from oracle import gp_oracle

from conftest import load_golden

IDS = [lc.key_id(k) for k in lc.CASE_KEYS]


def test_case_list_is_the_one_the_kernels_are_tested_on():
    assert len(lc.CASE_KEYS) == 2 * (20 + 7) + 4 and len(set(lc.CASE_KEYS)) == len(lc.CASE_KEYS)
    seen = {lc.instance(*lc.case(k)[0].shape) for k in lc.CASE_KEYS}
    assert seen == {"%s<%d>" % (f, dm) for f in ("mfma", "workspace+grad") for dm in (4, 8, 12, 16)}
    for n, d in lc.MFMA_SHAPES + lc.WORKSPACE_SHAPES:                      # the -9 cases are the ill-conditioned ones
        assert lc.truth_of((n, d, -9))["cond"] >= lc.truth_of((n, d, -4))["cond"]
    assert max(lc.truth_of((n, d, -9))["cond"] for n, d in lc.MFMA_SHAPES + lc.WORKSPACE_SHAPES) > 1e6


def test_truth_reproduces_the_committed_reference_results():
    g = load_golden("training_objective")
    for k in range(3):
        lc.check(lc.truth_of("smooth%d" % k), g["smooth_loglik"][k], g["smooth_grad"][k], label="golden smooth%d" % k)
    tr = lc.truth_of("prosail_pc0")
    assert 1e7 < tr["cond"] < 1e8
    lc.check(tr, g["prosail_pc0_loglik"], g["prosail_pc0_grad"], label="golden prosail_pc0")


@pytest.mark.parametrize("key", lc.CASE_KEYS, ids=IDS)
def test_reference_numpy_route_meets_the_bound(key):
    X, t, theta = lc.case(key)
    pl = gp_oracle.prepare_likelihood(X, t, theta)
    lc.check(lc.truth_of(key), gp_oracle.loglikelihood(X, t, theta), gp_oracle.partial_devs(X, t, theta),
             pl["invQ"], pl["invQt"], label="numpy " + lc.key_id(key))


def gauss_jordan_objective(X, t, theta):
    """cost, grad, invQ, invQt in float64: in-place Gauss-Jordan without pivoting, logdet from the pivots."""
    N, D = X.shape
    e = np.exp(theta)
    dl2 = (X[:, None, :] - X[None, :, :]) ** 2
    Z = e[D] * np.exp(-0.5 * (dl2 @ e[:D]))
    A = Z + e[D + 1] * np.eye(N)
    logdet = 0.0
    for k in range(N):
        p = A[k, k]
        logdet += np.log(p)
        row, col = A[k] / p, A[:, k].copy()
        A -= np.outer(col, row)
        A[k], A[:, k], A[k, k] = row, -col / p, 1.0 / p
    a = A @ t
    c = (np.outer(a, a) - A) * Z
    grad = np.concatenate([e[:D] / 4 * np.einsum("ij,ijd->d", c, dl2), [-0.5 * c.sum(), 0.5 * e[D + 1] * (np.trace(A) - a @ a)]])
    return 0.5 * logdet + 0.5 * (t @ a) + 0.5 * N * np.log(2 * np.pi), grad, A, a


@pytest.mark.parametrize("key", lc.CASE_KEYS, ids=IDS)
def test_float64_gauss_jordan_meets_the_bound(key):
    lc.check(lc.truth_of(key), *gauss_jordan_objective(*lc.case(key)), label="gauss-jordan " + lc.key_id(key))


def test_the_measure_sees_one_wrong_element():
    """One element of the inverse off by 1e-9 of the largest, one gradient component off by 1e-9 of its terms: far
    above 8 kappa u at cond 238, whatever the other entries do."""
    key = (24, 9, -4)
    tr = lc.truth_of(key)
    invQ = tr["invQ"].astype(np.float64)
    invQ[17, 3] += 1e-9 * np.max(np.abs(invQ))
    grad = tr["grad"].astype(np.float64)
    grad[4] += 1e-9 * float(tr["G"][4])
    r = lc.ratios(tr, float(tr["cost"]), grad, invQ, tr["invQt"].astype(np.float64))
    assert r["invQ"] > 1e3 and r["grad"] > 1e3 and r["cost"] <= 1 and r["invQt"] <= 1
    one = lc.truth_of((1, 1, -4))
    assert np.all(one["G"][:1] == 0) and lc.ratios(one, float(one["cost"]), np.array([1e-300, *one["grad"][1:].astype(np.float64)]))["grad"] == np.inf
