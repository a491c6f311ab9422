"""Moments under Gaussian inputs without a GPU: the numpy branch against the definition (tensor Gauss-Hermite quadrature
of the oracle's predict), against the longdouble truth inside the gates of moments_cases.py down to Sigma scaled by
1e-12, its limits and invalid inputs, the three public wrappers, the launch plan and the argument errors of the C
entry.  Every test here needs ``_moments_numpy``, the methods or the entry, none of which exist before this feature."""
import ctypes
import os
import re

import numpy as np
import pytest

import moments_cases as mc

from gp_emulator_amd import _lib, _moments_numpy as mn, perband
from gp_emulator_amd.GaussianProcess import GaussianProcess
from gp_emulator_amd.multivariate_gp import MultivariateEmulator
from oracle import gp_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PQ = [[0, 0], [0, 1], [1, 1]]


def oracle_predict(m, t):
    return gp_oracle.cpu_predict(m["inputs"], np.log(m["expX"]), m["invQ"], m["invQt"], t)


# ---- the definition ------------------------------------------------------------------------------------

def test_numpy_branch_against_the_definition():
    """D = 3, N = 20, two emulators and their cross pair, input standard deviations of about 0.2: M, V_pp, V_pq, Ev and
    the expected gradient within 1e-10 b of 48-node-per-axis tensor Gauss-Hermite quadrature of the oracle's mean,
    variance and gradient (measured: 2.5e-12, printed)."""
    d, n = 3, 20
    ems = [mc.emulator(n, d, 0), mc.emulator(n, d, 1)]
    m, S = mc.rows(1, d)
    t, w = np.polynomial.hermite_e.hermegauss(48)
    w = w / w.sum()
    C = np.linalg.cholesky(S[0])
    T = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, d)
    W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).reshape(-1)
    X = m[0] + T @ C.T
    mu, var, grad = zip(*(oracle_predict(e, X) for e in ems))
    Mq = [float(W @ u) for u in mu]
    mean, egrad, cov, evar, info = mn.moments_pairs_numpy(*mc.stack(ems), m, S, PQ)
    assert info[0] == 0
    b = [e["expX"][d] for e in ems]
    worst = 0.0
    for k, (p, q) in enumerate(PQ):
        worst = max(worst, abs(cov[0, k] - float(W @ ((mu[p] - Mq[p]) * (mu[q] - Mq[q])))) / np.sqrt(b[p] * b[q]))
    for e in range(2):
        worst = max(worst, abs(mean[0, e] - Mq[e]) / b[e], abs(evar[0, e] - float(W @ var[e])) / b[e],
                    float(np.max(np.abs(egrad[0, e] - W @ grad[e]))) / b[e])
    print("worst difference relative to b: %.3g" % worst)
    assert worst <= 1e-10


# ---- the truth -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [1.0, 1e-2, 1e-4, 1e-6])
@pytest.mark.parametrize("n,d", [(37, 3), (60, 5)])
def test_numpy_branch_and_kernel_form_inside_the_gate(n, d, s):
    """Both yardsticks stay far below the cap at every scale of Sigma (so the gates are theirs, not the cap's), and the
    numpy branch alone passes the gate."""
    args = mc.stack([mc.emulator(n, d, k) for k in range(2)])
    m, S = mc.rows(3, d, s)
    key = ("cpu", n, d, s)
    tr, g = mc.truth(key, *args, m, S, PQ), mc.gates(key, *args, m, S, PQ)
    print(key, "a", g["a"], "b", g["b"], "S / |V| up to %.3g" % float((tr["S_cov"] / np.abs(tr["cov"])).max()))
    assert not mc.within(mn.moments_pairs_numpy(*args, m, S, PQ), tr, g["gate"])
    assert max(max(g["a"].values()), max(g["b"].values())) <= mc.CAP / mc.MARGIN
    assert np.all(tr["cov"][:, [0, 2]] > 0)


def test_the_naive_form_is_no_truth():
    """alpha' Q alpha - M^2 in LONGDOUBLE is further from the truth at s = 1e-4 than the float64 numpy branch by orders
    of magnitude: the case the stable form exists for."""
    n, d = 60, 5
    args = mc.stack([mc.emulator(n, d, k) for k in range(2)])
    m, S = mc.rows(1, d, 1e-4)
    tr = mc.truth(("cpu", "naive"), *args, m, S, PQ)
    cov = mn.moments_pairs_numpy(*args, m, S, PQ)[2]
    naive = float(mc.naive_ld(args[0], args[1], args[2], m[0], S[0], 0, 1))
    t = float(tr["cov"][0, 1])
    print("relative errors: naive longdouble %.3g, stable float64 %.3g" % (abs(naive / t - 1), abs(cov[0, 1] / t - 1)))
    assert abs(cov[0, 1] / t - 1) <= 1e-9 and abs(naive / t - 1) >= 1e3 * abs(cov[0, 1] / t - 1)


# ---- limits and invalid inputs ---------------------------------------------------------------------------

def test_sigma_zero_is_predict():
    n, d = 37, 3
    ems = [mc.emulator(n, d, k) for k in range(2)]
    expX, x, alpha, invQ = mc.stack(ems)
    m, _ = mc.rows(3, d)
    mean, egrad, cov, evar, info = mn.moments_pairs_numpy(expX, x, alpha, invQ, m, np.zeros((d, d)), PQ)
    assert np.all(cov == 0.0) and np.all(info == 0)
    for e in range(2):
        mu, var, deriv = oracle_predict(ems[e], m)
        k = gp_oracle.kernel_rows(x, np.log(expX[e]), m)                                   # (N, M)
        assert np.all(np.abs(mean[:, e] - mu) <= 1e-12 * np.abs(alpha[e][:, None] * k).sum(axis=0))
        assert np.all(np.abs(evar[:, e] - var) <= 1e-12 * (expX[e, d] + np.einsum("jl,jm,lm->m", np.abs(invQ[e]), k, k)))
        mag = expX[e, :d] * np.einsum("jm,jmd->md", np.abs(alpha[e][:, None] * k), np.abs(x[:, None, :] - m[None]))
        assert np.all(np.abs(egrad[:, e] - deriv) <= 1e-12 * mag)


def test_a_fixed_input_is_the_smaller_problem():
    """Sigma with a zero row and column: the (D - 1)-dimensional problem with that input fixed -- the emulator on the
    other inputs with alpha_j exp(-e_k (x_jk - m_k)^2 / 2) -- inside the gates of the full problem."""
    n, d, kf = 37, 4, 1
    ems = [mc.emulator(n, d, k) for k in range(2)]
    expX, x, alpha, invQ = mc.stack(ems)
    m, S = mc.rows(2, d)
    S[:, kf, :] = 0.0
    S[:, :, kf] = 0.0
    full = mn.moments_pairs_numpy(expX, x, alpha, invQ, m, S, PQ)
    assert np.all(full[4] == 0)
    tr = mc.truth(("cpu", "fixed"), expX, x, alpha, invQ, m, S, PQ)
    gate = mc.gates(("cpu", "fixed"), expX, x, alpha, invQ, m, S, PQ)["gate"]
    keep = [i for i in range(d) if i != kf]
    for r in range(2):
        c = np.exp(-0.5 * expX[:, kf, None] * (x[None, :, kf] - m[r, kf]) ** 2)           # (E, N)
        small = mn.moments_pairs_numpy(expX[:, keep + [d, d + 1]], x[:, keep], alpha * c,
                                       invQ * (c[:, :, None] * c[:, None, :]),
                                       m[r:r + 1, keep], S[r][np.ix_(keep, keep)], PQ)
        u = mc.U
        assert np.all(np.abs(small[0][0] - full[0][r]) <= 2 * gate["mean"] * u * tr["S_mean"][r].astype(np.float64))
        assert np.all(np.abs(small[2][0] - full[2][r]) <= 2 * gate["V"] * u * tr["S_cov"][r].astype(np.float64))
        assert np.all(np.abs(small[1][0] - full[1][r][:, keep]) <= 2 * gate["grad"] * u * tr["S_grad"][r].astype(np.float64)[:, keep])
        # Ev: b - sum invQ q q exp(delta) with q carrying the fixed factor is the smaller problem's sum with invQ c c
        assert np.all(np.abs(small[3][0] - full[3][r]) <= 2 * gate["Ev"] * u * tr["S_evar"][r].astype(np.float64))


def test_indefinite_and_non_finite_rows():
    n, d = 37, 3
    args = mc.stack([mc.emulator(n, d, k) for k in range(2)])
    m, S = mc.rows(5, d)
    clean = mn.moments_pairs_numpy(*args, m, S, PQ)
    m2, S2 = m.copy(), S.copy()
    S2[1] = np.diag([0.04, 0.01, -1e-4])                      # pivot 2 negative
    m2[2, 0] = np.nan
    S2[3, 2, 1] = np.inf
    S2[4, 0, 1] = np.nan                                      # the upper triangle is not read
    got = mn.moments_pairs_numpy(*args, m2, S2, PQ)
    assert list(got[4]) == [0, 3, -1, -1, 0]
    for o, c in zip(got[:4], clean[:4]):
        assert np.all(np.isnan(o[1:4])) and np.array_equal(o[[0, 4]], c[[0, 4]])
    # a non-finite emulator: its own results and pairs, nothing else
    e2 = args[0].copy()
    e2[1, 0] = np.inf
    got = mn.moments_pairs_numpy(e2, *args[1:], m, S, PQ)
    assert np.all(np.isnan(got[2][:, 1:])) and np.array_equal(got[2][:, 0], clean[2][:, 0])
    assert np.all(np.isnan(got[0][:, 1])) and np.array_equal(got[0][:, 0], clean[0][:, 0])


def test_rank_deficient_sigma():
    """Sigma = v v' (rank one): two zero columns in C, finite results, and the truth agrees."""
    n, d = 37, 3
    args = mc.stack([mc.emulator(n, d, k) for k in range(2)])
    m, _ = mc.rows(1, d)
    v = np.array([0.2, -0.1, 0.15])
    S = np.outer(v, v)[None]
    C, info = mn.psd_cholesky(S[0])
    assert info == 0 and np.all(C[:, 1:] == 0.0)
    tr, g = mc.truth(("cpu", "rank1"), *args, m, S, PQ), mc.gates(("cpu", "rank1"), *args, m, S, PQ)
    assert not mc.within(mn.moments_pairs_numpy(*args, m, S, PQ), tr, g["gate"])


# ---- the wrappers --------------------------------------------------------------------------------------

def gps_of(ems):
    out = []
    for m in ems:
        gp = GaussianProcess(m["inputs"], np.zeros(m["n"]))
        gp.theta, gp.invQt, gp.invQ = np.log(m["expX"]), m["invQt"], m["invQ"]
        out.append(gp)
    return out


def small_mv(n=37, d=3, P=3, K=40):
    ems = [mc.emulator(n, d, k) for k in range(P)]
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    mv.n_pcs = P
    mv.basis_functions = np.random.RandomState(77).standard_normal((P, K))
    mv.emulators = gps_of(ems)
    return mv, ems


def test_wrappers_numpy():
    n, d = 37, 3
    mv, ems = small_mv(n, d)
    gps = mv.emulators
    m, S = mc.rows(4, d, seed=5)
    args = (np.stack([np.exp(gp.theta) for gp in gps]),) + mc.stack(ems)[1:]
    mean, egrad, cov, evar, info = mn.moments_pairs_numpy(*args, m, S, mn.upper_pairs(3))
    r = perband.predict_uncertain_bands(gps, m, S, is_gpu=False)
    assert np.array_equal(r.mean, mean.T) and np.array_equal(r.var_state, cov[:, [0, 3, 5]].T)
    assert np.array_equal(r.var_emulator, evar.T) and np.array_equal(r.expected_grad, egrad.transpose(1, 0, 2))
    assert r.info.shape == (4,) and np.all(r.info == 0)
    one = gps[2].predict_uncertain(m, S)
    assert one.mean.shape == (4,) and one.expected_grad.shape == (4, d)
    assert np.array_equal(one.mean, r.mean[2]) and np.array_equal(one.var_emulator, r.var_emulator[2])
    # the multivariate emulator: brute-force beta' V beta, and predict_many at Sigma = 0
    s = mv.predict_uncertain(m, S, is_gpu=False, return_pc=True)
    B = mv.basis_functions
    V = np.zeros((4, 3, 3))
    for k, (p, q) in enumerate(mn.upper_pairs(3)):
        V[:, p, q] = V[:, q, p] = cov[:, k]
    assert np.array_equal(s.pc_cov, V) and np.array_equal(s.pc_mean, mean)
    brute = np.array([[B[:, k] @ V[r_] @ B[:, k] for k in range(40)] for r_ in range(4)])
    scale = np.einsum("pk,mpq,qk->mk", np.abs(B), np.abs(V), np.abs(B))
    assert np.all(np.abs(s.var_state - brute) <= 1e-14 * scale) and np.all(s.var_state > 0)
    assert np.all(np.abs(s.var_emulator - evar @ (B * B)) <= 1e-14 * (np.abs(evar) @ (B * B)))
    z = mv.predict_uncertain(m, np.zeros((d, d)), is_gpu=False)
    ref = mv.predict_many(m, is_gpu=False)
    assert z.mean.shape == (4, 40) and np.all(z.var_state == 0.0)
    mag = np.stack([np.abs(e["invQt"][:, None] * gp_oracle.kernel_rows(e["inputs"], np.log(e["expX"]), m)).sum(axis=0)
                    for e in ems]).T @ np.abs(B)
    assert np.all(np.abs(z.mean - ref) <= 1e-12 * mag)
    plain = mv.predict_uncertain(m, S, is_gpu=False)
    assert len(plain) == 4 and np.array_equal(plain.mean, s.mean)
    with pytest.raises(ValueError):
        gps[0].predict_uncertain(m, np.zeros((2, d, d)))


# ---- launch plan and error returns -----------------------------------------------------------------------

def test_launch_plan_arithmetic():
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    assert re.search(r"#define GP_OP_MOMENTS %d\b" % _lib.GP_OP_MOMENTS, text) and _lib.GP_OP_MOMENTS == 10
    plan_code = int(re.search(r"#define GP_PLAN_MOMENTS (\d+)", text).group(1))
    assert plan_code == 16 and _lib.PLAN_KERNELS[plan_code] == "moments" and _lib._PLAN_OPS["moments"] == _lib.GP_OP_MOMENTS
    wgs = {8: 2, 12: 2, 16: 1}                                    # workgroups per compute unit by instance
    for cu in (1, 8, 256):
        for n in (1, 37, 250, 512):
            for d in (1, 8, 9, 12, 13, 16):
                for rows, pairs in ((1, 1), (3, 78), (100000, 78), (1000, 2101)):
                    p = _lib.launch_plan("moments", np.float64, rows, n_train=n, n_inputs=d, n_emulators=pairs, compute_units=cu)
                    items = rows * pairs
                    cap = cu * wgs[8 if d <= 8 else 12 if d <= 12 else 16]
                    assert p == dict(kernel="moments", rows_per_item=1, items=items, workgroups=min(items, cap), rest_items=0,
                                     rest_workgroups=0)
    for bad in (dict(n_train=513, n_inputs=2), dict(n_train=10, n_inputs=17)):
        with pytest.raises(_lib.GpuPredictError, match="status -4"):
            _lib.launch_plan("moments", np.float64, 1, n_emulators=1, **bad)
    with pytest.raises(_lib.GpuPredictError, match="status -1"):
        _lib.launch_plan("moments", np.float64, 1, n_emulators=1, n_train=0, n_inputs=2)


def test_error_returns_without_a_device():
    lib = _lib.load()
    d = (ctypes.c_double * 8)()
    i = (ctypes.c_int32 * 8)()
    assert lib.gp_moments_batch_f64(None, 1, d, d, d, None, 1, 1, 1, d, d, 1, None, d, d, d, None, i) == -1
    assert lib.gp_last_error_string().decode() == "null context"
    ctx = _lib.Context.__new__(_lib.Context)                      # the binding's own checks come before the library
    ok = dict(expX=np.ones((2, 5)), inputs=np.zeros((5, 3)), invQt=np.ones((2, 5)), invQ=None, mean_in=np.zeros((4, 3)),
              cov_in=np.zeros((3, 3)))
    for bad in (dict(expX=np.ones((2, 4))), dict(invQt=np.ones((2, 4))), dict(mean_in=np.zeros((4, 2))),
                dict(cov_in=np.zeros((3, 3, 3))), dict(invQ=np.ones((2, 5, 4))), dict(pairs=[0, 1, 1])):
        with pytest.raises(ValueError):
            _lib.Context.moments_batch(ctx, **dict(ok, **bad))
