"""Seeded inputs, the longdouble truth and the a-priori bounds shared by test_series_joint_cpu.py and
test_series_joint_gpu.py (not a test module).

Matrices, gradients and states are newton_cases.seeded(D, T * M, ...) reshaped to (T, M, ...): all dates share one set
of column scales, and the prior is that case's.  The process noise is prior_cases.noise(D, True, ...); W is its
longdouble inverse, symmetrised and rounded to the case's dtype.  Everything is rounded to the dtype before anything
is formed from it: the truth works from the inputs as the code under test is given them.

The truth is the assembled (T D) x (T D) system in longdouble: H' with the diagonal blocks A_t (+ P) (+ W) (+ W)
(+ damping) and the off-diagonal blocks -W, g' = grad_t (+ P (x_0 - xp)) + W (x_t - x_{t-1}) - W (x_{t+1} - x_t), its
Cholesky factor R (newton_cases.cholesky_ld) and, for the covariance, C = H^-1 (prior_cases.inverse_ld).

There is no free tolerance.  With u = 2^-53 and D the block size (the matrix has half-bandwidth 2 D - 1, so every
chain of the factorisation and of the substitutions has at most 2 D terms: the project's Cholesky constant with 2 D
for D),

    |H' step + g'| <= 2 (3 * 2 D + 8) u |R| |R|^T |step|
                      + (2 D + 2) u (|grad| + |P| |x_0 - xp| + |W| |x_t - x_{t-1}| + |W| |x_{t+1} - x_t|)
                      + 2^-24 |H'| |step|                                                 (float32 results only)
    |Sigma^_t - Sigma_t| <= max(B, B^T),   B = 2 (3 * 2 D + 8) u (|C| |R| |R|^T |C|)_tt + 1/2 spacing_T(|Sigma^_t|)
                                                                                          (the last: float32 only)
    sigma: posterior_cases.sigma_bound on Sigma_t and B.

Worst error over bound measured with these cases (D in {1, 3, 11, 16, 17, 32} x T in {1, 2, 3, 5}, T <= 2 at D = 32,
full-rank and rank-deficient matrices, both dampings, lambda in {1e-3, 1, 1e3}, shared and per-pixel prior and W):
    numpy branch (float64 out):  step 0.19,  cov 0.070,  sigma 0.068
    device:                      printed by test_series_joint_gpu.py (not measured when this was written)
"""
import numpy as np

import newton_cases as nc
import posterior_cases as pc
import prior_cases as prc

LD = nc.LD
U = LD(2) ** -53
DIMS = [1, 3, 11, 16, 17, 32]
DATES = [1, 2, 3, 5]
LAMBDAS = nc.LAMBDAS


def shapes():
    """(D, T): every block size with every series length, T <= 2 at D = 32 (the longdouble truth stays cheap)."""
    return [(D, T) for D in DIMS for T in DATES if D < 32 or T <= 2]


def sym(a):
    """The symmetric matrices whose lower triangles are those of ``a`` (..., D, D)."""
    return np.tril(a) + np.swapaxes(np.tril(a, -1), -1, -2)


def precision_of(Q, dtype):
    """W = Q^-1 in longdouble, symmetrised, rounded to ``dtype``; Q (D, D) or (M, D, D)."""
    Qm = sym(np.asarray(Q).astype(LD).reshape((-1,) + Q.shape[-2:]))
    R, ok = nc.cholesky_ld(Qm)
    assert ok.all()
    W = sym(prc.inverse_ld(R)).astype(dtype)
    return np.ascontiguousarray(W.reshape(Q.shape))


def seeded(D, T, M, dtype, full_rank=True, per_pixel=False, bounds=False, seed=1):
    """dict(x (T, M, D), grad, A (T, M, D, D), prior, W, Q, bounds) of ``dtype``; ``per_pixel`` makes the prior
    (prior_cases.row_priors) and the noise the pixel's own."""
    base = nc.seeded(D, T * M, full_rank, dtype, seed=seed, prior=True, bounds=bounds)
    case = dict(x=np.ascontiguousarray(base["x"].reshape(T, M, D)), grad=np.ascontiguousarray(base["grad"].reshape(T, M, D)),
                A=np.ascontiguousarray(base["A"].reshape(T, M, D, D)), prior=base["prior"], bounds=base["bounds"])
    if per_pixel:
        case["prior"] = prc.row_priors(dict(x=case["x"][0], prior=base["prior"]))["prior"]
    case["Q"] = prc.noise(D, full_rank, dtype, M if per_pixel else None)
    case["W"] = precision_of(case["Q"], dtype)
    return case


def pixels(case, sel):
    """The pixels ``sel`` (a slice) of a case."""
    out = dict(case, x=np.ascontiguousarray(case["x"][:, sel]), grad=np.ascontiguousarray(case["grad"][:, sel]),
               A=np.ascontiguousarray(case["A"][:, sel]))
    x0, P = case["prior"]
    out["prior"] = (np.ascontiguousarray(x0[sel]) if x0.ndim == 2 else x0, np.ascontiguousarray(P[sel]) if P.ndim == 3 else P)
    for k in ("W", "Q"):
        out[k] = np.ascontiguousarray(case[k][sel]) if case[k].ndim == 3 else case[k]
    return out


def repeated(case):
    """The case with its shared prior and W repeated for every pixel."""
    T, M, D = case["x"].shape
    x0, P = case["prior"]
    rep = lambda a, shape: np.ascontiguousarray(np.broadcast_to(a, shape))
    return dict(case, prior=(rep(x0, (M, D)), rep(P, (M, D, D))), W=rep(case["W"], (M, D, D)))


def assemble(case, lam=None, damping="diagonal", with_prior=True):
    """(H' (M, T D, T D), g' (M, T D), a (M, T D)) in longdouble: the matrix (lower triangles mirrored), the right-hand
    side and the sum of the absolute values of the terms g' is formed from.  ``lam`` None: no damping."""
    x, g, A = (case[k].astype(LD) for k in ("x", "grad", "A"))
    T, M, D = x.shape
    W = np.broadcast_to(case["W"].astype(LD), (M, D, D))
    Ws = sym(W)
    n = T * D
    H, gp, ab = np.zeros((M, n, n), LD), np.zeros((M, n), LD), np.zeros((M, n), LD)
    idx = np.arange(D)
    mv = lambda Mx, v: np.einsum("mij,mj->mi", Mx, v)
    for t in range(T):
        s = slice(t * D, (t + 1) * D)
        Ht, gt, at = sym(A[t]), g[t].copy(), np.abs(g[t])
        if t == 0 and with_prior and case["prior"] is not None:
            x0, P = (a.astype(LD) for a in case["prior"])
            Pm = np.broadcast_to(P, (M, D, D))
            Ht = Ht + sym(Pm)
            gt, at = gt + mv(Pm, x[0] - x0), at + mv(np.abs(Pm), np.abs(x[0] - x0))
        if t > 0:
            d = x[t] - x[t - 1]
            Ht = Ht + Ws
            gt, at = gt + mv(W, d), at + mv(np.abs(W), np.abs(d))
        if t < T - 1:
            d = x[t + 1] - x[t]
            Ht = Ht + Ws
            gt, at = gt - mv(W, d), at + mv(np.abs(W), np.abs(d))
        if lam is not None:
            diag = Ht[:, idx, idx]
            lm = np.broadcast_to(np.asarray(lam).astype(LD), (M,))
            Ht[:, idx, idx] = diag + lm[:, None] * (diag if damping == "diagonal" else LD(1))
        H[:, s, s], gp[:, s], ab[:, s] = Ht, gt, at
        if t > 0:
            b = slice((t - 1) * D, t * D)
            H[:, s, b] = -W
            H[:, b, s] = -np.transpose(W, (0, 2, 1))
    return H, gp, ab


def flat(a):
    """(T, M, D) -> (M, T D)."""
    T, M, D = a.shape
    return np.transpose(a, (1, 0, 2)).reshape(M, T * D)


def step_check(case, lam, damping, step, stored_f32):
    """Asserts the residual bound of the module docstring on every pixel; returns the worst residual over bound."""
    T, M, D = step.shape
    H, gp, ab = assemble(case, lam, damping)
    R, ok = nc.cholesky_ld(H)
    assert ok.all(), "the longdouble factorisation fails"
    s = flat(step.astype(LD))
    mv = lambda Mx, v: np.einsum("mij,mj->mi", Mx, v)
    res = np.abs(mv(H, s) + gp)
    bound = 2 * (3 * 2 * D + 8) * U * mv(pc.gram(R), np.abs(s)) + (2 * D + 2) * U * ab
    if stored_f32:
        bound = bound + LD(2) ** -24 * mv(np.abs(H), np.abs(s))
    ratio = float(np.max(res / np.maximum(bound, np.finfo(LD).tiny)))
    assert np.all(res <= bound), ("step", ratio)
    return ratio


def cov_truth(case, with_prior=True):
    """(C (M, T D, T D), Bfull (M, T D, T D)) in longdouble: H^-1 of the undamped matrix and
    2 (3 * 2 D + 8) u |C| |R| |R|^T |C|."""
    D = case["x"].shape[2]
    H, _, _ = assemble(case, None, with_prior=with_prior)
    R, ok = nc.cholesky_ld(H)
    assert ok.all(), "the longdouble factorisation fails"
    C = prc.inverse_ld(R)
    aC = np.abs(C)
    return C, 2 * (3 * 2 * D + 8) * U * np.matmul(np.matmul(aC, pc.gram(R)), aC)


def cov_check(truth, cov, sigma, stored_f32):
    """Asserts both bounds on every date and pixel; returns the worst error over bound of cov and of sigma."""
    C, Bfull = truth
    T, M, D = sigma.shape
    worst, sworst = 0.0, 0.0
    idx = np.arange(D)
    for t in range(T):
        s = slice(t * D, (t + 1) * D)
        Ct, B = C[:, s, s], Bfull[:, s, s]
        if stored_f32:
            B = B + 0.5 * np.spacing(np.abs(cov[t]).astype(np.float32)).astype(LD)
        B = np.maximum(B, np.transpose(B, (0, 2, 1)))
        err = np.abs(cov[t].astype(LD) - Ct)
        worst = max(worst, float(np.max(err / np.maximum(B, np.finfo(LD).tiny))))
        assert np.all(err <= B), ("cov", t, worst)
        sb = pc.sigma_bound(Ct, B, sigma[t], stored_f32)
        serr = np.abs(sigma[t].astype(LD) - np.sqrt(Ct[:, idx, idx]))
        sworst = max(sworst, float(np.max(serr / np.maximum(sb, np.finfo(LD).tiny))))
        assert np.all(serr <= sb), ("sigma", t, sworst)
    return worst, sworst


def planted(D, T):
    """pixel -> (t, k, A_kk): posterior_cases.planted's rows and indices (a case of 65 pixels), on date 0 and on later
    dates; its finite negative entry is -1e30 here, which no W on the diagonal outweighs."""
    out = {}
    for n, (m, (k, v)) in enumerate(sorted(pc.planted(D).items())):
        out[m] = ((0, T - 1, T // 2)[n % 3], k, -1e30 if v == -2.0 else v)
    return out


def same(a, b):
    nc.same(np.asarray(a), np.asarray(b))
