"""Moments under Gaussian inputs: emulators, the longdouble truth, numpy yardsticks and gates shared by
test_moments_cpu.py and test_moments_gpu.py (not a test module).

Truth.  The stable form of ``_moments_numpy`` (the docstring there) evaluated in np.longdouble from the float64
inputs: both factorisations, log1p, expm1, exp and every sum, written out here on its own.  It is NOT the naive
``alpha' Q alpha - M^2``: with Sigma scaled by 1e-8 that form, evaluated in longdouble, is already 1e-8 to 9e-6 away
from V in relative terms (``naive_ld`` below; test_moments_cpu.py shows it), so it can be no truth.  With each value comes S, the sum of the magnitudes of the terms
of its sum (for Ev including b; for the expected gradient the magnitudes pushed through |E^(1/2)| (I + |F| |F'|)).

Errors are in units of u S (u = 2^-53).  The gate of an output family (V, Ev, mean, grad) of a case is MARGIN x the
larger error of two float64 numpy evaluations against the truth, floor MARGIN, cap CAP -- the rule of sobol_cases.py:

    (a) ``_moments_numpy.moments_pairs_numpy``, the plain numpy branch;
    (b) ``kernel_form``: the kernels' summation restated -- in moments_pair_kernel a lane per column l = lane + 256 step
        adds its terms over (step, j) ascending, the 64 lanes of a wave are added by the xor butterfly 32, 16, .. 1, the
        four waves as ((0 + 1) + 2) + 3; in moments_mean_kernel a lane per j = lane + 64 step and the butterfly.

The yardsticks never come from the device.
"""
import numpy as np

import sobol_cases as sc

from gp_emulator_amd import _moments_numpy as mn

LD = np.longdouble
U = 2.0 ** -53
MARGIN = 16
CAP = 1024
FAMILIES = ("V", "Ev", "mean", "grad")


# ---- emulators and rows ------------------------------------------------------------------------------
_emulators = {}


def emulator(n, d, seed=0):
    """sobol_cases.emulator (trained-like, nugget 1e-5) with its invQ (N, N)."""
    key = (n, d, seed)
    if key not in _emulators:
        m = dict(sc.emulator(n, d, seed))
        X, ee, bb = m["inputs"], m["expX"][:d], m["expX"][d]
        diff = X[:, None, :] - X[None, :, :]
        Q = bb * np.exp(-0.5 * ((diff * diff) @ ee)) + 1e-5 * np.eye(n)
        m["invQ"] = np.linalg.inv(Q)
        _emulators[key] = m
    return _emulators[key]


def stack(ems):
    """(expX (E, D + 2), inputs, invQt (E, N), invQ (E, N, N)) of emulators of one shape."""
    return (np.stack([m["expX"] for m in ems]), ems[0]["inputs"], np.stack([m["invQt"] for m in ems]),
            np.stack([m["invQ"] for m in ems]))


def rows(n_rows, d, s=1.0, seed=0):
    """(m (M, D), Sigma (M, D, D)): seeded means inside the unit box and full covariances with standard deviations of
    about 0.2 s."""
    rs = np.random.RandomState(4100 + 17 * d + seed)
    m = rs.uniform(0.2, 0.8, size=(n_rows, d))
    A = rs.standard_normal((n_rows, d, d))
    S0 = 0.04 * (A @ A.transpose(0, 2, 1) / d + 0.1 * np.eye(d))
    return m, (s * s) * S0


# ---- the truth ---------------------------------------------------------------------------------------
def psd_cholesky_ld(S):
    D = S.shape[0]
    C = np.zeros((D, D), LD)
    for k in range(D):
        d = S[k, k] - (C[k, :k] * C[k, :k]).sum()
        tol = LD(64 * U) * S[k, k]
        if abs(d) <= tol:
            continue
        if not d > 0:
            return C, k + 1
        C[k, k] = np.sqrt(d)
        for j in range(k + 1, D):
            C[j, k] = (S[j, k] - (C[j, :k] * C[k, :k]).sum()) / C[k, k]
    return C, 0


def scale_class_ld(C, e):
    D = C.shape[0]
    A = np.array([[(C[:, i] * e * C[:, k]).sum() for k in range(D)] for i in range(D)], dtype=LD)
    L, Y = np.zeros((D, D), LD), np.zeros((D, D), LD)
    R = (np.sqrt(e)[:, None] * C).T
    ld = LD(0)
    for k in range(D):
        d = A[k, k] - (L[k, :k] * L[k, :k]).sum()
        ld += np.log1p(d)
        L[k, k] = np.sqrt(LD(1) + d)
        for j in range(k + 1, D):
            L[j, k] = (A[j, k] - (L[j, :k] * L[k, :k]).sum()) / L[k, k]
        Y[k] = (R[k] - (L[k, :k, None] * Y[:k]).sum(axis=0)) / L[k, k]
    return Y.T, ld / LD(2)


def _matvec_rows(a, F):
    """a (N, D) times F (D, D) in longdouble without BLAS."""
    return (a[:, :, None] * F[None, :, :]).sum(axis=1)


_truths = {}


def truth(key, expX, x, alpha, invQ, m_in, S_in, pairs=None):
    """dict(mean, S_mean (M, E), grad, S_grad (M, E, D), cov, S_cov (M, P), evar, S_evar (M, E) or None, info) in
    longdouble; ``key`` names the call (cached).  Rows with info != 0 hold NaN."""
    if key in _truths:
        return _truths[key]
    expX, alpha = np.atleast_2d(expX), np.atleast_2d(alpha)
    E, (N, D) = expX.shape[0], x.shape
    m_in, S_in = mn.rows_arrays(m_in, S_in, D)
    pairs = mn.pairs_array(pairs, E)
    M, P = m_in.shape[0], len(pairs)
    nan = lambda *shape: np.full(shape, np.nan, LD)                                              # noqa: E731
    out = dict(mean=nan(M, E), S_mean=nan(M, E), grad=nan(M, E, D), S_grad=nan(M, E, D), cov=nan(M, P), S_cov=nan(M, P),
               evar=None if invQ is None else nan(M, E), S_evar=None if invQ is None else nan(M, E),
               info=np.zeros(M, np.int32))
    xl, al = x.astype(LD), alpha.astype(LD)
    low = np.tril_indices(D)
    for r in range(M):
        if not (np.isfinite(m_in[r]).all() and np.isfinite(S_in[r][low]).all()):
            out["info"][r] = -1
            continue
        C, out["info"][r] = psd_cholesky_ld(S_in[r].astype(LD))
        if out["info"][r]:
            continue
        u = xl - m_in[r].astype(LD)
        per = {}
        for e in range(E):
            ee, b = expX[e, :D].astype(LD), LD(expX[e, D])
            F, ld = scale_class_ld(C, ee)
            z = np.sqrt(ee) * u
            f = _matvec_rows(z, F)
            hf = (f * f).sum(axis=1) / LD(2)
            q = b * np.exp(-ld - (z * z).sum(axis=1) / LD(2) + hf)
            w = al[e] * q
            per[e] = (hf, q, w, ld)
            h, ha = (w[:, None] * z).sum(axis=0), np.abs(w[:, None] * z).sum(axis=0)
            out["mean"][r, e], out["S_mean"][r, e] = w.sum(), np.abs(w).sum()
            out["grad"][r, e] = np.sqrt(ee) * (h - F @ (F.T @ h))
            out["S_grad"][r, e] = np.sqrt(ee) * (ha + np.abs(F) @ (np.abs(F.T) @ ha))
        for k, (p, q_) in enumerate(pairs):
            ep, eq = expX[p, :D].astype(LD), expX[q_, :D].astype(LD)
            Fs, lds = scale_class_ld(C, ep + eq)
            (hf_p, q_p, w_p, ld_p), (hf_q, q_q, w_q, ld_q) = per[p], per[q_]
            rs = LD(1) / np.sqrt(ep + eq)
            gp, gq = _matvec_rows(ep * rs * u, Fs), _matvec_rows(eq * rs * u, Fs)
            delta = np.zeros((N, N), LD)
            for d in range(D):
                t = gp[:, None, d] + gq[None, :, d]
                delta += t * t
            delta = delta / LD(2) - hf_p[:, None] - hf_q[None, :] + (ld_p + ld_q - lds)
            terms = np.multiply.outer(w_p, w_q) * np.expm1(delta)
            out["cov"][r, k], out["S_cov"][r, k] = terms.sum(), np.abs(terms).sum()
            if invQ is not None and p == q_:
                terms = invQ[p].astype(LD) * np.multiply.outer(q_p, q_p) * np.exp(delta)
                out["evar"][r, p] = LD(expX[p, D]) - terms.sum()
                out["S_evar"][r, p] = LD(expX[p, D]) + np.abs(terms).sum()
    _truths[key] = out
    return out


def naive_ld(expX, x, alpha, m, S, p, q):
    """Cov[mu_p, mu_q] of one row as ``alpha_p' Q alpha_q - M_p M_q`` in longdouble, Q and M from the textbook formulas
    (determinants and inverses of I + Sigma E): what the stable form replaces."""
    D = x.shape[1]
    xl, Sl, ml = x.astype(LD), S.astype(LD), m.astype(LD)

    def solve(A, B):      # Gauss-Jordan with partial pivoting, longdouble; returns (A^-1 B, det A)
        A, B = A.copy(), B.copy()
        n, det = A.shape[0], LD(1)
        for k in range(n):
            i = k + int(np.argmax(np.abs(A[k:, k])))
            if i != k:
                A[[k, i]], B[[k, i]], det = A[[i, k]], B[[i, k]], -det
            det *= A[k, k]
            B[k], A[k] = B[k] / A[k, k], A[k] / A[k, k]
            for j in range(n):
                if j != k:
                    B[j], A[j] = B[j] - A[j, k] * B[k], A[j] - A[j, k] * A[k]
        return B, det

    def expect(e, b, c):  # E[b exp(-(x - c)' E (x - c) / 2)] for the points c (.., D)
        W, det = solve(np.eye(D, dtype=LD) + Sl * e[None, :], Sl)          # (I + Sigma E)^-1 Sigma
        P = np.diag(e) - (e[:, None] * W) * e[None, :]                      # (E^-1 + Sigma)^-1
        v = c - ml
        return b * np.exp(-np.einsum("...i,ij,...j->...", v, P, v) / LD(2)) / np.sqrt(det)

    ep, eq = expX[p, :D].astype(LD), expX[q, :D].astype(LD)
    Mp = (alpha[p].astype(LD) * expect(ep, LD(expX[p, D]), xl)).sum()
    Mq = (alpha[q].astype(LD) * expect(eq, LD(expX[q, D]), xl)).sum()
    es = ep + eq
    c = (ep * xl[:, None, :] + eq * xl[None, :, :]) / es
    diff = xl[:, None, :] - xl[None, :, :]
    Q = np.exp(-((ep * eq / es) * diff * diff).sum(axis=2) / LD(2)) * expect(es, LD(expX[p, D]) * LD(expX[q, D]), c)
    return alpha[p].astype(LD) @ Q @ alpha[q].astype(LD) - Mp * Mq


# ---- yardsticks --------------------------------------------------------------------------------------
def _butterfly(v):
    """(..., 64) -> (...): the xor-shuffle tree of a wave."""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ off]
    return v[..., 0]


def _lane_sum(T, lanes):
    """The sum of T (N, ...) over its first axis as the kernels take it: lane = index mod ``lanes`` adds its own
    entries ascending, a wave's 64 lanes go through the butterfly, the waves are added in order."""
    N = T.shape[0]
    acc = np.zeros((lanes,) + T.shape[1:])
    for i0 in range(0, N, lanes):
        n = min(lanes, N - i0)
        acc[:n] += T[i0:i0 + n]
    wv = _butterfly(np.moveaxis(acc.reshape((lanes // 64, 64) + T.shape[1:]), 1, -1))
    total = wv[0]
    for k in range(1, lanes // 64):
        total = total + wv[k]
    return total


def kernel_form(expX, x, alpha, invQ, m_in, S_in, pairs=None):
    """(mean, egrad, cov, evar, info) in float64 with the kernels' order of summation."""
    expX, alpha = np.atleast_2d(expX), np.atleast_2d(alpha)
    E, (N, D) = expX.shape[0], x.shape
    m_in, S_in = mn.rows_arrays(m_in, S_in, D)
    pairs = mn.pairs_array(pairs, E)
    M, P = m_in.shape[0], len(pairs)
    mean, egrad, cov = np.full((M, E), np.nan), np.full((M, E, D), np.nan), np.full((M, P), np.nan)
    evar = None if invQ is None else np.full((M, E), np.nan)
    info = np.zeros(M, np.int32)
    low = np.tril_indices(D)
    for r in range(M):
        if not (np.isfinite(m_in[r]).all() and np.isfinite(S_in[r][low]).all()):
            info[r] = -1
            continue
        C, info[r] = mn.psd_cholesky(S_in[r])
        if info[r]:
            continue
        u = x - m_in[r]
        per = {}
        for e in range(E):
            ee, b = expX[e, :D], expX[e, D]
            F, ld = mn.scale_class(C, ee)
            z, hf, q = mn.point_terms(ee, b, F, ld, u)
            w = alpha[e] * q
            per[e] = (hf, q, w, ld)
            mean[r, e] = _lane_sum(w, 64)
            h = _lane_sum(w[:, None] * z, 64)
            t = np.zeros(D)
            for d in range(D):
                t = t + F[d, :] * h[d]
            rr = h.copy()
            for k in range(D):
                rr = rr - F[:, k] * t[k]
            egrad[r, e] = np.sqrt(ee) * rr
        for k, (p, q_) in enumerate(pairs):
            ep, eq = expX[p, :D], expX[q_, :D]
            Fs, lds = mn.scale_class(C, ep + eq)
            (hf_p, q_p, w_p, ld_p), (hf_q, q_q, w_q, ld_q) = per[p], per[q_]
            t = np.expm1(mn.pair_delta(ep, eq, Fs, hf_p, hf_q, ld_p + ld_q - lds, u))
            # a lane owns a column l and walks j: the lane axis is l, the walk j ascending inside each step of 256
            terms = (np.multiply.outer(w_p, w_q) * t).T                   # [l][j]
            cov[r, k] = _lane_sum(_walk(terms), 256)
            if evar is not None and p == q_:
                terms = ((invQ[p] * np.multiply.outer(q_p, q_p)) * (1.0 + t)).T
                evar[r, p] = expX[p, D] - _lane_sum(_walk(terms), 256)
    return mean, egrad, cov, evar, info


def _walk(terms):
    """terms [l][j] -> [l]: each column's own sum over j ascending (a sequential chain, as the lane forms it)."""
    acc = np.zeros(terms.shape[0])
    for j in range(terms.shape[1]):
        acc = acc + terms[:, j]
    return acc


def units(got, tr):
    """dict(V, Ev, mean, grad): the largest |got - truth| / (u S) of each family over the rows with info == 0 (NaN
    where the family is absent).  ``got`` is (mean, egrad, cov, evar, info)."""
    mean, egrad, cov, evar, _ = got
    ok = tr["info"] == 0

    def worst(g, t, S):
        if g is None or t is None or not ok.any():
            return float("nan")
        g, t, S = np.asarray(g).astype(LD).reshape(t.shape)[ok], t[ok], S[ok]
        fin = ~np.isnan(t)                                  # (an emulator without its (e, e) pair has no Ev)
        if not np.array_equal(np.isnan(np.asarray(g, dtype=np.float64)), ~fin):
            return float("inf")
        if not fin.any():
            return float("nan")
        return float((np.abs(g[fin] - t[fin]) / (LD(U) * S[fin])).max())

    return dict(V=worst(cov, tr["cov"], tr["S_cov"]), Ev=worst(evar, tr["evar"], tr["S_evar"]),
                mean=worst(mean, tr["mean"], tr["S_mean"]), grad=worst(egrad, tr["grad"], tr["S_grad"]))


_gates = {}


def gates(key, expX, x, alpha, invQ, m_in, S_in, pairs=None):
    """dict(a, b, gate): the yardsticks' errors per family and the gates, in units of u S."""
    if key not in _gates:
        tr = truth(key, expX, x, alpha, invQ, m_in, S_in, pairs)
        ya = units(mn.moments_pairs_numpy(expX, x, alpha, invQ, m_in, S_in, pairs), tr)
        yb = units(kernel_form(expX, x, alpha, invQ, m_in, S_in, pairs), tr)
        gate = {}
        for f in FAMILIES:
            y = max(ya[f], yb[f]) if not (np.isnan(ya[f]) or np.isnan(yb[f])) else float("nan")
            gate[f] = y if np.isnan(y) else min(MARGIN * max(y, 1.0), float(CAP))
        _gates[key] = dict(a=ya, b=yb, gate=gate)
    return _gates[key]


def within(got, tr, gate, factor=1.0):
    """The families of ``got`` whose error exceeds ``factor`` x the gate, with the error: empty when all is well.
    Non-finite results count as infinitely wrong; a family that the call does not have is passed over."""
    un = units(got, tr)
    return {f: un[f] for f in FAMILIES if not np.isnan(gate[f]) and not un[f] <= factor * gate[f]}


def as_truth(got, tr):
    """``got`` of the numpy branch in the place of the truth's values (its S kept): device against branch."""
    mean, egrad, cov, evar, _ = got
    out = dict(tr, mean=np.asarray(mean).astype(LD).reshape(tr["mean"].shape),
               grad=np.asarray(egrad).astype(LD).reshape(tr["grad"].shape),
               cov=np.asarray(cov).astype(LD).reshape(tr["cov"].shape))
    if tr["evar"] is not None:
        out["evar"] = np.asarray(evar).astype(LD).reshape(tr["evar"].shape)
    return out
