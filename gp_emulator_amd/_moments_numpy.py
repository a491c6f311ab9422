"""Moments of squared-exponential ARD emulators under a Gaussian input ``x ~ N(m, Sigma)``, in closed form (moment
matching in the sense of Girard and of Quinonero-Candela): the float64 numpy branch of ``gp_moments_batch_f64`` and the
small host steps both branches share.

With ``e = exp(theta)``, ``alpha = invQt``, ``Sigma = C C'`` (``psd_cholesky``: a direction without uncertainty is a
zero column of C) and, for a vector of precisions e (a *scale class*: ``e_p``, ``e_q`` or ``e_s = e_p + e_q``),

    B' = I + C' E C = L L',   F = E^(1/2) C L^-T,   ld = 1/2 log det B' = 1/2 sum_k log1p(d_k)

where the pivot minus one ``d_k = (C'EC)_kk - sum_{i<k} L_ki^2`` is formed as such (``scale_class``), so that
``(I + E^(1/2) Sigma E^(1/2))^-1 = I - F F'``.  Per training point ``z_j = E_p^(1/2)(x_j - m)``, ``f_j = F_p' z_j``,

    q_j    = b_p exp(-ld_p - |z_j|^2 / 2 + |f_j|^2 / 2)                  E[k_p(x, x_j)]
    M_p    = sum_j alpha_pj q_j                                           E[mu_p]
    dM_p   = E_p^(1/2) (h - F_p F_p' h),  h = sum_j alpha_pj q_j z_j      E[d mu_p / dx]   (Cov[x, mu_p] = Sigma dM_p)

and per pair ``(p, q)`` with ``g^p_j = F_s' E_p E_s^(-1/2)(x_j - m)`` and ``g^q_l`` likewise,

    delta_jl = |g^p_j + g^q_l|^2 / 2 - |f^p_j|^2 / 2 - |f^q_l|^2 / 2 + (ld_p + ld_q - ld_s)
    V_pq     = sum_jl alpha_pj alpha_ql q^p_j q^q_l expm1(delta_jl)                          Cov[mu_p, mu_q]
    Ev_p     = b_p - sum_jl invQ_p[j, l] q_j q_l (1 + expm1(delta_jl))                       E[v_p(x)]   (p = q)

Everything of order one has cancelled algebraically in delta, which is of the order of Sigma: V keeps its digits as
Sigma -> 0, where ``alpha' Q alpha - M^2`` has none left, and is exactly 0 at Sigma = 0.  The sums still cancel
(``sum |terms| / |V|`` of 1e2 to 2e3 for trained emulators), which is why there is no float32 form.
"""
import collections

import numpy as np

from ._sobol_numpy import mirror, upper_pairs  # noqa: F401  (their names here)

UncertainPrediction = collections.namedtuple("UncertainPrediction", "mean var_state var_emulator expected_grad info")
UncertainSpectrum = collections.namedtuple("UncertainSpectrum", "mean var_state var_emulator info")
UncertainSpectrumPC = collections.namedtuple("UncertainSpectrumPC", "mean var_state var_emulator info pc_mean pc_cov")

U = 2.0 ** -53
PIVOT_TOL = 64 * U      # |pivot| <= PIVOT_TOL * Sigma_kk: the direction carries no uncertainty


def rows_arrays(mean_in, cov_in, D):
    """``mean_in`` as C-contiguous float64 (M, D) and ``cov_in`` -- (D, D), or (M, D, D) -- as (M, D, D)."""
    m = np.ascontiguousarray(np.atleast_2d(np.asarray(mean_in, dtype=np.float64)))
    if m.ndim != 2 or m.shape[1] != D or m.shape[0] == 0:
        raise ValueError("the means must be (n_rows, %d), got %s" % (D, np.shape(mean_in)))
    c = np.asarray(cov_in, dtype=np.float64)
    if c.shape == (D, D):
        c = np.broadcast_to(c, (m.shape[0], D, D))
    if c.shape != (m.shape[0], D, D):
        raise ValueError("the covariances must be (%d, %d) or (%d, %d, %d), got %s"
                         % (D, D, m.shape[0], D, D, np.shape(cov_in)))
    return m, np.ascontiguousarray(c)


def pairs_array(pairs, E):
    """The (P, 2) pair list (None: (e, e) of every emulator) as int64, checked against E."""
    if pairs is None:
        return np.stack([np.arange(E)] * 2, axis=1)
    p = np.asarray(pairs, dtype=np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] == 0:
        raise ValueError("pairs must be (n_pairs, 2)")
    if p.min() < 0 or p.max() >= E:
        raise ValueError("a pair names an emulator outside 0..%d" % (E - 1))
    return p


def psd_cholesky(S):
    """``(C, info)``: the lower factor of a positive semi-definite S from its lower triangle.  A pivot d_k with
    ``|d_k| <= 64 u S_kk`` gives a zero column (that input is fixed); one below ``-64 u S_kk`` ends the
    factorisation with ``info = k + 1`` (posterior_cov's convention), else ``info = 0``."""
    D = S.shape[0]
    C = np.zeros((D, D), S.dtype)
    for k in range(D):
        d = S[k, k] - np.dot(C[k, :k], C[k, :k])
        tol = PIVOT_TOL * S[k, k]
        if abs(d) <= tol:
            continue
        if not d > 0:
            return C, k + 1
        C[k, k] = np.sqrt(d)
        C[k + 1:, k] = (S[k + 1:, k] - C[k + 1:, :k] @ C[k, :k]) / C[k, k]
    return C, 0


def scale_class(C, e):
    """``(F, ld)`` of the precisions e: the factor L of I + C'EC with the pivots minus one formed directly (so that
    log1p sees them whole), F = E^(1/2) C L^-T by forward substitution, ld = 1/2 sum log1p."""
    D = C.shape[0]
    A = C.T @ (e[:, None] * C)
    L = np.zeros((D, D), C.dtype)
    R = (np.sqrt(e)[:, None] * C).T          # L Y = R, Y = F'
    Y = np.zeros((D, D), C.dtype)
    ld = C.dtype.type(0)
    for k in range(D):
        d = A[k, k] - np.dot(L[k, :k], L[k, :k])
        ld = ld + np.log1p(d)
        L[k, k] = np.sqrt(1 + d)
        L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
        Y[k] = (R[k] - L[k, :k] @ Y[:k]) / L[k, k]
    return Y.T, ld / 2


def point_terms(e, b, F, ld, u):
    """``(z (N, D), hf (N,), q (N,))`` of an emulator on the centred training inputs u = x - m: hf = |F'z|^2 / 2."""
    z = np.sqrt(e) * u
    f = z @ F
    hf = 0.5 * (f * f).sum(axis=1)
    return z, hf, b * np.exp(-ld - 0.5 * (z * z).sum(axis=1) + hf)


def pair_delta(ep, eq, Fs, hf_p, hf_q, ld_pqs, u):
    """delta (N, N) of a pair from its class's F, the emulators' |f|^2 / 2 and ld_p + ld_q - ld_s."""
    rs = 1.0 / np.sqrt(ep + eq)
    gp, gq = (ep * rs * u) @ Fs, (eq * rs * u) @ Fs
    t = gp[:, None, :] + gq[None, :, :]
    return 0.5 * (t * t).sum(axis=2) - hf_p[:, None] - hf_q[None, :] + ld_pqs


def moments_pairs_numpy(expX, inputs, invQt, invQ, mean_in, cov_in, pairs=None):
    """The float64 numpy branch of ``Context.moments_batch``, same arguments and results: ``(mean (M, E), egrad
    (M, E, D), cov (M, P), evar (M, E) or None, info (M,) int32)``.  ``evar`` needs ``invQ`` (E, N, N) and is NaN for an
    emulator whose pair (e, e) is not in ``pairs``."""
    expX = np.atleast_2d(np.asarray(expX, dtype=np.float64))
    x = np.asarray(inputs, dtype=np.float64)
    alpha = np.atleast_2d(np.asarray(invQt, dtype=np.float64))
    (N, D), E = x.shape, expX.shape[0]
    if expX.shape != (E, D + 2) or alpha.shape != (E, N):
        raise ValueError("expX must be (n_emulators, n_inputs + 2) and invQt (n_emulators, n_train)")
    if invQ is not None:
        invQ = np.asarray(invQ, dtype=np.float64).reshape(-1, N, N)
        if invQ.shape[0] != E:
            raise ValueError("invQ must be (n_emulators, n_train, n_train)")
    m_in, S_in = rows_arrays(mean_in, cov_in, D)
    pairs = pairs_array(pairs, E)
    M, P = m_in.shape[0], pairs.shape[0]
    bad = ~(np.isfinite(expX[:, :D + 1]).all(axis=1) & np.isfinite(alpha).all(axis=1))
    if invQ is not None:
        bad |= ~np.isfinite(invQ).all(axis=(1, 2))
    mean, egrad, cov = np.full((M, E), np.nan), np.full((M, E, D), np.nan), np.full((M, P), np.nan)
    evar = None if invQ is None else np.full((M, E), np.nan)
    info = np.zeros(M, np.int32)
    low = np.tril_indices(D)
    with np.errstate(all="ignore"):
        for r in range(M):
            if not (np.isfinite(m_in[r]).all() and np.isfinite(S_in[r][low]).all()):
                info[r] = -1
                continue
            C, info[r] = psd_cholesky(S_in[r])
            if info[r]:
                continue
            u = x - m_in[r]
            per = {}
            for e in range(E):
                if bad[e]:
                    continue
                ee, b = expX[e, :D], expX[e, D]
                F, ld = scale_class(C, ee)
                z, hf, q = point_terms(ee, b, F, ld, u)
                w = alpha[e] * q
                per[e] = (hf, q, w, ld)
                h = (w[:, None] * z).sum(axis=0)
                mean[r, e] = w.sum()
                egrad[r, e] = np.sqrt(ee) * (h - F @ (F.T @ h))
            for k, (p, q_) in enumerate(pairs):
                if bad[p] or bad[q_]:
                    continue
                ep, eq = expX[p, :D], expX[q_, :D]
                Fs, lds = scale_class(C, ep + eq)
                (hf_p, q_p, w_p, ld_p), (hf_q, q_q, w_q, ld_q) = per[p], per[q_]
                t = np.expm1(pair_delta(ep, eq, Fs, hf_p, hf_q, ld_p + ld_q - lds, u))
                cov[r, k] = (np.multiply.outer(w_p, w_q) * t).sum()
                if evar is not None and p == q_:
                    evar[r, p] = expX[p, D] - (invQ[p] * np.multiply.outer(q_p, q_p) * (1.0 + t)).sum()
    return mean, egrad, cov, evar, info


# ---- the spectral step of a MultivariateEmulator: quadratic forms on the host, as _sobol_numpy.spectral ----------------
def spectral_variances(basis, pc_cov, pc_evar):
    """``(var_state (M, K), var_emulator (M, K))`` of the bands ``f_k = sum_p basis[p, k] mu_p`` from the PCs' mirrored
    covariances (M, P, P) and expected variances (M, P): ``beta_k' V beta_k`` and ``sum_p beta_pk^2 Ev_p``,
    ``beta_k = basis[:, k]``; nothing of size K is ever emulated."""
    basis = np.asarray(basis, dtype=np.float64)
    var_state = np.einsum("pk,mpq,qk->mk", basis, np.asarray(pc_cov, dtype=np.float64), basis)
    return var_state, np.asarray(pc_evar, dtype=np.float64) @ (basis * basis)
