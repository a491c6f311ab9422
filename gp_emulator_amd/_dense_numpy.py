"""The small dense solves in float64 numpy: the explicit CPU branches of ``Context.newton_step``, ``posterior_cov``,
``prior_propagate`` and ``rts_smooth`` and of the retrievals, and the reference the CPU tests compare against.  Pure
numpy: nothing here touches the library.  Every function is vectorised over the rows and written out as explicit loops
in the kernels' summation order (csrc/gp_dense_device.hpp and the four kernel headers); never a fallback.
"""
import numpy as np

DAMPINGS = ("diagonal", "identity")


def prec_rows(P, M, D, dtype=np.float64):
    """A prior precision (or a process noise) as a contiguous ``dtype`` array: one matrix ``(D, D)`` for all rows, or
    ``(M, D, D)``, row m's own.  With one row the two say the same and the array is taken as shared, so a one-row call
    goes the way it always went."""
    P = np.asarray(P, dtype=dtype)
    return np.ascontiguousarray(P if M > 1 and P.ndim == 3 and P.shape == (M, D, D) else P.reshape(D, D))


def prior_rows(prior, M, D, dtype=np.float64):
    """``prior = (x0, P)`` as contiguous ``dtype`` arrays: ``x0`` ``(D,)`` or per row ``(M, D)``, ``P`` ``(D, D)`` or
    per row ``(M, D, D)``, independently of one another (with one row: shared, as ``prec_rows``)."""
    x0 = np.asarray(prior[0], dtype=dtype)
    x0 = np.ascontiguousarray(x0 if M > 1 and x0.ndim == 2 and x0.shape == (M, D) else x0.reshape(D))
    return x0, prec_rows(prior[1], M, D, dtype)


def row_strides(x0, P):
    """The element strides of the ``_rows`` entries for what ``prior_rows`` / ``prec_rows`` returned: 0 = shared."""
    return (x0.shape[1] if x0 is not None and x0.ndim == 2 else 0), (P.shape[1] * P.shape[2] if P is not None and P.ndim == 3 else 0)


def _system_matrices(A, prior_prec):
    """``(A' = A (+ P), a fresh float64 (M, D, D); M; D)`` for ``A`` (M, D, D) and ``prior_prec`` None, (D, D) or (M, D, D)."""
    L = np.array(A, dtype=np.float64)
    if L.ndim != 3 or L.shape[1] != L.shape[2]:
        raise ValueError("A must be (n_rows, n_inputs, n_inputs)")
    M, D = L.shape[:2]
    if prior_prec is not None:
        L = L + prec_rows(prior_prec, M, D)
    return L, M, D


def _clip(x, bounds):
    """``x`` (M, D) clamped to ``bounds = (lo (D,), hi (D,))``: max with lo, then min with hi, as the kernels' clamp; a
    NaN stays NaN, there as here."""
    return np.minimum(np.maximum(x, np.asarray(bounds[0], dtype=np.float64)), np.asarray(bounds[1], dtype=np.float64))


def _cholesky_factor_numpy(L):
    """``L L^T`` of the lower triangles of ``L`` (M, D, D) in place, every sum in ascending index; ``status`` (M,) int32: 0,
    or k + 1 for the first pivot that is not > 0 or not finite.  The caller holds ``np.errstate(all="ignore")``."""
    M, D = L.shape[:2]
    status = np.zeros(M, np.int32)
    for k in range(D):
        s = L[:, k:, k].copy()                                   # rows j >= k of column k
        for q in range(k):
            s -= L[:, k:, q] * L[:, k, q][:, None]
        piv = s[:, 0]
        bad = ~(piv > 0.0) | ~np.isfinite(piv)
        status[(status == 0) & bad] = k + 1
        dk = np.sqrt(piv)
        L[:, k, k] = dk
        L[:, k + 1:, k] = s[:, 1:] / dk[:, None]
    return status


def newton_step_numpy(x, grad, A, lam, damping="diagonal", prior=None, bounds=None):
    """The damped Newton step of ``gp_newton_step_device`` in float64 numpy, vectorised over the rows and written out
    in the kernel's summation order (ascending index in the factorisation, in both substitutions and in the prior's
    chain): ``(step (M, D), trial (M, D), status (M,) int32)``.  The explicit CPU branch of ``Context.newton_step``
    and of ``perband.retrieve_bands``, and the reference of the CPU tests; never a fallback.

        A' = A (+ P),  g' = grad (+ P (x - x0)),  A'_dd += lam * (A'_dd | 1),  L L^T = A' (lower triangle read),
        step = -L^-T L^-1 g',  trial = clip(x + step, lo, hi);  status = k + 1 when pivot k is not > 0 or not finite,
        then step = 0 and trial = x.

    ``prior=(x0 (D,) or (M, D), P (D, D) or (M, D, D))`` (shared or row m's own, as ``gp_newton_step_rows_device``),
    ``bounds=(lo (D,), hi (D,))``, ``lam`` (M,) or a scalar."""
    if damping not in DAMPINGS:
        raise ValueError("damping must be 'diagonal' or 'identity'")
    x = np.array(x, dtype=np.float64, ndmin=2)
    M, D = x.shape
    g = np.array(grad, dtype=np.float64).reshape(M, D)
    L = np.array(A, dtype=np.float64).reshape(M, D, D)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (M,))
    if prior is not None:
        x0, P = prior_rows(prior, M, D)
        L = L + P
        for c in range(D):
            g += P[..., :, c] * (x[:, c] - x0[..., c])[:, None]
    idx = np.arange(D)
    diag = L[:, idx, idx]
    L[:, idx, idx] = diag + lam[:, None] * (diag if damping == "diagonal" else 1.0)
    with np.errstate(all="ignore"):
        status = _cholesky_factor_numpy(L)
        y = g                                                       # y = L^-1 g'
        for k in range(D):
            y[:, k] = y[:, k] / L[:, k, k]
            y[:, k + 1:] -= L[:, k + 1:, k] * y[:, k][:, None]
        z = np.zeros((M, D))                                        # z = L^-T y
        for i in range(D - 1, -1, -1):
            a = y[:, i].copy()
            for k in range(i + 1, D):
                a -= L[:, k, i] * z[:, k]
            z[:, i] = a / L[:, i, i]
    ok = (status == 0)[:, None]
    step = np.where(ok, -z, 0.0)
    trial = x + step
    if bounds is not None:
        trial = _clip(trial, bounds)
    trial = np.where(ok, trial, x)
    return step, trial, status


def _cholesky_inverse_numpy(L):
    """``(W, status)`` for the matrices ``L`` (M, D, D), factored in place: ``W[:, i, j]``, i >= j, is element (i, j) of
    the inverse by the kernels' chains (ascending index in the factorisation and in both substitutions of every unit
    vector), NaN throughout where ``status`` (k + 1 for the first pivot that is not > 0 or not finite) is not 0.  Only
    the lower triangle of ``L`` is read."""
    M, D = L.shape[:2]
    W = np.zeros((M, D, D))                                         # W[:, i, j]: y_i, then z_i, of column j
    with np.errstate(all="ignore"):
        status = _cholesky_factor_numpy(L)
        for i in range(D):                                           # y = L^-1 e_j, the columns j <= i side by side
            s = np.zeros((M, i + 1))
            s[:, i] = 1.0
            for k in range(i):                                       # (column j takes the terms k >= j)
                s[:, :k + 1] -= L[:, i, k][:, None] * W[:, k, :k + 1]
            W[:, i, :i + 1] = s / L[:, i, i][:, None]
        for i in range(D - 1, -1, -1):                               # z = L^-T y, down to row j
            a = W[:, i, :i + 1].copy()
            for k in range(i + 1, D):
                a -= L[:, k, i][:, None] * W[:, k, :i + 1]
            W[:, i, :i + 1] = a / L[:, i, i][:, None]
        W[status != 0] = np.nan
    return W, status


def _mirror_lower(W):
    """The symmetric matrices whose lower triangles are those of ``W`` (M, D, D)."""
    return np.tril(W) + np.transpose(np.tril(W, -1), (0, 2, 1))


def posterior_cov_numpy(A, prior_prec=None):
    """The posterior covariance of ``gp_posterior_cov_device`` in float64 numpy, vectorised over the rows and written
    out in the kernel's summation order (ascending index in the factorisation and in both substitutions):
    ``(cov (M, D, D), sigma (M, D), status (M,) int32)``.  The explicit CPU branch of ``Context.posterior_cov`` and of
    ``perband.retrieve_bands(return_cov=True)``, and the reference of the CPU tests; never a fallback.

        A' = A (+ P), no damping,  L L^T = A' (lower triangle read),  C[:, j] = L^-T L^-1 e_j,
        cov = C with the elements i >= j from column j's solve and the upper triangle mirrored from them,
        sigma = sqrt(diag C);  status = k + 1 when pivot k is not > 0 or not finite, then cov and sigma are NaN.

    ``prior_prec`` is ``(D, D)``, shared, or ``(M, D, D)``, row m's own (``gp_posterior_cov_rows_device``)."""
    L, M, D = _system_matrices(A, prior_prec)
    W, status = _cholesky_inverse_numpy(L)
    with np.errstate(all="ignore"):
        cov = _mirror_lower(W)
        idx = np.arange(D)
        sigma = np.sqrt(W[:, idx, idx])
    return cov, sigma, status


def prior_propagate_numpy(A, prior_prec, noise):
    """The prior propagation of ``gp_prior_propagate_device`` in float64 numpy, in the kernel's summation order:
    ``(next_prec (M, D, D), status (M,) int32)``.  The explicit CPU branch of ``Context.prior_propagate`` and of the
    retrievals' ``next_prior=``, and the reference of the CPU tests; never a fallback.

        A' = A (+ P),  C = A'^-1 as ``posterior_cov_numpy``,  S = C + Q (lower triangles),  N = S^-1 the same way,
        next_prec = N with the upper triangle mirrored;  status = k + 1 when pivot k of A' fails, D + k + 1 when pivot
        k of S fails, then next_prec is NaN.

    ``prior_prec`` is None, ``(D, D)`` or ``(M, D, D)``; ``noise`` (the process-noise covariance Q) ``(D, D)`` or
    ``(M, D, D)``."""
    L, M, D = _system_matrices(A, prior_prec)
    C, first = _cholesky_inverse_numpy(L)
    with np.errstate(all="ignore"):
        S = C + prec_rows(noise, M, D)                               # (NaN where the first inversion failed)
    W, second = _cholesky_inverse_numpy(S)
    status = np.where(first != 0, first, np.where(second != 0, D + second, 0)).astype(np.int32)
    return _mirror_lower(W), status


def rts_smooth_numpy(A, prior_prec, noise, x, x_next, cov_next, bounds=None):
    """One backward step of the Rauch-Tung-Striebel smoother of ``gp_rts_smooth_device`` in float64 numpy, in the
    kernel's summation order: ``(x_smooth (M, D), cov_smooth (M, D, D), sigma_smooth (M, D), status (M,) int32)``.  The
    explicit CPU branch of ``Context.rts_smooth`` and of the series' ``smooth=True``, and the reference of the CPU
    tests; never a fallback.

        A' = A (+ P),  C = A'^-1,  S = C + Q,  N = S^-1 as ``prior_propagate_numpy``,  G = C N,
        x_smooth = clip(x + G (x_next - x), lo, hi),  Delta = cov_next - S,  cov_smooth = C + (G Delta) G^T (the lower
        triangle computed, the upper mirrored),  sigma_smooth = sqrt(diag cov_smooth);  every product a sum from 0 in
        ascending index;  status = k + 1 when pivot k of A' fails, D + k + 1 when pivot k of S fails, then the row's
        outputs are NaN.

    ``prior_prec`` is None, ``(D, D)`` or ``(M, D, D)``; ``noise`` ``(D, D)`` or ``(M, D, D)``; ``x`` the filtered
    states of the date, ``x_next`` and ``cov_next`` the smoothed state and covariance of the next date;
    ``bounds=(lo (D,), hi (D,))``.  Only the lower triangles of the matrices are read."""
    L, M, D = _system_matrices(A, prior_prec)
    x = np.asarray(x, dtype=np.float64).reshape(M, D)
    d = np.asarray(x_next, dtype=np.float64).reshape(M, D) - x
    Cw, first = _cholesky_inverse_numpy(L)
    with np.errstate(all="ignore"):
        S = Cw + prec_rows(noise, M, D)                              # (NaN where the first inversion failed)
        Delta = _mirror_lower(np.asarray(cov_next, dtype=np.float64).reshape(M, D, D) - S)
    Nw, second = _cholesky_inverse_numpy(S)                          # (factors S in place: Delta is taken first)
    status = np.where(first != 0, first, np.where(second != 0, D + second, 0)).astype(np.int32)
    with np.errstate(all="ignore"):
        C, N = _mirror_lower(Cw), _mirror_lower(Nw)
        G, F, K = np.zeros((M, D, D)), np.zeros((M, D, D)), np.zeros((M, D, D))
        gd = np.zeros((M, D))
        for k in range(D):
            G += C[:, :, k, None] * N[:, None, k, :]
        for c in range(D):
            gd += G[:, :, c] * d[:, c, None]
        for l in range(D):
            F += G[:, :, l, None] * Delta[:, None, l, :]
        for k in range(D):
            K += F[:, :, k, None] * G[:, None, :, k]                 # K_ij += F_ik G_jk
        xs = x + gd
        if bounds is not None:
            xs = _clip(xs, bounds)
        cov = _mirror_lower(C + K)
        idx = np.arange(D)
        sigma = np.sqrt(cov[:, idx, idx])
    bad = status != 0
    xs[bad], cov[bad], sigma[bad] = np.nan, np.nan, np.nan
    return xs, cov, sigma, status
