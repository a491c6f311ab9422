"""The small dense solves in float64 numpy: the explicit CPU branches of ``Context.newton_step``, ``posterior_cov``,
``prior_propagate``, ``rts_smooth``, ``series_step`` and ``series_cov`` and of the retrievals, and the reference the CPU
tests compare against.  Pure numpy: nothing here touches the library.  Every function is vectorised over the rows and
written out as explicit loops in the kernels' summation order (csrc/gp_dense_device.hpp and the five kernel headers); never
a fallback.
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


def box_pass_cap(D):
    """The most passes a row of the box step runs; a row cut off there reports one more."""
    return 3 * D + 4


def box_step_numpy(x, grad, A, lam, damping="diagonal", prior=None, bounds=None):
    """The bound-constrained damped Newton step of ``gp_box_step_device`` in float64 numpy, vectorised over the rows and
    written out in the kernel's order (csrc/gp_box_step_kernel.hpp): ``(step (M, D), trial (M, D), status (M,) int32,
    at_lo (M,) uint32, at_hi (M,) uint32, passes (M,) int32)``.  The explicit CPU branch of ``Context.box_step`` and of
    the retrievals' ``bounds_mode="active_set"``, and the reference of the CPU tests; never a fallback.

        H = the damped A' and g' of ``newton_step_numpy``;  l = lo - x, u = hi - x;
        step = argmin 1/2 d^T H d + g'^T d over l <= d <= u by the primal active-set method: start at clip(0, l, u); a
        pass factors H with the bound components' rows and columns replaced by the identity, solves s_F = -H_FF^-1 r_F,
        goes to the first bound it meets (lowest index of the smallest ratio) and fixes that component, or takes the
        whole step and frees the bound component with the largest wrong-signed multiplier (lowest index), or is done;
        trial = clip(x + step, lo, hi);  status = k + 1 when pivot k of any pass fails, then step = 0 and trial = x.

    At most ``box_pass_cap(D)`` passes: a row that is cut off there returns its iterate with one more in ``passes``.  A
    row with a non-finite ``x``, ``g'`` or bound is NaN in every element of step and trial, with status, masks and passes
    0.  ``bounds`` is required; the other arguments are ``newton_step_numpy``'s."""
    if damping not in DAMPINGS:
        raise ValueError("damping must be 'diagonal' or 'identity'")
    if bounds is None:
        raise ValueError("the box step needs bounds")
    x = np.array(x, dtype=np.float64, ndmin=2)
    M, D = x.shape
    g = np.array(grad, dtype=np.float64).reshape(M, D)
    H = np.array(A, dtype=np.float64).reshape(M, D, D)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (M,))
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(D) for b in bounds)
    rows, idx = np.arange(M), np.arange(D)
    with np.errstate(all="ignore"):
        if prior is not None:
            x0, P = prior_rows(prior, M, D)
            H = H + P
            for c in range(D):
                g += P[..., :, c] * (x[:, c] - x0[..., c])[:, None]
        diag = H[:, idx, idx]
        H[:, idx, idx] = diag + lam[:, None] * (diag if damping == "diagonal" else 1.0)
        H = _mirror_lower(H)                                         # (the lower triangle is the matrix)
        l, u = lo - x, hi - x
        poisoned = ~(np.isfinite(x).all(axis=1) & np.isfinite(g).all(axis=1) & np.isfinite(lo).all() & np.isfinite(hi).all())

        def residual(d):
            r = g.copy()
            for c in range(D):
                r += H[:, :, c] * d[:, c, None]
            return r
        d = np.minimum(np.maximum(0.0, l), u)
        r = residual(d)
        cls = np.where((d <= l) & (r > 0.0), -1, np.where((d >= u) & (r < 0.0), 1, 0))
        done = poisoned.copy()
        status, passes = np.zeros(M, np.int32), np.zeros(M, np.int32)
        cap = box_pass_cap(D)
        eye = np.eye(D)
        for _ in range(cap):
            if done.all():
                break
            passes[~done] += 1
            free = cls == 0
            L = np.where(free[:, :, None] & free[:, None, :], H, eye)
            st = _cholesky_factor_numpy(L)
            failed = ~done & (st != 0)
            status[failed] = st[failed]
            done = done | failed
            y = np.where(free, -r, 0.0)                              # y = L^-1 (-r_F)
            for k in range(D):
                y[:, k] = y[:, k] / L[:, k, k]
                y[:, k + 1:] -= L[:, k + 1:, k] * y[:, k][:, None]
            s = np.zeros((M, D))                                     # s = L^-T y
            for i in range(D - 1, -1, -1):
                a = y[:, i].copy()
                for k in range(i + 1, D):
                    a -= L[:, k, i] * s[:, k]
                s[:, i] = a / L[:, i, i]
            s = np.where(free, s, 0.0)
            ratio = np.where(free & (s > 0.0), (u - d) / s, np.where(free & (s < 0.0), (l - d) / s, np.inf))
            ratio[np.isnan(ratio)] = np.inf
            k = np.argmin(ratio, axis=1)                             # (the lowest index of the minimum)
            amin = ratio[rows, k]
            blocked = amin < 1.0
            dn = np.where(blocked[:, None], np.minimum(np.maximum(d + amin[:, None] * s, l), u), d + s)
            cn = cls.copy()
            up_ = s[rows, k] > 0.0
            dn[blocked, k[blocked]] = np.where(up_, u[rows, k], l[rows, k])[blocked]
            cn[blocked, k[blocked]] = np.where(up_, 1, -1)[blocked]
            go = ~done
            d[go], cls[go] = dn[go], cn[go]
            r[go] = residual(d)[go]
            mult = np.where(cls == -1, -r, np.where(cls == 1, r, -np.inf))
            mult[np.isnan(mult)] = -np.inf
            q = np.argmax(mult, axis=1)                              # (the lowest index of the maximum)
            release = go & ~blocked & (mult[rows, q] > 0.0)
            cls[release, q[release]] = 0
            done = done | (go & ~blocked & ~release)
        passes[~done] = cap + 1
        ok = (status == 0)[:, None]
        step = np.where(ok, d, 0.0)
        trial = np.where(ok, _clip(x + step, (lo, hi)), x)
        step[poisoned], trial[poisoned], passes[poisoned] = np.nan, np.nan, 0
        clear = poisoned | (status != 0)
        bits = np.uint64(1) << idx.astype(np.uint64)
        at_lo = np.where(clear, 0, ((cls == -1) * bits).sum(axis=1)).astype(np.uint32)
        at_hi = np.where(clear, 0, ((cls == 1) * bits).sum(axis=1)).astype(np.uint32)
    return step, trial, status, at_lo, at_hi, passes


def active_set_numpy(X, grad, A, prior, bounds):
    """What the retrievals' ``return_active=True`` appends, from the returned ``X`` (M, D) and the loop's final ``grad``
    (M, D), ``A`` (M, D, D) and prior (``prior_rows``' pair or None), in float64: ``active`` (M, D) int8, -1 where ``X <=
    lo`` and ``g' > 0``, +1 where ``X >= hi`` and ``g' < 0``, 0 otherwise, with ``g' = grad (+ P (X - x0))``; and ``kkt``
    (M,), the largest ``|g'_d| / sqrt(A'_dd)`` over the components with ``active == 0``, ``A' = A (+ P)`` -- the scaled
    projected gradient: near 0 at a constrained minimum, whatever ``state`` says."""
    X = np.asarray(X, dtype=np.float64)
    M, D = X.shape
    g = np.array(grad, dtype=np.float64).reshape(M, D)
    Ad = np.array(A, dtype=np.float64).reshape(M, D, D)[:, np.arange(D), np.arange(D)]
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(D) for b in bounds)
    with np.errstate(all="ignore"):
        if prior is not None:
            x0, P = prior_rows(prior, M, D)
            Ad = Ad + P[..., np.arange(D), np.arange(D)]
            for c in range(D):
                g += P[..., :, c] * (X[:, c] - x0[..., c])[:, None]
        active = np.where((X <= lo) & (g > 0.0), -1, np.where((X >= hi) & (g < 0.0), 1, 0)).astype(np.int8)
        kkt = np.max(np.where(active == 0, np.abs(g) / np.sqrt(Ad), 0.0), axis=1)
    return active, kkt


def _cholesky_inverse_numpy(L):
    """``(W, status)`` for the matrices ``L`` (M, D, D), factored in place: ``W[:, i, j]``, i >= j, is element (i, j) of
    the inverse by the kernels' chains (ascending index in the factorisation and in both substitutions of every unit
    vector), NaN throughout where ``status`` (k + 1 for the first pivot that is not > 0 or not finite) is not 0.  Only
    the lower triangle of ``L`` is read."""
    with np.errstate(all="ignore"):
        status = _cholesky_factor_numpy(L)
    return _factor_inverse_numpy(L, status), status


def _factor_inverse_numpy(L, status):
    """``W`` of ``_cholesky_inverse_numpy`` from the factors ``L`` (M, D, D) that ``_cholesky_factor_numpy`` left and
    its ``status``."""
    M, D = L.shape[:2]
    W = np.zeros((M, D, D))                                         # W[:, i, j]: y_i, then z_i, of column j
    with np.errstate(all="ignore"):
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
    return W


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


def _series_factor_numpy(A, W, prior_prec, lam, damping):
    """The forward sweep of the series kernels: ``(L, B, status)``, ``L[t]`` (M, D, D) the factor of
    ``S_t = H'_tt - B_t B_t^T`` (lower triangle), ``B[t]`` (M, D, D) with ``B_t L_{t-1}^T = -W`` (``B[0]`` is None),
    ``status`` (M,) int32: 0, or t D + k + 1 for the first failed pivot.  ``W`` is (M, D, D); ``lam`` None = no damping.
    The caller holds ``np.errstate(all="ignore")``."""
    T, M, D = A.shape[:3]
    idx = np.arange(D)
    Ls, Bs = [], [None]
    status = np.zeros(M, np.int32)
    for t in range(T):
        H = np.array(A[t], dtype=np.float64)
        if t == 0 and prior_prec is not None:
            H = H + prior_prec
        if t > 0:
            H = H + W
        if t < T - 1:
            H = H + W
        if lam is not None:
            diag = H[:, idx, idx]
            H[:, idx, idx] = diag + lam[:, None] * (diag if damping == "diagonal" else 1.0)
        if t > 0:
            B = Bs[t]
            for k in range(D):
                H -= B[:, :, k, None] * B[:, None, :, k]
        st = _cholesky_factor_numpy(H)
        status = np.where((status == 0) & (st != 0), t * D + st, status).astype(np.int32)
        Ls.append(H)
        if t < T - 1:
            Bn = np.zeros((M, D, D))
            for k in range(D):                                       # row i of B by substitution, the rows side by side
                s = -W[:, :, k]
                for q in range(k):
                    s = s - Bn[:, :, q] * H[:, k, q][:, None]
                Bn[:, :, k] = s / H[:, k, k][:, None]
            Bs.append(Bn)
    return Ls, Bs, status


def _series_arrays(A, W, prior_prec):
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 4 or A.shape[2] != A.shape[3]:
        raise ValueError("A must be (n_dates, n_rows, n_inputs, n_inputs)")
    T, M, D = A.shape[:3]
    Wm = np.broadcast_to(prec_rows(W, M, D), (M, D, D))
    P = prec_rows(prior_prec, M, D) if prior_prec is not None else None
    return A, Wm, P, T, M, D


def series_step_numpy(x, grad, A, lam, W, damping="diagonal", prior=None, bounds=None):
    """The block-tridiagonal damped Newton step of ``gp_series_step_device`` in float64 numpy, vectorised over the pixels
    and written out in the kernel's order (csrc/gp_series_kernel.hpp): ``(step (T, M, D), trial (T, M, D), status (M,)
    int32)`` for date-major ``x``, ``grad`` (T, M, D) and ``A`` (T, M, D, D).  The explicit CPU branch of
    ``Context.series_step`` and of the joint retrievals, and the reference of the CPU tests; never a fallback.

        H_tt = A_t (+ P, t = 0) (+ W, t > 0) (+ W, t < T-1),  H_t,t-1 = -W,
        g'_t = grad_t (+ P (x_0 - x0)) + W (x_t - x_{t-1}) - W (x_{t+1} - x_t),  H'_dd = H_dd + lam * (H_dd | 1),
        S_0 = H'_00, S_t = H'_tt - B_t B_t^T, L_t L_t^T = S_t, B_{t+1} L_t^T = -W, forward and backward substitutions,
        trial = clip(x + step, lo, hi);  status = t D + k + 1 for the first failed pivot, then step = 0 and trial = x.

    ``W`` is the precision of the process noise, (D, D) or (M, D, D); ``prior=(x0, P)`` is date 0's, shared or per
    pixel; ``lam`` (M,) or a scalar.  With T = 1 this is ``newton_step_numpy`` bit for bit."""
    if damping not in DAMPINGS:
        raise ValueError("damping must be 'diagonal' or 'identity'")
    x = np.array(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("x must be (n_dates, n_rows, n_inputs)")
    A, Wm, _, T, M, D = _series_arrays(A, W, None)
    g = np.array(grad, dtype=np.float64).reshape(T, M, D)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (M,))
    P = None
    with np.errstate(all="ignore"):
        if prior is not None:
            x0, P = prior_rows(prior, M, D)
            for c in range(D):
                g[0] += P[..., :, c] * (x[0][:, c] - x0[..., c])[:, None]
        for t in range(T):
            if t > 0:
                d = x[t] - x[t - 1]
                for c in range(D):
                    g[t] += Wm[:, :, c] * d[:, c, None]
            if t < T - 1:
                d = x[t + 1] - x[t]
                for c in range(D):
                    g[t] -= Wm[:, :, c] * d[:, c, None]
        Ls, Bs, status = _series_factor_numpy(A, Wm, P, lam, damping)
        ys = []
        for t in range(T):                                           # y_t = L_t^-1 (g'_t - B_t y_{t-1})
            L, y = Ls[t], g[t]
            if t > 0:
                for k in range(D):
                    y -= Bs[t][:, :, k] * ys[t - 1][:, k, None]
            for k in range(D):
                y[:, k] = y[:, k] / L[:, k, k]
                y[:, k + 1:] -= L[:, k + 1:, k] * y[:, k][:, None]
            ys.append(y)
        zs = [None] * T
        for t in range(T - 1, -1, -1):                               # z_t = L_t^-T (y_t - B_{t+1}^T z_{t+1})
            L, a_t = Ls[t], ys[t].copy()
            if t < T - 1:
                for k in range(D):
                    a_t -= Bs[t + 1][:, k, :] * zs[t + 1][:, k, None]
            z = np.zeros((M, D))
            for i in range(D - 1, -1, -1):
                a = a_t[:, i].copy()
                for k in range(i + 1, D):
                    a -= L[:, k, i] * z[:, k]
                z[:, i] = a / L[:, i, i]
            zs[t] = z
        ok = (status == 0)[None, :, None]
        step = np.where(ok, -np.stack(zs), 0.0)
        trial = x + step
        if bounds is not None:
            trial = _clip(trial, bounds)
        trial = np.where(ok, trial, x)
    return step, trial, status


def series_cov_numpy(A, W, prior_prec=None):
    """The marginal posterior covariances of ``gp_series_cov_device`` in float64 numpy, in the kernel's order:
    ``(cov (T, M, D, D), sigma (T, M, D), status (M,) int32)``.  The explicit CPU branch of ``Context.series_cov`` and
    of the joint retrievals, and the reference of the CPU tests; never a fallback.

        the forward factorisation of ``series_step_numpy`` without damping,  Sigma_{T-1} = (L L^T)^-1 as
        ``posterior_cov_numpy``,  K_t = -L_t^-T B_{t+1}^T,  Sigma_t = (L_t L_t^T)^-1 + (K_t Sigma_{t+1}) K_t^T (lower
        triangle computed, upper mirrored), every product a sum from 0 in ascending index;  sigma = sqrt(diag);  on a
        failed pivot the pixel's outputs are NaN.

    With T = 1 this is ``posterior_cov_numpy`` bit for bit."""
    A, Wm, P, T, M, D = _series_arrays(A, W, prior_prec)
    idx = np.arange(D)
    with np.errstate(all="ignore"):
        Ls, Bs, status = _series_factor_numpy(A, Wm, P, None, None)
        covs = [None] * T
        N = _mirror_lower(_factor_inverse_numpy(Ls[T - 1], status))
        covs[T - 1] = N
        for t in range(T - 2, -1, -1):
            L, B = Ls[t], Bs[t + 1]
            K = np.zeros((M, D, D))
            for k in range(D - 1, -1, -1):                           # column r of K by back substitution, side by side
                s = -B[:, :, k]
                for q in range(k + 1, D):
                    s = s - L[:, q, k][:, None] * K[:, q, :]
                K[:, k, :] = s / L[:, k, k][:, None]
            C = _mirror_lower(_factor_inverse_numpy(L, np.zeros(M, np.int32)))
            F, Kx = np.zeros((M, D, D)), np.zeros((M, D, D))
            for l in range(D):
                F += K[:, :, l, None] * N[:, None, l, :]
            for k in range(D):
                Kx += F[:, :, k, None] * K[:, None, :, k]
            N = _mirror_lower(C + Kx)
            N[status != 0] = np.nan
            covs[t] = N
        cov = np.stack(covs)
        sigma = np.sqrt(cov[:, :, idx, idx])
    return cov, sigma, status


def _quadratic_numpy(d, P):
    """1/2-less ``d^T P d`` per row, outer and inner index ascending as the update kernels sum it."""
    D = d.shape[1]
    q = np.zeros(d.shape[0])
    for i in range(D):
        ri = np.zeros(d.shape[0])
        for c in range(D):
            ri += P[..., i, c] * d[:, c]
        q += d[:, i] * ri
    return q


def series_objective_numpy(X, cost, prior, W):
    """``F`` (M,) of the trajectories ``X`` (T, M, D) with the data terms ``cost`` (T, M): the sum of the costs over t
    ascending, the prior term on date 0, then 1/2 d_t^T W d_t for t ascending -- ``gp_series_update_device``'s order."""
    T, M, D = X.shape
    F = np.zeros(M)
    for t in range(T):
        F = F + cost[t]
    if prior is not None:
        F = F + 0.5 * _quadratic_numpy(X[0] - prior[0], prior[1])
    for t in range(1, T):
        F = F + 0.5 * _quadratic_numpy(X[t] - X[t - 1], W)
    return F


def series_update_numpy(X, trial, cost, cost_t, grad, grad_t, A, A_t, lam, status, state, prior, W, down, up, lam_min,
                        lam_max, ftol, xtol, F_out=None):
    """``gp_series_update_device`` in float64 numpy, in place on ``X`` (T, M, D), ``cost`` (T, M), ``grad``, ``A``,
    ``lam``, ``state`` (and ``F_out`` (M,), the objective of the state each active pixel is left with); returns
    ``accepted`` (M,) int32.  ``prior = (x0, P)`` as ``prior_rows`` returns it, or None; ``W`` (D, D) or (M, D, D)."""
    active = state == 0
    with np.errstate(all="ignore"):
        F, Ft = series_objective_numpy(X, cost, prior, W), series_objective_numpy(trial, cost_t, prior, W)
        accept = active & (np.asarray(status) == 0) & np.isfinite(Ft) & (Ft < F)
        conv = ((F - Ft) <= ftol * F) | (np.max(np.abs(trial - X), axis=(0, 2)) <= xtol)
    reject = active & ~accept
    X[:, accept], cost[:, accept] = trial[:, accept], cost_t[:, accept]
    if grad is not None:
        grad[:, accept] = grad_t[:, accept]
    if A is not None:
        A[:, accept] = A_t[:, accept]
    lam[accept] = np.maximum(lam[accept] * down, lam_min)
    lam[reject] = np.minimum(lam[reject] * up, lam_max)
    state[accept & conv] = 1
    if F_out is not None:
        F_out[accept], F_out[reject] = Ft[accept], F[reject]
    return accept.astype(np.int32)
