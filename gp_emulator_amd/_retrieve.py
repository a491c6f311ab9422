"""The Levenberg-Marquardt loop of ``perband.retrieve_bands`` and ``MultivariateEmulator.retrieve_many``: what belongs
to the loop and to neither emulator type.  The callers keep their argument checks, their uploads and the data term
(a callable); the accept / reject update, the damping, the convergence read-back, the results and the posterior
covariance are stated here once, for the host (``lm_numpy``) and for the device (``lm_device``)."""
import numpy as np

from . import _lib

LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12     # the clamps of the loop's damping


def _prior_term(X, prior):
    """1/2 (x - x0)^T P (x - x0) per row, outer and inner index ascending as lm_update_kernel sums it; ``x0`` (D,) or
    per row (M, D), ``P`` (D, D) or per row (M, D, D)."""
    if prior is None:
        return 0.0
    x0, P = prior
    d = X - x0
    D = d.shape[1]
    q = np.zeros(d.shape[0])
    for i in range(D):
        ri = np.zeros(d.shape[0])
        for c in range(D):
            ri += P[..., i, c] * d[:, c]
        q += d[:, i] * ri
    return 0.5 * q


def _lm_update_numpy(X, trial, cost, cost_t, grad, grad_t, A, A_t, lam, status, state, prior, down, up, lam_min, lam_max,
                     ftol, xtol):
    """``gp_lm_update_device`` in float64 numpy, in place on X, cost, grad, A, lam, state; returns accepted (M,) int32."""
    active = state == 0
    F, Ft = cost + _prior_term(X, prior), cost_t + _prior_term(trial, prior)
    with np.errstate(invalid="ignore"):
        accept = active & (status == 0) & np.isfinite(Ft) & (Ft < F)
        conv = ((F - Ft) <= ftol * F) | (np.max(np.abs(trial - X), axis=1) <= xtol)
    reject = active & ~accept
    X[accept], cost[accept], grad[accept], A[accept] = trial[accept], cost_t[accept], grad_t[accept], A_t[accept]
    lam[accept] = np.maximum(lam[accept] * down, lam_min)
    lam[reject] = np.minimum(lam[reject] * up, lam_max)
    state[accept & conv] = 1
    return accept.astype(np.int32)


def prior_and_bounds(prior, bounds, D, M=1):
    """``prior`` as float64 ``(x0, P)`` -- ``x0`` (D,) or per row (M, D), ``P`` (D, D) or per row (M, D, D) -- and
    ``bounds`` as float64 ``(lo (D,), hi (D,))``; None stays None."""
    if prior is not None:
        prior = _lib.prior_rows(prior, M, D)
    if bounds is not None:
        bounds = (np.asarray(bounds[0], dtype=np.float64).reshape(D), np.asarray(bounds[1], dtype=np.float64).reshape(D))
    return prior, bounds


BOUNDS_MODES = ("clamp", "active_set")


def check_bounds_mode(bounds_mode, bounds, return_active=False):
    """The retrievals' argument rules of the bounds: ``bounds_mode`` is "clamp" (the unconstrained step, clamped) or
    "active_set" (the box step: the minimiser of the damped model inside the box); the latter and ``return_active``
    need ``bounds``."""
    if bounds_mode not in BOUNDS_MODES:
        raise ValueError("bounds_mode must be 'clamp' or 'active_set'")
    if bounds_mode == "active_set" and bounds is None:
        raise ValueError("bounds_mode='active_set' needs bounds")
    if return_active and bounds is None:
        raise ValueError("return_active needs bounds")


def clamp_only(bounds_mode):
    """The joint retrievals' rule: their block-tridiagonal step has the clamp only."""
    if bounds_mode != "clamp":
        raise ValueError("the joint retrieval offers bounds_mode='clamp' only")


def numpy_step(prior, bounds, bounds_mode):
    """The host loop's step: ``(x, grad, A, lam) -> (step, trial, status, ...)`` by ``newton_step_numpy`` or, with
    ``bounds_mode="active_set"``, ``box_step_numpy`` (diagonal damping)."""
    form = _lib.box_step_numpy if bounds_mode == "active_set" else _lib.newton_step_numpy
    return lambda x, g, A, lam: form(x, g, A, lam, "diagonal", prior, bounds)


def lm_numpy(data_term, step, X0, lam0, max_iter, down, up, ftol, xtol, prior, return_cov, next_prior=None, return_A=False,
             active_bounds=None):
    """The loop on the host in float64: ``data_term(X) -> (cost, grad, A)``, ``step(x, grad, A, lam) -> (step, trial,
    status)``.  Returns ``(X, cost, state, n_accepted, lam)``, with ``return_cov`` ``_lib.posterior_cov_numpy``'s
    three of the loop's ``A`` behind them, and with a process noise ``next_prior`` ``_lib.prior_propagate_numpy``'s
    two behind those; ``return_A`` appends the loop's final data-term matrix ``A (M, D, D)`` behind those (what
    the smoother of a series needs of a date); ``active_bounds=(lo, hi)`` (the callers' ``return_active``) appends
    ``_lib.active_set_numpy``'s two of the returned ``X`` and the loop's final ``grad``, ``A`` and prior as the last
    elements.  Only the first three of what ``step`` returns are read."""
    M = X0.shape[0]
    X = np.array(X0, dtype=np.float64)
    lam = np.full(M, float(lam0))
    state, n_acc = np.zeros(M, np.int32), np.zeros(M, np.int32)
    cost, grad, A = (np.array(a) for a in data_term(X))
    for it in range(max_iter):
        _, trial, status = step(X, grad, A, lam)[:3]
        trial = np.asarray(trial, dtype=np.float64)
        cost_t, grad_t, A_t = data_term(trial)
        n_acc += _lm_update_numpy(X, trial, cost, cost_t, grad, grad_t, A, A_t, lam, np.asarray(status), state, prior,
                                  down, up, LAMBDA_MIN, LAMBDA_MAX, ftol, xtol)
        if it % 4 == 3 and np.all(state == 1):
            break
    out = (X, cost, state, n_acc, lam)
    if return_cov:
        out += _lib.posterior_cov_numpy(A, prior[1] if prior is not None else None)
    if next_prior is not None:
        out += _lib.prior_propagate_numpy(A, prior[1] if prior is not None else None, next_prior)
    if return_A:
        out += (A,)
    if active_bounds is not None:
        out += _lib.active_set_numpy(X, grad, A, prior, active_bounds)
    return out


Scratch = _lib.Scratch     # the device arrays of one call (the loop's callers open it; tests take it from here)


def lm_device(scratch, M, D, X0, lam0, prior, bounds, max_iter, down, up, ftol, xtol, return_cov, misfit, next_prior=None,
              return_A=False, bounds_mode="clamp", return_active=False):
    """The loop on the device from the host rows ``X0``, in the precision and on the context of ``scratch`` (the
    caller's ``Scratch``, which also holds whatever ``misfit`` reads).  ``misfit(d_rows, d_cost, d_grad, d_A)`` enqueues
    the data term at ``d_rows`` on the context's stream.  Every iteration is that, ``lm_update_device`` and
    ``newton_step_device``; nothing comes back inside the loop but ``state``, every fourth iteration, to stop when every
    row has converged.  With a per-row prior -- ``x0`` (M, D) or ``P`` (M, D, D) -- the two are the ``_rows`` entries
    with the arrays' row strides; with a shared or absent prior the calls are exactly the plain ones.  A process noise
    ``next_prior`` (D, D) or (M, D, D) adds one ``prior_propagate_device`` call after the loop (and after the
    covariance) on the loop's own ``d_A`` and ``d_P``; ``return_A`` adds one download, of ``d_A``, behind everything
    else.  ``bounds_mode="active_set"`` calls ``box_step_device`` where the Newton step is called (one entry for the
    shared and the per-row prior: the strides say which); ``"clamp"`` makes exactly the calls it always made.
    ``return_active`` adds one download, of ``d_grad`` (and of ``d_A`` unless ``return_A`` brought it), and appends
    ``_lib.active_set_numpy``'s two, in float64 numpy from the downloaded arrays.  Returns what ``lm_numpy`` returns, in
    the scratch's precision."""
    check_bounds_mode(bounds_mode, bounds, return_active)
    ctx, dt = scratch.ctx, scratch.dt
    up_, alloc, isz = scratch.up, scratch.alloc, dt.itemsize
    d_x, d_lam = up_(X0), up_(np.full(M, float(lam0)))
    d_x0, d_P = (up_(prior[0]), up_(prior[1])) if prior is not None else (None, None)
    d_lo, d_hi = (up_(bounds[0]), up_(bounds[1])) if bounds is not None else (None, None)
    d_cost, d_grad, d_A = alloc(M * isz), alloc(M * D * isz), alloc(M * D * D * isz)
    d_cost_t, d_grad_t, d_A_t = alloc(M * isz), alloc(M * D * isz), alloc(M * D * D * isz)
    d_trial, d_status, d_state = alloc(M * D * isz), alloc(M * 4), alloc(M * 4)
    d_acc = alloc(max_iter * M * 4)            # one (M,) slice per iteration, summed after the loop
    _lib.check(ctx.lib.gp_memset(ctx.h, d_state, 0, M * 4), "gp_memset")

    strides = _lib.row_strides(*prior) if prior is not None else (0, 0)
    rows = any(strides)

    def newton():
        if bounds_mode == "active_set":
            ctx.box_step_device(dt, d_x, d_grad, d_A, d_lam, None, d_trial, d_status, M, D, d_lo, d_hi, "diagonal", d_x0, d_P,
                                strides[0], strides[1])
        elif rows:
            ctx.newton_step_rows_device(dt, d_x, d_grad, d_A, d_lam, None, d_trial, d_status, M, D, "diagonal", d_x0,
                                        d_P, d_lo, d_hi, strides[0], strides[1])
        else:
            ctx.newton_step_device(dt, d_x, d_grad, d_A, d_lam, None, d_trial, d_status, M, D, "diagonal", d_x0, d_P,
                                   d_lo, d_hi)
    misfit(d_x, d_cost, d_grad, d_A)
    newton()
    done = 0
    for it in range(max_iter):
        misfit(d_trial, d_cost_t, d_grad_t, d_A_t)
        update = (dt, d_x, d_trial, d_cost, d_cost_t, d_grad, d_grad_t, d_A, d_A_t, d_lam, d_status, d_state,
                  _lib.c_void_p(d_acc.value + it * M * 4), M, D, d_x0, d_P, down, up, LAMBDA_MIN, LAMBDA_MAX, ftol, xtol)
        if rows:
            ctx.lm_update_rows_device(*update + strides)
        else:
            ctx.lm_update_device(*update)
        newton()
        done = it + 1
        if it % 4 == 3:                       # (the copy synchronises the stream first)
            ctx.synchronize()
            if np.all(np.asarray(ctx.to_host(d_state, (M,), np.int32)) == 1):
                break
    ctx.synchronize()
    X, cost, lam = (np.array(ctx.to_host(p, s, dt)) for p, s in ((d_x, (M, D)), (d_cost, (M,)), (d_lam, (M,))))
    state = np.array(ctx.to_host(d_state, (M,), np.int32))
    n_acc = np.array(ctx.to_host(d_acc, (done, M), np.int32)).sum(axis=0, dtype=np.int32) if done else np.zeros(M, np.int32)
    out = (X, cost, state, n_acc, lam)
    if return_cov:
        d_cov, d_sigma, d_cstat = alloc(M * D * D * isz), alloc(M * D * isz), alloc(M * 4)
        if strides[1]:
            ctx.posterior_cov_rows_device(dt, d_A, d_P, d_cov, d_sigma, d_cstat, M, D, strides[1])
        else:
            ctx.posterior_cov_device(dt, d_A, d_P, d_cov, d_sigma, d_cstat, M, D)
        ctx.synchronize()
        out += (np.array(ctx.to_host(d_cov, (M, D, D), dt)), np.array(ctx.to_host(d_sigma, (M, D), dt)),
                np.array(ctx.to_host(d_cstat, (M,), np.int32)))
    if next_prior is not None:
        Q = _lib.prec_rows(next_prior, M, D)
        d_Q, d_next, d_pstat = up_(Q), alloc(M * D * D * isz), alloc(M * 4)
        ctx.prior_propagate_device(dt, d_A, d_P, strides[1], d_Q, _lib.row_strides(None, Q)[1], d_next, d_pstat, M, D)
        ctx.synchronize()
        out += (np.array(ctx.to_host(d_next, (M, D, D), dt)), np.array(ctx.to_host(d_pstat, (M,), np.int32)))
    A_host = np.array(ctx.to_host(d_A, (M, D, D), dt)) if return_A or return_active else None
    if return_A:
        out += (A_host,)
    if return_active:
        out += _lib.active_set_numpy(X, np.array(ctx.to_host(d_grad, (M, D), dt)), A_host, prior, bounds)
    return out


def lm_series_numpy(data_term, X0, W, lam0, prior, bounds, max_iter, down, up, ftol, xtol, return_cov):
    """The loop over whole trajectories on the host in float64: the joint objective of DESIGN.md §4.23 from ``X0``
    (T, M, D).  ``data_term(rows (T M, D)) -> (cost, grad, A)`` is one call on all dates' rows, date-major; the step is
    ``_lib.series_step_numpy`` (diagonal damping), the decision ``_lib.series_update_numpy``, on ``lm_numpy``'s
    schedule and constants.  ``W`` is the precision of the process noise, ``prior`` date 0's (as ``prior_and_bounds``
    returns it).  Returns ``(X (T, M, D), sigma (T, M, D), cost (T, M), F (M,), state, n_accepted, lam, cov_status)``,
    with ``return_cov`` ``cov (T, M, D, D)`` behind them: ``_lib.series_cov_numpy`` of the loop's ``A``.  ``F`` is the
    joint objective the last decision left a pixel with (NaN for a pixel no decision was made for)."""
    T, M, D = X0.shape

    def term(X):
        cost, grad, A = data_term(X.reshape(T * M, D))
        return np.array(cost).reshape(T, M), np.array(grad).reshape(T, M, D), np.array(A).reshape(T, M, D, D)
    X = np.array(X0, dtype=np.float64)
    lam, F = np.full(M, float(lam0)), np.full(M, np.nan)
    state, n_acc = np.zeros(M, np.int32), np.zeros(M, np.int32)
    cost, grad, A = term(X)
    for it in range(max_iter):
        _, trial, status = _lib.series_step_numpy(X, grad, A, lam, W, "diagonal", prior, bounds)
        cost_t, grad_t, A_t = term(trial)
        n_acc += _lib.series_update_numpy(X, trial, cost, cost_t, grad, grad_t, A, A_t, lam, status, state, prior, W, down, up,
                                          LAMBDA_MIN, LAMBDA_MAX, ftol, xtol, F_out=F)
        if it % 4 == 3 and np.all(state == 1):
            break
    cov, sigma, cstat = _lib.series_cov_numpy(A, W, prior[1] if prior is not None else None)
    return (X, sigma, cost, F, state, n_acc, lam, cstat) + ((cov,) if return_cov else ())


def lm_series_device(scratch, X0, W, lam0, prior, bounds, max_iter, down, up, ftol, xtol, return_cov, misfit):
    """``lm_series_numpy`` on the device, in the precision and on the context of ``scratch``: ``misfit(d_rows, d_cost,
    d_grad, d_A)`` enqueues the data term of the T M date-major rows at ``d_rows``.  Every iteration is that,
    ``series_update_device`` and ``series_step_device`` on the one stream; nothing comes back inside the loop but
    ``state``, every fourth iteration.  After the loop one ``series_cov_device`` call on the loop's own arrays.  The
    work memory of the two kernels is allocated once, in the scratch: the caller slices the pixels under its budget."""
    ctx, dt = scratch.ctx, scratch.dt
    up_, alloc, isz = scratch.up, scratch.alloc, dt.itemsize
    T, M, D = X0.shape
    R = T * M
    d_x, d_lam, d_F = up_(X0), up_(np.full(M, float(lam0))), up_(np.full(M, np.nan))
    d_x0, d_P = (up_(prior[0]), up_(prior[1])) if prior is not None else (None, None)
    d_lo, d_hi = (up_(bounds[0]), up_(bounds[1])) if bounds is not None else (None, None)
    d_W, ws = up_(W), _lib.row_strides(None, W)[1]
    d_cost, d_grad, d_A = alloc(R * isz), alloc(R * D * isz), alloc(R * D * D * isz)
    d_cost_t, d_grad_t, d_A_t = alloc(R * isz), alloc(R * D * isz), alloc(R * D * D * isz)
    d_trial, d_status, d_state = alloc(R * D * isz), alloc(M * 4), alloc(M * 4)
    d_acc = alloc(max(1, max_iter) * M * 4)    # one (M,) slice per iteration, summed after the loop
    nbytes = _lib.series_work_bytes(M, T, D)
    d_work = alloc(nbytes)
    _lib.check(ctx.lib.gp_memset(ctx.h, d_state, 0, M * 4), "gp_memset")
    ms, ps = _lib.row_strides(*prior) if prior is not None else (0, 0)

    def step():
        ctx.series_step_device(dt, d_x, d_grad, d_A, d_lam, d_W, ws, None, d_trial, d_status, d_work, nbytes, M, T, D,
                               "diagonal", d_x0, d_P, d_lo, d_hi, ms, ps)
    misfit(d_x, d_cost, d_grad, d_A)
    step()
    done = 0
    for it in range(max_iter):
        misfit(d_trial, d_cost_t, d_grad_t, d_A_t)
        ctx.series_update_device(dt, d_x, d_trial, d_cost, d_cost_t, d_grad, d_grad_t, d_A, d_A_t, d_lam, d_status, d_state,
                                 _lib.c_void_p(d_acc.value + it * M * 4), d_F, d_W, ws, M, T, D, d_x0, d_P, down, up,
                                 LAMBDA_MIN, LAMBDA_MAX, ftol, xtol, ms, ps)
        step()
        done = it + 1
        if it % 4 == 3:                       # (the copy synchronises the stream first)
            ctx.synchronize()
            if np.all(np.asarray(ctx.to_host(d_state, (M,), np.int32)) == 1):
                break
    d_cov = alloc(R * D * D * isz) if return_cov else None
    d_sigma, d_cstat = alloc(R * D * isz), alloc(M * 4)
    ctx.series_cov_device(dt, d_A, d_P, ps, d_W, ws, d_cov, d_sigma, d_cstat, d_work, nbytes, M, T, D)
    ctx.synchronize()
    down_ = lambda p, shape, t=dt: np.array(ctx.to_host(p, shape, t))
    n_acc = down_(d_acc, (done, M), np.int32).sum(axis=0, dtype=np.int32) if done else np.zeros(M, np.int32)
    out = (down_(d_x, (T, M, D)), down_(d_sigma, (T, M, D)), down_(d_cost, (T, M)), down_(d_F, (M,)),
           down_(d_state, (M,), np.int32), n_acc, down_(d_lam, (M,)), down_(d_cstat, (M,), np.int32))
    return out + ((down_(d_cov, (T, M, D, D)),) if return_cov else ())


def series_precision(noise, M, D, context=None, dt=np.float64):
    """``W = Q^-1`` for the process noise ``noise`` (D, D) or (M, D, D), inverted once: on the device ``context`` with
    ``gp_posterior_cov_device(A = Q)`` in the precision ``dt``, without one by ``_lib.posterior_cov_numpy``.  A shared
    ``Q`` that does not factor raises ``ValueError``; a pixel's own that does not leaves that pixel a NaN ``W``."""
    Q = _lib.prec_rows(noise, M, D)
    rows = Q if Q.ndim == 3 else Q[None]
    if context is None:
        W, _, status = _lib.posterior_cov_numpy(rows)
    else:
        W, _, status = context.posterior_cov(np.ascontiguousarray(rows, dtype=dt), None, precision=dt)
    if Q.ndim == 2:
        if status[0] != 0:
            raise ValueError("noise is not positive definite (pivot %d fails): the joint form needs its inverse" % (status[0] - 1))
        return W[0]
    return W


JOINT_AXES = (1, 1, 1, 0, 0, 0, 0, 0, 1)     # the pixel axis of what the joint loops return


def retrieve_joint(X0, prior, noise, bounds, lam0, max_iter, down, up, ftol, xtol, return_cov, numpy_term=None,
                   device_term=None, context=None, precision=np.float64, work_budget=None):
    """The joint retrieval of both emulator types behind their argument checks: ``X0`` (T, M, D).  On the host
    (``numpy_term(m0, m1)`` gives the data term of those pixels' T (m1 - m0) date-major rows) one ``lm_series_numpy``.
    On the device ``context`` the pixels are cut into runs whose work memory stays under ``work_budget`` bytes
    (``_lib.series_slices``) and every run is one ``lm_series_device`` in a scratch of its own, its data term from
    ``device_term(scratch, m0, m1)``; pixels are independent, so the cut changes no bit."""
    T, M, D = X0.shape
    prior, bounds = prior_and_bounds(prior, bounds, D, M)
    max_iter = int(max_iter)
    if numpy_term is not None:
        W = series_precision(noise, M, D)
        return lm_series_numpy(numpy_term(0, M), X0, W, lam0, prior, bounds, max_iter, down, up, ftol, xtol, return_cov)
    dt = np.dtype(precision)
    W = series_precision(noise, M, D, context, dt)
    budget = _lib.SERIES_WORK_BUDGET if work_budget is None else work_budget
    parts = []
    for m0, m1 in _lib.series_slices(M, T, D, budget):
        cut = lambda a, nd: np.ascontiguousarray(a[m0:m1]) if a.ndim == nd else a
        with Scratch(context, dt) as scratch:
            parts.append(lm_series_device(scratch, np.ascontiguousarray(X0[:, m0:m1]), cut(W, 3), lam0,
                                          (cut(prior[0], 2), cut(prior[1], 3)), bounds, max_iter, down, up, ftol, xtol,
                                          return_cov, device_term(scratch, m0, m1)))
    return tuple(np.concatenate([p[k] for p in parts], axis=ax) for k, ax in zip(range(len(parts[0])), JOINT_AXES))


def joint_start(X0, T, name="X0"):
    """``X0`` (T, M, D), or (M, D) taken for every date, as a float64 (T, M, D) array."""
    X0 = np.asarray(X0, dtype=np.float64)
    if X0.ndim == 2:
        X0 = np.broadcast_to(X0, (T,) + X0.shape)
    if X0.ndim != 3 or X0.shape[0] != T:
        raise ValueError("%s must be (n_rows, n_inputs) or (%d, n_rows, n_inputs), got %s" % (name, T, X0.shape))
    return np.ascontiguousarray(X0)


def smooth_numpy(A, P, noise, X, cov_last, sigma_last, bounds):
    """The backward pass of a series on the host: ``_lib.rts_smooth_numpy`` for t = T-2 .. 0 on the dates' ``A[t]``,
    ``P[t]`` and filtered states ``X[t]``, started from the last date's state and covariance.  Returns ``(X_s (T, M, D),
    sigma_s (T, M, D), status (T, M) int32)``; the last date's are the filtered ones and zeros."""
    T = len(A)
    xs, cov = np.asarray(X[T - 1], dtype=np.float64), cov_last
    keep = [(xs, np.asarray(sigma_last, dtype=np.float64), np.zeros(xs.shape[0], np.int32))]
    for t in range(T - 2, -1, -1):
        xs, cov, sig, status = _lib.rts_smooth_numpy(A[t], P[t], noise, X[t], xs, cov, bounds)
        keep.append((xs, sig, status))
    return tuple(np.stack(a) for a in zip(*keep[::-1]))


def smooth_device(ctx, dt, A, P, noise, X, cov_last, sigma_last, bounds):
    """The backward pass of a series on the device in the precision ``dt``: one ``rts_smooth_device`` call per date,
    t = T-2 .. 0.  The smoothed state and covariance of date t + 1 stay on the device: two buffer pairs take turns as
    the call's input and output.  The noise and the bounds go up once; per date only ``A[t]``, ``P[t]`` and ``X[t]`` go
    up and only the smoothed state, its sigma and the status come down.  Returns what ``smooth_numpy`` returns, in
    ``dt``."""
    T = len(A)
    M, D = np.shape(X[T - 1])
    isz = dt.itemsize
    keep = [(np.array(X[T - 1], dtype=dt), np.array(sigma_last, dtype=dt), np.zeros(M, np.int32))]
    if T == 1:
        return tuple(np.stack(a) for a in zip(*keep))
    with Scratch(ctx, dt) as scratch:
        up_, alloc = scratch.up, scratch.alloc
        Q = _lib.prec_rows(noise, M, D)
        d_Q, q_stride = up_(Q), _lib.row_strides(None, Q)[1]
        d_lo, d_hi = (up_(bounds[0]), up_(bounds[1])) if bounds is not None else (None, None)
        d_A, d_P, d_x = alloc(M * D * D * isz), alloc(M * D * D * isz), alloc(M * D * isz)
        pairs = [(up_(X[T - 1]), up_(cov_last)), (alloc(M * D * isz), alloc(M * D * D * isz))]
        d_sigma, d_status = alloc(M * D * isz), alloc(M * 4)
        for n, t in enumerate(range(T - 2, -1, -1)):
            nxt, cur = pairs[n % 2], pairs[(n + 1) % 2]
            Pt = _lib.prec_rows(P[t], M, D, dt)
            ctx.h2d(d_A, np.ascontiguousarray(A[t], dtype=dt))
            ctx.h2d(d_P, Pt)
            ctx.h2d(d_x, np.ascontiguousarray(X[t], dtype=dt))
            ctx.rts_smooth_device(dt, d_A, d_P, _lib.row_strides(None, Pt)[1], d_Q, q_stride, d_x, nxt[0], nxt[1], d_lo, d_hi,
                                  cur[0], cur[1], d_sigma, d_status, M, D)
            ctx.synchronize()
            keep.append((np.array(ctx.to_host(cur[0], (M, D), dt)), np.array(ctx.to_host(d_sigma, (M, D), dt)),
                         np.array(ctx.to_host(d_status, (M,), np.int32))))
    return tuple(np.stack(a) for a in zip(*keep[::-1]))


def retrieve_series(retrieve, X0, obs, weights, prior, noise, smooth=False, context=None, **loop_args):
    """A time series of retrievals, date after date, each date's posterior the next date's prior (random-walk
    dynamics: the next prior mean is the retrieved state, the next prior precision ``((A + P)^-1 + Q)^-1`` with the
    process noise ``Q = noise`` (D, D) or (M, D, D)).  ``retrieve(X0, obs, weights, prior=, return_cov=, next_prior=,
    **loop_args)`` is one date's retrieval (``retrieve_bands`` on its emulators, or ``retrieve_many``); ``obs`` and
    ``weights`` carry a leading date axis T (``weights`` may be None).  ``prior`` is required: it keeps ``A + P``
    positive definite for the pixels without a valid observation on a date.  Date 0 starts from ``X0`` with ``prior``,
    date t from ``X[t - 1]`` with ``(X[t - 1], next_prec[t - 1])``.

    Returns ``(X (T, M, D), sigma (T, M, D), cost (T, M), state (T, M), cov_status (T, M), prior_status (T, M),
    next_prec (M, D, D))``, the last the prior precision for the date after the series.  A host loop over the dates:
    the state goes down and up once per date.

    That is a forward filter: date t has seen the observations up to t only.  ``smooth=True`` adds the fixed-interval
    (Rauch-Tung-Striebel) backward pass over the filtered posteriors and appends ``X_s (T, M, D)``, ``sigma_s
    (T, M, D)`` and ``smooth_status (T, M) int32`` to the seven: for t = T-2 .. 0, with ``C = (A[t] + P[t])^-1``,
    ``S = C + Q`` and ``G = C S^-1``, ``X_s[t] = X[t] + G (X_s[t + 1] - X[t])`` (clamped to the series' ``bounds``) and
    ``C_s[t] = C + G (C_s[t + 1] - S) G^T``, ``sigma_s[t]`` the square roots of its diagonal; the last date's are the
    filtered ones and its status zeros; a status is ``prior_status``' code of that date's two inversions, and then the
    row's smoothed values are NaN.  The forward pass then also keeps, per date, the loop's matrix ``A[t]`` (the
    retrievals' ``return_A=True``) and the prior precision ``P[t]`` the date was retrieved with, and the last date's
    covariance; the first seven values are those of ``smooth=False``.  ``context`` is a callable that returns the
    ``_lib.Context`` of the forward pass: the backward pass is then ``smooth_device`` in ``loop_args``' precision;
    with ``None`` it is ``smooth_numpy``, the explicit host branch.  With ``smooth=False`` nothing changes."""
    if prior is None:
        raise ValueError("a series needs a prior")
    T = len(obs)
    if T == 0:
        raise ValueError("obs has no dates")
    if weights is not None and len(weights) != T:
        raise ValueError("obs has %d dates, weights %d" % (T, len(weights)))
    for name in ("prior", "return_cov", "next_prior") + (("return_A",) if smooth else ()):
        if name in loop_args:
            raise ValueError("%s is the series' own argument" % name)
    more = dict(return_A=True) if smooth else {}
    X, keep, next_prec, mats, cov = X0, [], None, [], None
    for t in range(T):
        out = retrieve(X, obs[t], weights[t] if weights is not None else None, prior=prior, return_cov=True,
                       next_prior=noise, **dict(loop_args, **more))
        if smooth:
            mats.append((out[10], prior[1]))
            cov = out[5]
        X, next_prec = out[0], out[8]
        keep.append((X, out[6], out[1], out[2], out[7], out[9]))
        prior = (X, next_prec)
    result = tuple(np.stack(a) for a in zip(*keep)) + (next_prec,)
    if not smooth:
        return result
    A, P = zip(*mats)
    bounds = loop_args.get("bounds")
    if context is None:
        return result + smooth_numpy(A, P, noise, result[0], cov, result[1][T - 1], bounds)
    dt = np.dtype(loop_args.get("precision", np.float64))
    return result + smooth_device(context(), dt, A, P, noise, result[0], cov, result[1][T - 1], bounds)
