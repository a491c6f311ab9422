"""Per-band emulators predicted together.

The reference's per-band pattern (tests/test_perband_emulator.py:22-37) builds one
``GaussianProcess`` per spectral band on the SAME training inputs ``y_train`` -- each with
its own targets, theta, invQ, invQt -- and then calls ``gp.predict(X, is_gpu=True)`` band by
band (:48-50).  ``predict_bands`` runs all of them over the shared test rows in one launch
of the fused kernel (BASELINE config 3: 2101 bands x N_train=250 x D=11, shared test set).
"""
import numpy as np

from . import _lib, _retrieve
from ._retrieve import LAMBDA_MAX, LAMBDA_MIN, _lm_update_numpy, _prior_term     # noqa: F401  (their names here)


def _check_shared_inputs(gps):
    if not gps:
        raise ValueError("need at least one GaussianProcess")
    inputs = np.asarray(gps[0].inputs)
    for gp in gps[1:]:
        other = np.asarray(gp.inputs)
        if other.shape != inputs.shape or not np.array_equal(other, inputs):
            raise ValueError("per-band emulators must share the same training inputs")
    return inputs


def _batch_model(ctx, gps, inputs, precision, do_unc):
    """The BatchModel of a block of emulators on ``inputs``; ``do_unc=False`` stacks and uploads no invQ."""
    return _lib.BatchModel(ctx, np.stack([np.exp(gp.theta) for gp in gps]), inputs,
                           np.stack([np.asarray(gp.invQt) for gp in gps]),
                           np.stack([np.asarray(gp.invQ) for gp in gps]) if do_unc else None, precision)


def make_batch(gps, precision=np.float64, device=None, do_unc=True):
    """Pack a list of GaussianProcess objects sharing ``inputs`` into one BatchModel.  ``do_unc=False``:
    no invQ is stacked or uploaded (2101 bands x 250^2 x 8 B = 1.05 GB); the batch then serves
    ``predict_mean_grad`` only."""
    inputs = _check_shared_inputs(gps)
    return _batch_model(_lib.default_context(device), gps, inputs, precision, do_unc)


def predict_bands(gps, testing, precision=np.float64, device=None, devices=None, predict_fn=None, do_unc=True):
    """mu (E, M), var (E, M), deriv (E, M, D) for the E emulators in ``gps``.

    ``devices`` (a list of device ids) shards the EMULATORS over the GPUs of a node -- BASELINE
    config 3's other partition: GPU g takes a contiguous block of the E
    bands with the shared test rows replicated (8.8 MB for 1e5 rows) instead of every GPU holding
    all E inverses (1 GB for 2101 bands).  One Python thread and one context per device (the C
    ABI releases the GIL), every device's slab pipeline writing its own ``[e0:e1]`` slice of the
    three output arrays: a host gather, no collective.  ``predict_fn(device, gps_block, testing)
    -> (mu, var, deriv)`` replaces the HIP path in the CPU tests of the sharding logic.

    ``do_unc=False``: mu (E, M) and deriv (E, M, D) only, from the mean+gradient kernels (bit for
    bit those of ``do_unc=True``); no invQ is stacked or uploaded, and ``predict_fn`` then
    returns ``(mu, deriv)``."""
    testing = np.asarray(testing)
    if devices is None:
        batch = make_batch(gps, precision, device, do_unc=do_unc)
        try:
            return batch.predict(testing) if do_unc else batch.predict_mean_grad(testing)
        finally:
            batch.close()
    from . import multi_gpu
    if not gps:
        raise ValueError("need at least one GaussianProcess")
    E, (M, D) = len(gps), testing.shape
    dt = np.float64 if (testing.dtype == np.float64 or np.dtype(precision) == np.float64) else np.float32
    mu, deriv = np.empty((E, M), dt), np.empty((E, M, D), dt)
    var = np.empty((E, M), dt) if do_unc else None
    blocks = multi_gpu.row_shards(E, len(devices))       # contiguous blocks of emulators
    inputs = _check_shared_inputs(gps)

    def work(k, dev, e0, e1):
        if predict_fn is not None:
            if do_unc:
                mu[e0:e1], var[e0:e1], deriv[e0:e1] = predict_fn(dev, gps[e0:e1], testing)
            else:
                mu[e0:e1], deriv[e0:e1] = predict_fn(dev, gps[e0:e1], testing)
            return
        ctx, lock = multi_gpu._device_context(dev)
        with lock:
            batch = _batch_model(ctx, gps[e0:e1], inputs, precision, do_unc)
            try:
                if do_unc:
                    batch.predict(testing, out=(mu[e0:e1], var[e0:e1], deriv[e0:e1]))
                else:
                    batch.predict_mean_grad(testing, out=(mu[e0:e1], deriv[e0:e1]))
            finally:
                batch.close()

    multi_gpu.run_shards(devices, blocks, work)
    return (mu, var, deriv) if do_unc else (mu, deriv)


def variance_gradient_bands(gps, X, precision=np.float64, device=None):
    """var (E, M) and dvar (E, M, D): the predictive variance of the E emulators in ``gps`` at the shared rows ``X``
    (M, D) and its gradient with respect to the row, in one launch per 2^20 rows (``BatchModel.predict_var_grad``).
    Arrays of ``precision``; emulator e bit for bit what ``Model.predict_var_grad`` of it gives."""
    batch = make_batch(gps, precision, device)
    try:
        return batch.predict_var_grad(np.asarray(X))
    finally:
        batch.close()


def hessian_bands(gps, testing, precision=np.float64, weights=None, device=None, devices=None, hessian_fn=None):
    """Hessians of the E emulators' means over shared test rows: ``(E, M, D, D)``, or with ``weights``
    ``(E, M)`` the weighted sum over the emulators ``sum_e weights[e, m] * H_e[m]``, ``(M, D, D)`` -- the
    second-derivative term of a spectral cost function, summed on the device (the per-band result of 2101
    bands x 1e5 rows could never be stored).  One batched launch per slab of rows (``BatchModel.hessian`` /
    ``hessian_weighted``); no inverse is stacked or uploaded.

    ``devices`` shards the EMULATORS like ``predict_bands``: device g takes a contiguous block.  Unweighted,
    every device writes its own ``[e0:e1]`` slice; weighted, every device returns the partial sum of its block
    and the partial sums are added on the host in device order (so the result does not depend on which device
    finishes first).  ``hessian_fn(device, gps_block, testing[, weights_block])`` replaces the HIP path in the
    CPU tests of the sharding logic."""
    testing = np.asarray(testing)
    if testing.ndim != 2:
        raise ValueError("testing must be (n_predict, n_inputs)")
    inputs = _check_shared_inputs(gps)
    E, (M, D) = len(gps), testing.shape
    if D != inputs.shape[1]:
        raise ValueError("testing has %d columns, the emulators have %d inputs" % (D, inputs.shape[1]))
    if weights is not None:
        weights = np.asarray(weights)
        if weights.shape != (E, M):
            raise ValueError("weights must be (%d, %d), got %s" % (E, M, weights.shape))
    if devices is None:
        if hessian_fn is not None:
            return hessian_fn(device, gps, testing) if weights is None else hessian_fn(device, gps, testing, weights)
        batch = make_batch(gps, precision, device, do_unc=False)
        try:
            return batch.hessian(testing) if weights is None else batch.hessian_weighted(testing, weights)
        finally:
            batch.close()
    from . import multi_gpu
    if len(devices) < 1:
        raise ValueError("devices must name at least one device")
    dt = np.float64 if (testing.dtype == np.float64 or np.dtype(precision) == np.float64) else np.float32
    blocks = multi_gpu.row_shards(E, len(devices))       # contiguous blocks of emulators
    out = np.empty((E, M, D, D), dt) if weights is None else None
    partial = [None] * len(devices)

    def work(k, dev, e0, e1):
        part = gps[e0:e1]
        if hessian_fn is not None:
            if weights is None:
                out[e0:e1] = hessian_fn(dev, part, testing)
            else:
                partial[k] = np.asarray(hessian_fn(dev, part, testing, weights[e0:e1]))
            return
        ctx, lock = multi_gpu._device_context(dev)
        with lock:
            batch = _batch_model(ctx, part, inputs, precision, False)
            try:
                if weights is None:
                    batch.hessian(testing, out=out[e0:e1])
                else:
                    partial[k] = np.array(batch.hessian_weighted(testing, weights[e0:e1]))   # (own memory, not the pool's)
            finally:
                batch.close()

    multi_gpu.run_shards(devices, blocks, work)
    if weights is None:
        return out
    total = np.zeros((M, D, D), dt)
    for part in partial:                      # device order
        if part is not None:
            total += part
    return total


def _em_broadcast(a, E, M, name):
    """An (E,) or (E, M) array as (E, 1) or (E, M) float64."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape == (E,):
        return a[:, None]
    if a.shape == (E, M):
        return a
    raise ValueError("%s must be (%d,) or (%d, %d), got %s" % (name, E, E, M, a.shape))


def _misfit_numpy(gps, X, obs, weights, second_order, return_residual):
    """The formulas as they stand, emulator after emulator, from ``cpu_predict`` and ``hessian``."""
    E, (M, D) = len(gps), X.shape
    cost, grad = np.zeros(M), np.zeros((M, D))
    second = np.zeros((M, D, D)) if second_order else None
    wr = np.empty((E, M)) if return_residual else None
    for e, gp in enumerate(gps):
        mu, deriv = gp.cpu_predict(X, do_unc=False)
        w = np.broadcast_to(weights[e], (M,)) if weights is not None else np.ones(M)
        r = mu - np.broadcast_to(obs[e], (M,))
        cost += 0.5 * w * r * r
        grad += (w * r)[:, None] * deriv
        if second_order:
            second += w[:, None, None] * (deriv[:, :, None] * deriv[:, None, :])     # (exactly symmetric)
        if second_order == "full":
            second += (w * r)[:, None, None] * gp.hessian(X)
        if return_residual:
            wr[e] = w * r
    out = (cost, grad)
    if second_order:
        out += (second,)
    if return_residual:
        out += (wr,)
    return out


def misfit_bands(gps, X, obs, weights=None, second_order=None, return_residual=False, is_gpu=True,
                 precision=np.float64, device=None, devices=None, misfit_fn=None):
    """Data term of a variational retrieval on E per-band emulators over shared rows ``X`` (M, D):

        r[e, m] = mu_e(x_m) - obs[e, m]            w = 1 without ``weights``
        cost[m] = 1/2 sum_e w r^2                  grad[m] = sum_e w r dmu_e/dx
        gn[m]   = sum_e w dmu_e/dx dmu_e/dx^T      hess[m] = gn[m] + sum_e w r H_e[m]

    Returns ``cost (M,), grad (M, D)``, then ``gn`` (``second_order="gauss_newton"``) or ``hess`` (``"full"``)
    ``(M, D, D)``, then with ``return_residual`` ``wr = w r (E, M)`` -- the ``weights`` of ``hessian_bands``.
    ``obs`` and ``weights`` are ``(E,)`` (one spectrum for all rows) or ``(E, M)``.  On the GPU
    (``BatchModel.misfit``, ``gp_band_misfit_host``) the per-emulator means, gradients and residuals never leave the
    device; no inverse is stacked or uploaded.  ``is_gpu=False`` is the explicit numpy branch, built from each
    emulator's ``cpu_predict(do_unc=False)`` and ``hessian``; never a fallback.

    ``devices`` shards the EMULATORS like ``hessian_bands``: every device returns the partial sums of its block and
    they are added on the host in device order (``wr`` rows are the blocks' own).  ``misfit_fn(device, gps_block, X,
    obs_block, weights_block, second_order, return_residual)`` replaces the HIP path in the CPU tests of that logic."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be (n_rows, n_inputs)")
    if second_order not in (None, "gauss_newton", "full"):
        raise ValueError("second_order must be None, 'gauss_newton' or 'full'")
    inputs = _check_shared_inputs(gps)
    E, (M, D) = len(gps), X.shape
    if D != inputs.shape[1]:
        raise ValueError("X has %d columns, the emulators have %d inputs" % (D, inputs.shape[1]))
    obs = _em_broadcast(obs, E, M, "obs")
    if weights is not None:
        weights = _em_broadcast(weights, E, M, "weights")

    def block(a, e0, e1):           # a block of emulators in the shape the caller gave: (e,) or (e, M)
        if a is None:
            return None
        return a[e0:e1, 0] if a.shape[1] == 1 and M != 1 else a[e0:e1]

    def on_device(ctx, part, o, w):
        batch = _batch_model(ctx, part, inputs, precision, False)
        try:
            return batch.misfit(X, o, w, second_order, return_residual)
        finally:
            batch.close()

    if devices is None:
        o, w = block(obs, 0, E), block(weights, 0, E)
        if misfit_fn is not None:
            return tuple(misfit_fn(device, gps, X, o, w, second_order, return_residual))
        if not is_gpu:
            return _misfit_numpy(gps, np.asarray(X, dtype=np.float64), obs, weights, second_order, return_residual)
        return on_device(_lib.default_context(device), gps, o, w)
    from . import multi_gpu
    if len(devices) < 1:
        raise ValueError("devices must name at least one device")
    if not is_gpu and misfit_fn is None:
        raise ValueError("devices= shards the GPU path; the numpy branch runs in the calling thread")
    blocks = multi_gpu.row_shards(E, len(devices))       # contiguous blocks of emulators
    partial = [None] * len(devices)

    def work(k, dev, e0, e1):
        o, w = block(obs, e0, e1), block(weights, e0, e1)
        if misfit_fn is not None:
            partial[k] = tuple(misfit_fn(dev, gps[e0:e1], X, o, w, second_order, return_residual))
            return
        ctx, lock = multi_gpu._device_context(dev)
        with lock:
            partial[k] = on_device(ctx, gps[e0:e1], o, w)

    multi_gpu.run_shards(devices, blocks, work)
    parts = [p for p in partial if p is not None]          # device order
    n_sum = 3 if second_order else 2
    total = [np.array(a) for a in parts[0][:n_sum]]
    for p in parts[1:]:
        for acc, a in zip(total, p[:n_sum]):
            acc += a
    if return_residual:
        total.append(np.concatenate([p[n_sum] for p in parts], axis=0))
    return tuple(total)


def retrieve_bands(gps, X0, obs, weights=None, second_order="gauss_newton", prior=None, bounds=None, lam0=1e-2,
                   max_iter=20, down=1.0 / 3.0, up=4.0, ftol=1e-10, xtol=0.0, is_gpu=True, precision=np.float64,
                   device=None, step_fn=None, return_cov=False, next_prior=None, return_A=False):
    """Levenberg-Marquardt retrieval of M state vectors at once on E per-band emulators: minimises, row by row,

        F(x) = 1/2 sum_e w (mu_e(x) - obs[e])^2  (+ 1/2 (x - x0)^T P (x - x0) with ``prior=(x0 (D,), P (D, D))``)

    from ``X0`` (M, D), inside ``bounds=(lo (D,), hi (D,))`` when given.  ``obs`` and ``weights`` as in
    ``misfit_bands``; ``second_order`` is "gauss_newton" or "full" (the matrix A of the step).  An iteration is: the
    misfit at the trial rows, the accept / reject update (a trial that lowers F is taken and lambda multiplied by
    ``down``, any other is dropped and lambda multiplied by ``up``, between ``LAMBDA_MIN`` and ``LAMBDA_MAX``; a row
    whose accepted step gains no more than ``ftol * F`` or moves no more than ``xtol`` is converged and frozen), then
    the damped Newton step ``(A + P + lambda diag(A + P)) step = -(grad + P (x - x0))``, ``trial = clip(x + step)``.
    At most ``max_iter`` trials per row.

    Returns ``(X (M, D), cost (M,), state (M,) int32, n_accepted (M,) int32, lam (M,))``: ``cost`` is the DATA term
    at ``X`` (the prior term is not included), ``state`` 1 for converged rows, ``n_accepted`` the trials taken.

    On the GPU one ``BatchModel`` is built and ``X0``, ``obs`` and ``weights`` go up once; every iteration is
    ``misfit_device``, ``lm_update_device``, ``newton_step_device`` on the context's stream, and nothing comes back
    inside the loop but ``state``, every fourth iteration, to stop when every row has converged.  ``is_gpu=False`` is
    the explicit numpy branch, the same loop from ``_misfit_numpy`` and ``_lib.newton_step_numpy``; never a fallback.
    ``step_fn(x, grad, A, lam) -> (step, trial, status)`` replaces the Newton step in the CPU tests of the loop's
    logic: the loop then runs on the host whatever ``is_gpu`` says.

    ``return_cov=True`` appends ``cov (M, D, D)``, ``sigma (M, D)`` and ``cov_status (M,) int32`` to the five: the
    posterior covariance ``C = (A + P)^-1`` of every row, the square roots of its diagonal (the ``x +- sigma`` of the
    retrieval) and 0, or the 1-based index of the pivot at which ``A + P`` failed to factor, in which case the row's
    ``cov`` and ``sigma`` are NaN.  ``A`` is the matrix of the row's last accepted step (the one at the returned
    ``X``), WITHOUT the damping: the Gauss-Newton term by default; with ``second_order="full"`` the full
    second-order term, which may be indefinite away from a minimum -- ``cov_status`` then says so.  Active bounds are
    ignored: a component held at its bound gets the unconstrained variance.  ``C`` is a covariance only when
    ``weights`` are the inverse variances of the observations (and ``P`` that of the prior).  On the GPU this is one
    ``posterior_cov_device`` call on the loop's own device arrays after the loop, and only the three results come
    back; on the numpy branch ``_lib.posterior_cov_numpy`` on the loop's ``A``.  With ``False`` nothing changes.

    ``prior=(x0, P)`` is shared by the rows -- ``x0`` (D,), ``P`` (D, D) -- or per row -- ``x0`` (M, D), ``P`` (M, D, D) --
    each of the two independently: a prior map, or the propagated posterior of an earlier date.  On the GPU a per-row
    prior goes up once and the loop calls the ``_rows`` entries (the same kernels with a row stride); a shared prior
    makes exactly the calls it always made.

    ``next_prior=Q``, a process-noise covariance (D, D) or per row (M, D, D), appends ``next_prec (M, D, D)`` and
    ``prior_status (M,) int32`` behind everything else: ``next_prec = ((A + P)^-1 + Q)^-1``, the posterior precision
    relaxed by ``Q``, which with the returned state as its mean is the prior of the next date of a time series
    (random-walk dynamics).  ``prior_status`` is 0, k + 1 when pivot k of ``A + P`` fails, or D + k + 1 when pivot k of
    ``(A + P)^-1 + Q`` fails; then the row's ``next_prec`` is NaN.  On the GPU this is one ``prior_propagate_device`` call
    on the loop's own device arrays after the loop (the covariance in between never leaves the chip); on the numpy
    branch ``_lib.prior_propagate_numpy``.  With ``None`` nothing changes.

    ``return_A=True`` appends, as the last element, the loop's final data-term matrix ``A (M, D, D)``: the matrix whose
    ``(A + P)^-1`` is ``cov``, which the backward pass of a smoothed series reads (on the GPU one more download).  With
    ``False`` nothing changes."""
    if second_order not in ("gauss_newton", "full"):
        raise ValueError("second_order must be 'gauss_newton' or 'full'")
    X0 = np.asarray(X0)
    if X0.ndim != 2:
        raise ValueError("X0 must be (n_rows, n_inputs)")
    inputs = _check_shared_inputs(gps)
    E, (M, D) = len(gps), X0.shape
    if D != inputs.shape[1]:
        raise ValueError("X0 has %d columns, the emulators have %d inputs" % (D, inputs.shape[1]))
    obs = _em_broadcast(obs, E, M, "obs")
    if weights is not None:
        weights = _em_broadcast(weights, E, M, "weights")
    prior, bounds = _retrieve.prior_and_bounds(prior, bounds, D, M)
    max_iter = int(max_iter)

    if step_fn is not None or not is_gpu:
        step = step_fn if step_fn is not None else (
            lambda x, g, A, lam: _lib.newton_step_numpy(x, g, A, lam, "diagonal", prior, bounds))
        return _retrieve.lm_numpy(lambda X: _misfit_numpy(gps, X, obs, weights, second_order, False), step, X0, lam0,
                                  max_iter, down, up, ftol, xtol, prior, return_cov, next_prior, return_A)

    ctx = _lib.default_context(device)
    batch = _batch_model(ctx, gps, inputs, precision, False)

    def strides(a):
        return (1, 0) if a.shape[1] == 1 and M != 1 else (M, 1)
    try:
        with _retrieve.Scratch(ctx, np.dtype(precision)) as scratch:
            d_obs = scratch.up(obs)
            d_w = scratch.up(weights) if weights is not None else None
            os_, ws = strides(obs), strides(weights) if weights is not None else (0, 0)

            def misfit(d_rows, c, g, a):
                batch.misfit_device(d_rows, d_obs, os_, d_w, ws, c, g, M, d_gn=a if second_order == "gauss_newton" else None,
                                    d_hess=a if second_order == "full" else None)
            return _retrieve.lm_device(scratch, M, D, X0, lam0, prior, bounds, max_iter, down, up, ftol, xtol, return_cov,
                                       misfit, next_prior, return_A)
    finally:
        batch.close()


def retrieve_bands_series(gps, X0, obs, weights, prior, noise, smooth=False, **loop_args):
    """A time series of ``retrieve_bands`` on the emulators ``gps``: ``obs`` (T, E, M) -- or anything ``retrieve_bands``
    takes, per date -- and ``weights`` the same or None, one retrieval per date, the posterior of a date propagated by
    the process noise ``noise`` (D, D) or (M, D, D) into the prior of the next (``_retrieve.retrieve_series``: what it
    returns, and why ``prior`` is required).  ``loop_args`` are ``retrieve_bands``' other keywords.

    ``smooth=True`` appends the Rauch-Tung-Striebel smoothed trajectory ``X_s (T, M, D)``, ``sigma_s (T, M, D)`` and
    ``smooth_status (T, M)``: every date then also carries the observations after it (a gap is filled from both
    sides).  On the GPU the backward pass is one ``rts_smooth_device`` call per date with the smoothed state and
    covariance of the later date resident on the device; with ``is_gpu=False`` (or a ``step_fn``) it is
    ``_lib.rts_smooth_numpy``; never a fallback."""
    def retrieve(X, obs_t, weights_t, **kw):
        return retrieve_bands(gps, X, obs_t, weights_t, **kw)
    if not smooth:
        return _retrieve.retrieve_series(retrieve, X0, obs, weights, prior, noise, **loop_args)
    on_device = loop_args.get("is_gpu", True) and loop_args.get("step_fn") is None
    context = (lambda: _lib.default_context(loop_args.get("device"))) if on_device else None
    return _retrieve.retrieve_series(retrieve, X0, obs, weights, prior, noise, smooth=True, context=context, **loop_args)


# ---------------------------------------------------------------------------------------------
# Training many per-band emulators at once
# ---------------------------------------------------------------------------------------------
class _GatheredObjective(object):
    """Turns many concurrent single-theta evaluations into few batched ones.

    Each optimiser thread calls ``evaluate(slot, theta)`` and blocks.  When every thread that
    is still optimising has a request in, the thread that completed the set runs ONE batched
    evaluation for all of them (``batch_fn(thetas, targets) -> (cost, grad)``; on the GPU one
    launch of the likelihood kernels, one workgroup per request) and wakes the others.  No
    dispatcher thread, no polling; the scipy L-BFGS-B instances stay ordinary and independent.

    Synchronisation is deliberately primitive: one short critical section to register a request,
    and one private lock per thread to sleep on (released by whoever ran the batch).  A shared
    ``Condition`` + ``notify_all`` makes every woken thread queue for the same lock again and,
    with a few hundred threads, costs several times more than the evaluations themselves.
    """

    def __init__(self, batch_fn, n_slots, n_train, n_theta):
        import threading
        self._fn = batch_fn
        self._lock = threading.Lock()
        self._wake = [threading.Lock() for _ in range(n_slots)]
        for w in self._wake:
            w.acquire()                 # held: a waiter blocks until the batch runner releases it
        self._thetas = np.zeros((n_slots, n_theta))
        self._targets = np.zeros((n_slots, n_train))
        self._cost = np.zeros(n_slots)
        self._grad = np.zeros((n_slots, n_theta))
        self._waiting = []              # slots with a request in
        self._active = n_slots          # threads that may still submit requests
        self._error = None
        self.launches = 0
        self.evaluations = 0

    def set_targets(self, slot, targets):
        self._targets[slot] = targets

    def _run(self, batch, me):
        # every live thread is in `batch` and asleep (or is `me`): nothing else touches the state
        idx = np.array(batch)
        try:
            cost, grad = self._fn(self._thetas[idx], self._targets[idx])
            self._cost[idx] = cost
            self._grad[idx] = grad
        except BaseException as exc:    # wake everybody, re-raise in every thread
            self._error = exc
        self.launches += 1
        self.evaluations += len(batch)
        for s in batch:
            if s != me:
                self._wake[s].release()

    def evaluate(self, slot, theta):
        self._thetas[slot] = theta
        with self._lock:
            self._waiting.append(slot)
            batch = None
            if len(self._waiting) >= self._active:
                batch, self._waiting = self._waiting, []
        if batch is not None:
            self._run(batch, slot)
        else:
            self._wake[slot].acquire()
        if self._error is not None:
            raise self._error
        return float(self._cost[slot]), self._grad[slot].copy()

    def retire(self):
        """The calling thread will submit no more requests."""
        with self._lock:
            self._active -= 1
            batch = None
            if self._active > 0 and len(self._waiting) >= self._active:
                batch, self._waiting = self._waiting, []
        if batch is not None:
            self._run(batch, -1)


_driver_probe = []          # [setulb or None] once probed in this process


def _probe_setulb(setulb):
    """True when ``setulb`` behaves like the routine _Population is written for: called with that
    argument list on f(x) = (x0 - 1)^2 + (x1 + 2)^2 it asks for f, g with task 3, reports new
    iterations with task 1 and stops at the minimum within a few evaluations.  A private entry
    point has no compatibility promise: a scipy that renames an argument, changes a work-array size
    or the task codes fails here (an exception or a wrong answer), never inside a training run."""
    pop = _Population(setulb, [(0, 0)], np.array([[3.0, 4.0]]))
    results = None
    for _ in range(60):
        th, es, finished = pop.advance(results)
        if finished:
            e, k, cost, theta = finished[0]
            return bool(np.isfinite(cost) and cost < 1e-12 and np.allclose(theta, [1.0, -2.0], atol=1e-6))
        if th.shape != (1, 2):
            return False
        d = th - np.array([1.0, -2.0])
        results = (np.sum(d * d, axis=1), 2.0 * d)
    return False


def _lockstep_driver(warn=True):
    """scipy's reverse-communication L-BFGS-B entry point (``scipy.optimize._lbfgsb.setulb``, the
    routine ``fmin_l_bfgs_b`` itself loops over), or None -- with a warning, once -- when this scipy
    does not have it in the form written for here (1.15: C translation, integer task codes).  The
    binding is private, so it is PROBED, not trusted: version, then a run on a two-variable
    quadratic (``_probe_setulb``).  ``learn_bands(method="auto")`` then uses the threaded driver
    (one public ``fmin_l_bfgs_b`` per start, objective calls coalesced into batched launches)."""
    if _driver_probe:
        return _driver_probe[0]
    found, why = None, ""
    try:
        import scipy
        from scipy.optimize import _lbfgsb
        major, minor = (int(v) for v in scipy.__version__.split(".")[:2])
        if (major, minor) < (1, 15):
            why = "scipy %s predates the routine's C translation (1.15)" % scipy.__version__
        elif not _probe_setulb(_lbfgsb.setulb):
            why = "scipy %s: the routine did not minimise the probe problem with the 1.15 argument list" % scipy.__version__
        else:
            found = _lbfgsb.setulb
    except Exception as exc:
        why = "%s: %s" % (type(exc).__name__, exc)
    _driver_probe.append(found)
    if found is None and warn:
        import warnings
        warnings.warn("gp_emulator_amd.perband: scipy.optimize._lbfgsb.setulb is not usable (%s); training falls back "
                      "to the threaded L-BFGS-B driver (same results, more launches)" % why, RuntimeWarning, stacklevel=2)
    return found


class _Instance(object):
    """One L-BFGS-B minimisation in reverse communication: the state ``fmin_l_bfgs_b`` keeps in
    local variables (scipy/optimize/_lbfgsb_py.py, ``_minimize_lbfgsb``), same sizes and defaults
    (m = 10, maxls = 20, maxfun = maxiter = 15000, no bounds)."""
    __slots__ = ("e", "k", "x", "f", "g", "wa", "iwa", "task", "ln_task", "lsave", "isave", "dsave",
                 "nit", "nfev", "low", "up", "nbd", "last_good", "failed")

    def __init__(self, e, k, x0):
        n, m = x0.size, 10
        self.e, self.k = e, k
        self.x = np.array(x0, dtype=np.float64)
        self.f = 0.0
        self.g = np.zeros(n)
        self.wa = np.zeros(2 * m * n + 5 * n + 11 * m * m + 8 * m)
        self.iwa = np.zeros(3 * n, dtype=np.int32)
        self.task = np.zeros(2, dtype=np.int32)
        self.ln_task = np.zeros(2, dtype=np.int32)
        self.lsave = np.zeros(4, dtype=np.int32)
        self.isave = np.zeros(44, dtype=np.int32)
        self.dsave = np.zeros(29)
        self.low, self.up = np.zeros(n), np.zeros(n)
        self.nbd = np.zeros(n, dtype=np.int32)
        self.nit = self.nfev = 0
        self.last_good = self.x.copy()
        self.failed = False


class _Population(object):
    """A set of L-BFGS-B instances advanced in lockstep: ``advance(results)`` hands the instances
    that asked last time their costs and gradients, steps every live instance through scipy's
    routine until it asks for a cost/gradient or stops, and returns the new requests and the
    instances that finished.  Lives in the calling process or in a worker process (``_worker``)."""

    factr, pgtol, m, maxls, maxfun, maxiter = 0.1, 1e-20, 10, 20, 15000, 15000

    def __init__(self, setulb, ids, starts):
        self.setulb = setulb
        self.n = int(np.asarray(starts).shape[1])
        self.live = [_Instance(e, k, x0) for (e, k), x0 in zip(ids, starts)]
        self.asking = []

    def advance(self, results):
        """results: (cost (A,), grad (A, n)) for the A requests returned by the previous call
        (None the first time).  Returns (thetas (A', n), e (A',), finished) where finished is a
        list of (e, k, cost, theta)."""
        finished = []
        if results is not None:
            c, g = results
            keep = []
            for j, it in enumerate(self.asking):
                it.nfev += 1
                if not np.isfinite(c[j]):
                    # a pivot <= 0: the reference's numpy path raises LinAlgError here and its
                    # optimiser loop gives the restart up with cost 9999 (:176-181)
                    finished.append((it.e, it.k, 9999.0, it.last_good))
                else:
                    it.f = float(c[j])
                    it.g[:] = g[j]
                    it.last_good[:] = it.x
                    keep.append(it)
            self.live = keep
        setulb, m, factr, pgtol, maxls = self.setulb, self.m, self.factr, self.pgtol, self.maxls
        asking = []
        for it in self.live:
            while True:
                setulb(m, it.x, it.low, it.up, it.nbd, it.f, it.g, factr, pgtol, it.wa, it.iwa,
                       it.task, it.lsave, it.isave, it.dsave, maxls, it.ln_task)
                task = it.task[0]
                if task == 3:                            # wants f and g at x
                    if it.nfev and it.x.tobytes() == it.last_good.tobytes():
                        continue                         # same point again: f, g are current
                    asking.append(it)                    # (what scipy's ScalarFunction cache does)
                    break
                if task == 1:                            # new iteration
                    it.nit += 1
                    if it.nit >= self.maxiter:
                        it.task[0], it.task[1] = 5, 504
                    elif it.nfev > self.maxfun:
                        it.task[0], it.task[1] = 5, 502
                    continue
                finished.append((it.e, it.k, it.f, it.x.copy()))   # converged / stopped
                break
        self.asking = self.live = asking
        th = np.stack([it.x for it in asking]) if asking else np.zeros((0, self.n))
        es = np.array([it.e for it in asking], dtype=np.int64)
        return th, es, finished


def _worker_main():
    """Body of a lockstep worker process (``python -c "from gp_emulator_amd.perband import
    _worker_main; _worker_main()"``): a _Population driven over its stdin / stdout with pickled
    messages.  It never touches the GPU -- the objective is evaluated by the parent, for all
    workers' requests at once.  A plain child process rather than ``multiprocessing``: a spawned
    multiprocessing child re-imports the caller's main script, which a library must not require
    to be import-safe."""
    import os
    import pickle
    import sys
    inp, out = sys.stdin.buffer, os.fdopen(os.dup(sys.stdout.fileno()), "wb")
    sys.stdout = sys.stderr                       # nothing but messages on the pipe
    try:
        ids, starts = pickle.load(inp)
        pop = _Population(_lockstep_driver(), ids, starts)
        results = None
        while True:
            pickle.dump(pop.advance(results), out, protocol=4)
            out.flush()
            results = pickle.load(inp)
            if results is None:
                return
    except EOFError:
        return
    except BaseException as exc:                  # report, the parent raises
        try:
            pickle.dump(RuntimeError("%s: %s" % (type(exc).__name__, exc)), out, protocol=4)
            out.flush()
        except Exception:
            pass


def _lockstep_processes(n_instances, processes):
    """How many worker processes step the optimisers.  scipy's routine holds the GIL and costs
    ~10 us of host time per evaluation -- 2e6 evaluations for 2101 bands x 5 restarts -- while the
    GPU needs 1.5 us for the same evaluation, so large jobs spread the stepping over processes;
    small ones are not worth the workers' start-up (an interpreter + numpy + scipy each)."""
    if processes is not None:
        return max(0, int(processes))
    if n_instances < 2048:
        return 0
    import os
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return max(0, min(8, avail - 1, n_instances // 512))


def _learn_lockstep(setulb, batch_fn, targets, starts, max_batch=4096, processes=0):
    """Every (emulator, restart) optimisation advances through scipy's own L-BFGS-B routine, no
    callbacks: each instance is stepped until it asks for a cost/gradient, then ALL the requests
    are evaluated in one batched call.  Iterates are those of ``fmin_l_bfgs_b(factr=0.1,
    pgtol=1e-20)`` (reference GaussianProcess.py:168-170) because it is the same routine fed the
    same numbers.  ``processes`` > 0: the instances are dealt to that many worker processes
    (child interpreters that import numpy and scipy and never touch the GPU); the parent only
    gathers their requests, runs the batched objective and scatters the answers."""
    E, n_tries, n = starts.shape
    ids = [(e, k) for e in range(E) for k in range(n_tries)]
    flat = starts.reshape(E * n_tries, n)
    cost = np.full((E, n_tries), np.inf)
    theta = np.zeros((E, n_tries, n))
    launches = evaluations = 0

    def evaluate(th, es):
        nonlocal launches, evaluations
        c = np.empty(len(th))
        g = np.empty((len(th), n))
        for s0 in range(0, len(th), max_batch):
            c[s0:s0 + max_batch], g[s0:s0 + max_batch] = batch_fn(th[s0:s0 + max_batch], targets[es[s0:s0 + max_batch]])
            launches += 1
        evaluations += len(th)
        return c, g

    def record(finished):
        for e, k, f, x in finished:
            cost[e, k], theta[e, k] = f, x

    if processes <= 0:
        pop = _Population(setulb, ids, flat)
        results = None
        while True:
            th, es, finished = pop.advance(results)
            record(finished)
            if not len(th):
                break
            results = evaluate(th, es)
        return cost, theta, launches, evaluations

    import os
    import pickle
    import subprocess
    import sys
    # the workers' BLAS must be single-threaded: the routine makes tiny LAPACK calls, and several
    # processes each spinning a thread team per call are hundreds of times slower than one thread
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "BLIS_NUM_THREADS"):
        env[k] = "1"
    pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = pkg_parent + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    code = "from gp_emulator_amd.perband import _worker_main; _worker_main()"
    workers = []

    def send(proc, msg):
        pickle.dump(msg, proc.stdin, protocol=4)
        proc.stdin.flush()

    try:
        for w in range(processes):
            mine = list(range(w, len(ids), processes))          # dealt round-robin: even load
            proc = subprocess.Popen([sys.executable, "-c", code], stdin=subprocess.PIPE,
                                    stdout=subprocess.PIPE, env=env)
            workers.append(proc)
            send(proc, ([ids[i] for i in mine], flat[mine]))
        # two groups of workers take turns: while the objective of one group's requests runs on
        # the GPU (the GIL is released in the call), the other group's optimisers are stepping
        groups = [list(range(0, processes, 2)), list(range(1, processes, 2))]
        while groups[0] or groups[1]:
            for gi in (0, 1):
                if not groups[gi]:
                    continue
                asked = []
                for w in groups[gi]:
                    try:
                        msg = pickle.load(workers[w].stdout)
                    except EOFError:
                        raise RuntimeError("lockstep worker %d exited (status %s)" % (w, workers[w].poll()))
                    if isinstance(msg, BaseException):
                        raise RuntimeError("lockstep worker %d failed: %s" % (w, msg))
                    th, es, finished = msg
                    record(finished)
                    asked.append((w, th, es))
                th_all = np.concatenate([th for _, th, _ in asked])
                es_all = np.concatenate([es for _, _, es in asked])
                c, g = evaluate(th_all, es_all) if len(th_all) else (np.zeros(0), np.zeros((0, n)))
                s0, still = 0, []
                for w, th, _ in asked:
                    k = len(th)
                    if k:
                        send(workers[w], (c[s0:s0 + k], g[s0:s0 + k]))
                        still.append(w)
                    else:
                        send(workers[w], None)              # nothing left in that worker
                    s0 += k
                groups[gi] = still
        for proc in workers:
            proc.wait(10)
    finally:
        for proc in workers:                            # the exact children started above
            for fh in (proc.stdin, proc.stdout):
                try:
                    fh.close()
                except Exception:
                    pass
            if proc.poll() is None:
                proc.terminate()
                try:
                    proc.wait(5)
                except Exception:
                    proc.kill()
    return cost, theta, launches, evaluations


def _leave_set(gps, thetas, inputs, ctx):
    """Leave every emulator set to its optimum (theta, invQ, invQt), as the reference's
    learn_hyperparameters does (:207-209); on the GPU a few launches of 128 inverses each."""
    if ctx is None:
        for e, gp in enumerate(gps):
            gp._set_params(thetas[e].copy())
        return
    step = 128
    for s in range(0, len(gps), step):
        part = gps[s:s + step]
        tg = np.stack([np.asarray(gp.targets, dtype=np.float64) for gp in part])
        c, g, invQ, invQt = ctx.likelihood_batch(thetas[s:s + len(part)], inputs, tg, want_inverse=True)
        for i, gp in enumerate(part):
            if not np.isfinite(c[i]):     # every restart failed: the reference's final
                raise np.linalg.LinAlgError("Matrix is not positive definite")   # loglikelihood raises too
            gp.theta = thetas[s + i].copy()
            gp.invQ, gp.invQt = invQ[i].copy(), invQt[i].copy()
            gp.current_theta, gp.current_loglikelihood = gp.theta, float(c[i])
            gp._gpu_models = {}


def _finite(cost_grad):
    """A non-finite cost means a pivot of the elimination was <= 0 -- what the reference's numpy
    path reports as LinAlgError (GaussianProcess.py:66) and its optimiser loop catches (:176-181)."""
    if not np.isfinite(cost_grad[0]):
        raise np.linalg.LinAlgError("Matrix is not positive definite")
    return cost_grad


def learn_bands(gps, n_tries=5, concurrency=256, is_gpu=True, starts=None, batch_fn=None,
                device=None, verbose=False, method="auto", processes=None):
    """``learn_hyperparameters(n_tries)`` for every GaussianProcess in ``gps`` (per-band
    emulators on the SAME training inputs, tests/test_perband_emulator.py:22-37), with the
    optimisations of all bands and all restarts advancing side by side: ``concurrency``
    scipy L-BFGS-B instances run in threads and their cost/gradient requests are gathered
    into batched launches of the likelihood kernels (one workgroup per request).

    Starting points are drawn exactly as a loop of ``gp.learn_hyperparameters(n_tries)`` calls
    would draw them (``5 (rand(n_tries, D+2) - 0.5)`` per emulator, in order, from
    ``numpy.random``), unless ``starts`` (E, n_tries, D+2) is given.  On return every emulator
    is set to its best theta (``theta``, ``invQ``, ``invQt``), as the reference leaves it
    (GaussianProcess.py:183-209).  Returns ``(costs (E,), thetas (E, D+2), stats)``.

    ``batch_fn(thetas, targets) -> (cost, grad)`` replaces the GPU objective (tests use a numpy
    one); ``is_gpu`` must be true otherwise -- there is no silent CPU path.

    ``method``: "lockstep" steps scipy's reverse-communication L-BFGS-B routine directly for every
    (emulator, restart) from one thread and evaluates all pending requests per round in one
    launch -- the same iterates as ``fmin_l_bfgs_b`` at a fraction of its per-call Python cost;
    "threads" runs ``concurrency`` ordinary ``fmin_l_bfgs_b`` calls in threads and gathers their
    requests; "auto" takes lockstep when this scipy exposes the routine with the known signature.
    """
    import threading
    import warnings
    from queue import Queue, Empty
    from scipy.optimize import fmin_l_bfgs_b
    inputs = np.ascontiguousarray(_check_shared_inputs(gps), dtype=np.float64)
    E, (N, D) = len(gps), inputs.shape
    ctx = None
    if batch_fn is None:
        if not is_gpu:
            raise ValueError("learn_bands runs the objective on the GPU; pass is_gpu=True")
        ctx = _lib.default_context(device)

        def batch_fn(thetas, targets):
            return ctx.likelihood_batch(thetas, inputs, targets)
    if starts is None:
        starts = np.stack([5. * (np.random.rand(n_tries, D + 2) - 0.5) for _ in range(E)])
    starts = np.asarray(starts, dtype=np.float64).reshape(E, -1, D + 2)
    n_tries = starts.shape[1]
    setulb = _lockstep_driver() if method in ("auto", "lockstep") else None
    if method == "lockstep" and setulb is None:
        raise RuntimeError("this scipy does not expose the L-BFGS-B routine learn_bands knows how to drive")
    if method not in ("auto", "lockstep", "threads"):
        raise ValueError("method must be 'auto', 'lockstep' or 'threads'")
    if setulb is not None:
        tg_all = np.stack([np.asarray(gp.targets, dtype=np.float64) for gp in gps])
        n_proc = _lockstep_processes(E * n_tries, processes)
        best_cost, best_theta, launches, evaluations = _learn_lockstep(setulb, batch_fn, tg_all, starts,
                                                                       processes=n_proc)
        pick = np.argmin(best_cost, axis=1)
        costs = best_cost[np.arange(E), pick]
        thetas = best_theta[np.arange(E), pick]
        _leave_set(gps, thetas, inputs, ctx)
        stats = {"launches": launches, "evaluations": evaluations, "threads": 1, "method": "lockstep",
                 "processes": n_proc}
        if verbose:
            print("learn_bands: %d emulators x %d starts, %d evaluations in %d launches" % (
                E, n_tries, evaluations, launches))
        return costs, thetas, stats
    jobs = Queue()
    for e in range(E):
        for k in range(n_tries):
            jobs.put((e, k))
    n_threads = int(max(1, min(concurrency, E * n_tries)))
    gather = _GatheredObjective(batch_fn, n_threads, N, D + 2)
    best_cost = np.full((E, n_tries), np.inf)
    best_theta = np.zeros((E, n_tries, D + 2))
    failures = []

    def worker(slot):
        try:
            while True:
                try:
                    e, k = jobs.get_nowait()
                except Empty:
                    return
                gather.set_targets(slot, np.asarray(gps[e].targets, dtype=np.float64))
                try:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        th, f, _ = fmin_l_bfgs_b(lambda t: _finite(gather.evaluate(slot, t)),
                                                 starts[e, k], factr=0.1, pgtol=1e-20, iprint=-1)
                    best_cost[e, k], best_theta[e, k] = f, th
                except np.linalg.LinAlgError:      # reference :176-181: keep going, cost 9999
                    best_cost[e, k], best_theta[e, k] = 9999.0, starts[e, k]
        except BaseException as exc:
            failures.append(exc)
        finally:
            gather.retire()

    threads = [threading.Thread(target=worker, args=(s,), daemon=True) for s in range(n_threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if failures:
        raise failures[0]
    pick = np.argmin(best_cost, axis=1)
    costs = best_cost[np.arange(E), pick]
    thetas = best_theta[np.arange(E), pick]
    _leave_set(gps, thetas, inputs, ctx)
    stats = {"launches": gather.launches, "evaluations": gather.evaluations, "threads": n_threads,
             "method": "threads"}
    if verbose:
        print("learn_bands: %d emulators x %d starts, %d evaluations in %d launches" % (
            E, n_tries, gather.evaluations, gather.launches))
    return costs, thetas, stats
