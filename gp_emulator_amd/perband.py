"""Per-band emulators predicted together.

The reference's per-band pattern (tests/test_perband_emulator.py:22-37) builds one
``GaussianProcess`` per spectral band on the SAME training inputs ``y_train`` -- each with
its own targets, theta, invQ, invQt -- and then calls ``gp.predict(X, is_gpu=True)`` band by
band (:48-50).  ``predict_bands`` runs all of them over the shared test rows in one launch
of the fused kernel (BASELINE config 3: 2101 bands x N_train=250 x D=11, shared test set).
"""
import numpy as np

from . import _first_guess, _lib, _moments_numpy, _retrieve, _sobol_numpy, multi_gpu
from ._retrieve import LAMBDA_MAX, LAMBDA_MIN, _lm_update_numpy, _prior_term     # noqa: F401  (their names here)
from .perband_train import (learn_bands, _driver_probe, _lockstep_driver, _lockstep_processes,     # noqa: F401  (training
                            _Population, _probe_setulb, _worker_main)                              # many bands at once)


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


def _rows_and_inputs(gps, rows, name, n_name="n_rows"):
    """``rows`` as an array and the emulators' shared training inputs; the rows are 2-D and have the inputs' column
    count, or the ``ValueError`` names the argument."""
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError("%s must be (%s, n_inputs)" % (name, n_name))
    inputs = _check_shared_inputs(gps)
    if rows.shape[1] != inputs.shape[1]:
        raise ValueError("%s has %d columns, the emulators have %d inputs" % (name, rows.shape[1], inputs.shape[1]))
    return rows, inputs


def _host_dtype(rows, precision):
    """The dtype of a sharded call's gathered results: float64 when the rows or the device precision are, else float32."""
    return np.float64 if (rows.dtype == np.float64 or np.dtype(precision) == np.float64) else np.float32


def _on_shards(gps, devices, inputs, precision, do_unc, call, hook=None):
    """The per-device scaffold of the ``devices=`` paths: the emulators are cut into contiguous blocks, one per device
    and one thread each (``multi_gpu.run_shards``: empty blocks are skipped, the first exception is raised in the
    caller).  A block's thread runs ``call(batch, e0, e1)`` on the block's ``BatchModel``, built on the device's
    long-lived context under its lock and closed afterwards -- or, in the CPU tests of the sharding logic,
    ``hook(device, e0, e1)`` instead.  Returns what the blocks returned, in device order (None for a skipped one)."""
    results = [None] * len(devices)

    def work(k, dev, e0, e1):
        if hook is not None:
            results[k] = hook(dev, e0, e1)
            return
        ctx, lock = multi_gpu._device_context(dev)
        with lock, _batch_model(ctx, gps[e0:e1], inputs, precision, do_unc) as batch:
            results[k] = call(batch, e0, e1)

    multi_gpu.run_shards(devices, multi_gpu.row_shards(len(gps), len(devices)), work)
    return results


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
        with make_batch(gps, precision, device, do_unc=do_unc) as batch:
            return batch.predict(testing) if do_unc else batch.predict_mean_grad(testing)
    if not gps:
        raise ValueError("need at least one GaussianProcess")
    E, (M, D) = len(gps), testing.shape
    dt = _host_dtype(testing, precision)
    mu, deriv = np.empty((E, M), dt), np.empty((E, M, D), dt)
    var = np.empty((E, M), dt) if do_unc else None
    outs = (mu, var, deriv) if do_unc else (mu, deriv)

    def hook(dev, e0, e1):
        if do_unc:
            mu[e0:e1], var[e0:e1], deriv[e0:e1] = predict_fn(dev, gps[e0:e1], testing)
        else:
            mu[e0:e1], deriv[e0:e1] = predict_fn(dev, gps[e0:e1], testing)

    def on_device(batch, e0, e1):      # every device's slab pipeline writes its own slice
        views = tuple(a[e0:e1] for a in outs)
        batch.predict(testing, out=views) if do_unc else batch.predict_mean_grad(testing, out=views)

    _on_shards(gps, devices, _check_shared_inputs(gps), precision, do_unc, on_device, hook if predict_fn else None)
    return outs


def variance_gradient_bands(gps, X, precision=np.float64, device=None):
    """var (E, M) and dvar (E, M, D): the predictive variance of the E emulators in ``gps`` at the shared rows ``X``
    (M, D) and its gradient with respect to the row, in one launch per 2^20 rows (``BatchModel.predict_var_grad``).
    Arrays of ``precision``; emulator e bit for bit what ``Model.predict_var_grad`` of it gives."""
    with make_batch(gps, precision, device) as batch:
        return batch.predict_var_grad(np.asarray(X))


def _sobol_constants(gps):
    """expX (E, D + 2), the shared inputs and invQt (E, N) of the emulators, float64."""
    inputs = np.asarray(_check_shared_inputs(gps), dtype=np.float64)
    return (np.stack([np.exp(np.asarray(gp.theta, dtype=np.float64)) for gp in gps]), inputs,
            np.stack([np.asarray(gp.invQt, dtype=np.float64).reshape(inputs.shape[0]) for gp in gps]))


def sobol_pairs(expX, inputs, invQt, bounds, pairs=None, is_gpu=True, device=None):
    """``(mean, cov)`` of ``Context.sobol_batch`` on the default context of ``device``, or with ``is_gpu=False`` of its
    numpy branch ``_sobol_numpy.sobol_pairs_numpy``."""
    if is_gpu:
        return _lib.default_context(device).sobol_batch(expX, inputs, invQt, bounds[0], bounds[1], pairs)
    return _sobol_numpy.sobol_pairs_numpy(expX, inputs, invQt, bounds[0], bounds[1], pairs)


def sobol_bands(gps, bounds, is_gpu=True, device=None):
    """Sobol sensitivity indices of the E emulators in ``gps`` (shared training inputs) for independent uniform inputs
    on ``bounds = (lo, hi)``, each (D,) or (n_boxes, D): ``SobolIndices(first (E, D), total (E, D), variance (E,),
    mean (E,))`` -- which inputs drive which band, over which prior range -- with a leading ``n_boxes`` axis for 2-D
    bounds.  One call of ``gp_sobol_batch_f64`` (float64 only) for all bands and boxes; ``is_gpu=False`` is the numpy
    branch.  See ``GaussianProcess.sobol_indices``."""
    mean, cov = sobol_pairs(*_sobol_constants(gps), bounds, is_gpu=is_gpu, device=device)
    first, total, variance = _sobol_numpy.indices(cov)
    return _sobol_numpy.SobolIndices(first, total, variance, mean)


def sobol_interaction_pairs(expX, inputs, invQt, bounds, pairs=None, is_gpu=True, device=None):
    """``inter`` of ``Context.sobol_interactions`` on the default context of ``device``, or with ``is_gpu=False`` of its
    numpy branch ``_sobol_numpy.interactions_numpy``."""
    if is_gpu:
        return _lib.default_context(device).sobol_interactions(expX, inputs, invQt, bounds[0], bounds[1], pairs)
    return _sobol_numpy.interactions_numpy(expX, inputs, invQt, bounds[0], bounds[1], pairs)


def sobol_interactions_bands(gps, bounds, is_gpu=True, device=None):
    """Second-order Sobol indices of the E emulators in ``gps`` (shared training inputs) on ``bounds = (lo, hi)``, each
    (D,) or (n_boxes, D): ``SobolInteractions(second (E, D, D), higher (E,), first, total, variance, mean)``.
    ``second`` is symmetric with ``S_ik = V2^{ik} / V`` off the diagonal -- which input ``i`` interacts with when
    ``total[i] - first[i]`` is large -- and ``first`` on it; ``higher = 1 - sum_{i <= k} second`` is the share of the
    interactions of order three and more; NaN where ``V <= 0``.  The last four fields are ``sobol_bands``'s, from one
    ``gp_sobol_batch_f64`` call; the interaction covariances from one ``gp_sobol_interactions_f64`` call (float64 only).
    ``is_gpu=False`` is the numpy branch.  A leading ``n_boxes`` axis for 2-D bounds."""
    consts = _sobol_constants(gps)
    mean, cov = sobol_pairs(*consts, bounds, is_gpu=is_gpu, device=device)
    inter = sobol_interaction_pairs(*consts, bounds, is_gpu=is_gpu, device=device)
    first, total, variance = _sobol_numpy.indices(cov)
    second, higher = _sobol_numpy.second_order(cov, inter)
    return _sobol_numpy.SobolInteractions(second, higher, first, total, variance, mean)


def main_effects_bands(gps, bounds, grid=None, n_grid=33, is_gpu=True, device=None):
    """Main-effect curves of the E emulators in ``gps`` on ``bounds = (lo, hi)``, each (D,) or (n_boxes, D):
    ``MainEffects(grid (D, G), effect (E, D, G), mean (E,))`` with ``effect[e, d, g] = E[mu_e | t_d = grid[d, g]] - mean[e]``
    -- the picture next to the indices; its mean over ``t_d`` is 0 and its mean square ``first[d] * variance``.
    ``grid`` is (D, G) or (n_boxes, D, G) of points of input d (outside the box is allowed); ``None`` means ``n_grid``
    equally spaced points from ``lo`` to ``hi`` inclusive.  One ``gp_sobol_main_effects_f64`` call (float64 only; the
    means from ``gp_sobol_batch_f64``); ``is_gpu=False`` is the numpy branch.  A leading ``n_boxes`` axis for 2-D bounds."""
    expX, inputs, invQt = _sobol_constants(gps)
    lo, hi, boxed = _sobol_numpy.bounds_arrays(bounds[0], bounds[1], inputs.shape[1])
    grid = _sobol_numpy.grid_array(grid, lo, hi, n_grid)
    if is_gpu:
        ctx = _lib.default_context(device)
        effect = ctx.sobol_main_effects(expX, inputs, invQt, lo, hi, grid)
        mean, _ = ctx.sobol_batch(expX, inputs, invQt, lo, hi)
    else:
        effect = _sobol_numpy.main_effects_numpy(expX, inputs, invQt, lo, hi, grid)
        mean = _sobol_numpy.means_numpy(expX, inputs, invQt, lo, hi)
    if not boxed:
        grid, effect, mean = grid[0], effect[0], mean[0]
    return _sobol_numpy.MainEffects(grid, effect, mean)


def _moments_constants(gps):
    """``_sobol_constants`` and invQ (E, N, N) -- None when an emulator has none."""
    expX, inputs, invQt = _sobol_constants(gps)
    N = inputs.shape[0]
    if any(getattr(gp, "invQ", None) is None for gp in gps):
        return expX, inputs, invQt, None
    return expX, inputs, invQt, np.stack([np.asarray(gp.invQ, dtype=np.float64).reshape(N, N) for gp in gps])


def moments_pairs(expX, inputs, invQt, invQ, X, cov, pairs=None, is_gpu=True, device=None):
    """``(mean, egrad, cov, evar, info)`` of ``Context.moments_batch`` on the default context of ``device``, or with
    ``is_gpu=False`` of its numpy branch ``_moments_numpy.moments_pairs_numpy``."""
    if is_gpu:
        return _lib.default_context(device).moments_batch(expX, inputs, invQt, invQ, X, cov, pairs)
    return _moments_numpy.moments_pairs_numpy(expX, inputs, invQt, invQ, X, cov, pairs)


def predict_uncertain_bands(gps, X, cov, is_gpu=True, device=None):
    """The E emulators in ``gps`` (shared training inputs) under Gaussian inputs ``x_m ~ N(X[m], cov[m])`` -- ``X``
    (M, D), ``cov`` (D, D) or (M, D, D), positive semi-definite, only the lower triangles read -- in closed form:
    ``UncertainPrediction(mean (E, M), var_state (E, M), var_emulator (E, M), expected_grad (E, M, D), info (M,))``.
    ``mean = E[mu_e(x)]``, ``var_state = Var[mu_e(x)]`` (the state's share of a band's uncertainty), ``var_emulator =
    E[v_e(x)]`` (the emulator's; NaN when an emulator has no ``invQ``), their sum the total predictive variance, and
    ``expected_grad = E[d mu_e / dx]``, so that ``Cov[x, mu_e] = cov @ expected_grad``.  ``info`` is nonzero, and the
    row NaN, where ``cov[m]`` is not positive semi-definite (k + 1: pivot k) or the row is not finite (-1).  One call
    of ``gp_moments_batch_f64`` (float64 only) for all bands and rows; ``is_gpu=False`` is the numpy branch::

        x, *_, cov, sigma, status = retrieve_bands(gps, X0, obs, return_cov=True)
        other = predict_uncertain_bands(other_sensor_gps, x, cov)      # what the state implies for another sensor

    See ``GaussianProcess.predict_uncertain``."""
    mean, egrad, V, evar, info = moments_pairs(*_moments_constants(gps), X, cov, is_gpu=is_gpu, device=device)
    evar = np.full(mean.shape, np.nan) if evar is None else evar
    return _moments_numpy.UncertainPrediction(mean.T.copy(), V.T.copy(), evar.T.copy(), egrad.transpose(1, 0, 2).copy(), info)


def hessian_bands(gps, testing, precision=np.float64, weights=None, device=None, devices=None, hessian_fn=None):
    """Hessians of the E emulators' means over shared test rows: ``(E, M, D, D)``, or with ``weights``
    ``(E, M)`` the weighted sum over the emulators ``sum_e weights[e, m] * H_e[m]``, ``(M, D, D)`` -- the
    second-derivative term of a spectral cost function, summed on the device (the per-band result of 2101
    bands x 1e5 rows could never be stored).  One batched launch per slab of rows (the batch's ``hessian`` /
    ``hessian_weighted``); no inverse is stacked or uploaded.

    ``devices`` shards the EMULATORS like ``predict_bands``: device g takes a contiguous block.  Unweighted,
    every device writes its own ``[e0:e1]`` slice; weighted, every device returns the partial sum of its block
    and the partial sums are added on the host in device order (so the result does not depend on which device
    finishes first).  ``hessian_fn(device, gps_block, testing[, weights_block])`` replaces the HIP path in the
    CPU tests of the sharding logic."""
    testing, inputs = _rows_and_inputs(gps, testing, "testing", "n_predict")
    E, (M, D) = len(gps), testing.shape
    if weights is not None:
        weights = np.asarray(weights)
        if weights.shape != (E, M):
            raise ValueError("weights must be (%d, %d), got %s" % (E, M, weights.shape))
    if devices is None:
        if hessian_fn is not None:
            return hessian_fn(device, gps, testing) if weights is None else hessian_fn(device, gps, testing, weights)
        with make_batch(gps, precision, device, do_unc=False) as batch:
            return batch.hessian(testing) if weights is None else batch.hessian_weighted(testing, weights)
    if len(devices) < 1:
        raise ValueError("devices must name at least one device")
    dt = _host_dtype(testing, precision)
    out = np.empty((E, M, D, D), dt) if weights is None else None

    def hook(dev, e0, e1):
        if weights is None:
            out[e0:e1] = hessian_fn(dev, gps[e0:e1], testing)
        else:
            return np.asarray(hessian_fn(dev, gps[e0:e1], testing, weights[e0:e1]))

    def on_device(batch, e0, e1):
        if weights is None:
            batch.hessian(testing, out=out[e0:e1])
        else:
            return np.array(batch.hessian_weighted(testing, weights[e0:e1]))   # (own memory, not the pool's)

    partial = _on_shards(gps, devices, inputs, precision, False, on_device, hook if hessian_fn else None)
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


def _misfit_unc_numpy(gps, X, obs, weights, second_order, return_residual):
    """The data term with the emulators' variance (``misfit_bands(emulator_unc=True)``: the formulas) in float64, emulator
    after emulator, from ``cpu_predict(do_unc=True)`` and ``variance_gradient(is_gpu=False)``."""
    E, (M, D) = len(gps), X.shape
    cost, grad = np.zeros(M), np.zeros((M, D))
    gn = np.zeros((M, D, D)) if second_order else None
    wr, weffs = (np.empty((E, M)), np.empty((E, M))) if return_residual else (None, None)
    with np.errstate(invalid="ignore", over="ignore"):
        for e, gp in enumerate(gps):
            mu, v, deriv = gp.cpu_predict(X, do_unc=True)
            dv = gp.variance_gradient(X, is_gpu=False)[1]
            w = np.broadcast_to(weights[e], (M,)) if weights is not None else np.ones(M)
            r = mu - np.broadcast_to(obs[e], (M,))
            clamp = v <= 0                                  # (False for a NaN v: it goes through every formula)
            vp = np.where(clamp, 0.0, v)
            dvp = np.where(clamp[:, None], 0.0, dv)
            weff = w / (1.0 + w * vp)
            a = weff * r
            c = np.where(clamp, 0.0, 0.5 * weff * (1.0 - a * r))
            q = np.where(clamp, 0.0, 0.5 * weff * weff)
            cost += a * r + np.log1p(w * vp)
            grad += a[:, None] * deriv + c[:, None] * dvp
            if second_order:
                gn += weff[:, None, None] * (deriv[:, :, None] * deriv[:, None, :])      # (exactly symmetric)
                gn += q[:, None, None] * (dvp[:, :, None] * dvp[:, None, :])
            if return_residual:
                wr[e], weffs[e] = a, weff
    out = (0.5 * cost, grad)
    if second_order:
        out += (gn,)
    if return_residual:
        out += (wr, weffs)
    return out


def _check_unc_order(second_order):
    if second_order == "full":
        raise ValueError("second_order='full' needs the Hessian of the variance: not available with emulator_unc=True")


def misfit_bands(gps, X, obs, weights=None, second_order=None, return_residual=False, is_gpu=True,
                 precision=np.float64, device=None, devices=None, misfit_fn=None, emulator_unc=False):
    """Data term of a variational retrieval on E per-band emulators over shared rows ``X`` (M, D):

        r[e, m] = mu_e(x_m) - obs[e, m]            w = 1 without ``weights``
        cost[m] = 1/2 sum_e w r^2                  grad[m] = sum_e w r dmu_e/dx
        gn[m]   = sum_e w dmu_e/dx dmu_e/dx^T      hess[m] = gn[m] + sum_e w r H_e[m]

    Returns ``cost (M,), grad (M, D)``, then ``gn`` (``second_order="gauss_newton"``) or ``hess`` (``"full"``)
    ``(M, D, D)``, then with ``return_residual`` ``wr = w r (E, M)`` -- the ``weights`` of ``hessian_bands``.
    ``obs`` and ``weights`` are ``(E,)`` (one spectrum for all rows) or ``(E, M)``.  A weight of exactly 0 (as rounded to
    the call's ``precision`` on the GPU, in float64 on the numpy branch) masks its band whatever ``obs`` holds there: 0
    is selected into ``obs`` before the upload and before the numpy data term, whose kernels and formulas multiply by
    the weight and do not select; a NaN or an infinity in ``obs`` under a non-zero weight, or in a weight, makes the
    row's results NaN.  On the GPU
    (``BatchModel.misfit``, ``gp_band_misfit_host``) the per-emulator means, gradients and residuals never leave the
    device; no inverse is stacked or uploaded.  ``is_gpu=False`` is the explicit numpy branch, built from each
    emulator's ``cpu_predict(do_unc=False)`` and ``hessian``; never a fallback.

    ``devices`` shards the EMULATORS like ``hessian_bands``: every device returns the partial sums of its block and
    they are added on the host in device order (``wr`` rows are the blocks' own).  ``misfit_fn(device, gps_block, X,
    obs_block, weights_block, second_order, return_residual)`` replaces the HIP path in the CPU tests of that logic.

    ``emulator_unc=True`` adds each emulator's own predictive variance ``v_e(x)`` to the observation's ``1 / w``
    (``weights`` must then be inverse variances, >= 0).  With ``vp = v if v > 0 else 0`` (and ``dvp = dv/dx`` likewise):

        weff = w / (1 + w vp)                      a = weff r        c = 1/2 weff (1 - a r)      q = 1/2 weff^2
        cost[m] = 1/2 sum_e [a r + log1p(w vp)]    grad[m] = sum_e [a dmu_e/dx + c dvp]
        gn[m]   = sum_e [weff dmu dmu^T + q dvp dvp^T]       (c = q = 0 where v <= 0: the plain term with weff = w)

    the Gaussian negative log-likelihood without the constant ``-log w`` and, for ``gn``, the Fisher information of a
    Gaussian whose mean and variance both depend on x.  ``second_order`` is None or "gauss_newton" ("full" would need
    the Hessian of the variance: ``ValueError``); ``return_residual`` appends ``wr = weff r`` AND ``weff``, both
    ``(E, M)``.  On the GPU (``BatchModel.misfit_unc``, ``gp_band_misfit_unc_device``) the batch is built WITH invQ and
    arrays are converted to ``precision``; ``is_gpu=False`` is the explicit numpy branch from ``cpu_predict(do_unc=True)``
    and ``variance_gradient(is_gpu=False)``; never a fallback.  ``devices=`` shards as above (every sum is additive
    over blocks of emulators); ``misfit_fn`` then also receives ``emulator_unc=True`` as a keyword.  With ``False``
    every path makes exactly the calls it always made."""
    if second_order not in (None, "gauss_newton", "full"):
        raise ValueError("second_order must be None, 'gauss_newton' or 'full'")
    if emulator_unc:
        _check_unc_order(second_order)
    X, inputs = _rows_and_inputs(gps, X, "X")
    E, M = len(gps), X.shape[0]
    obs = _em_broadcast(obs, E, M, "obs")
    if weights is not None:
        weights = _em_broadcast(weights, E, M, "weights")
    obs = _first_guess.mask_obs(obs, weights, precision if is_gpu else np.float64)

    def block(a, e0, e1):           # a block of emulators in the shape the caller gave: (e,) or (e, M)
        if a is None:
            return None
        return a[e0:e1, 0] if a.shape[1] == 1 and M != 1 else a[e0:e1]

    def hook(dev, e0, e1):
        kw = {"emulator_unc": True} if emulator_unc else {}
        return tuple(misfit_fn(dev, gps[e0:e1], X, block(obs, e0, e1), block(weights, e0, e1), second_order,
                               return_residual, **kw))

    def on_device(batch, e0, e1):
        call = batch.misfit_unc if emulator_unc else batch.misfit
        return call(X, block(obs, e0, e1), block(weights, e0, e1), second_order, return_residual)

    if devices is None:
        if misfit_fn is not None:
            return hook(device, 0, E)
        if not is_gpu:
            numpy_form = _misfit_unc_numpy if emulator_unc else _misfit_numpy
            return numpy_form(gps, np.asarray(X, dtype=np.float64), obs, weights, second_order, return_residual)
        with _batch_model(_lib.default_context(device), gps, inputs, precision, bool(emulator_unc)) as batch:
            return on_device(batch, 0, E)
    if len(devices) < 1:
        raise ValueError("devices must name at least one device")
    if not is_gpu and misfit_fn is None:
        raise ValueError("devices= shards the GPU path; the numpy branch runs in the calling thread")
    partial = _on_shards(gps, devices, inputs, precision, bool(emulator_unc), on_device, hook if misfit_fn else None)
    parts = [p for p in partial if p is not None]          # device order
    n_sum = 3 if second_order else 2
    total = [np.array(a) for a in parts[0][:n_sum]]
    for p in parts[1:]:
        for acc, a in zip(total, p[:n_sum]):
            acc += a
    if return_residual:
        for k in range(n_sum, n_sum + (2 if emulator_unc else 1)):          # wr (and weff): the blocks' own rows
            total.append(np.concatenate([p[k] for p in parts], axis=0))
    return tuple(total)


def retrieve_bands(gps, X0, obs, weights=None, second_order="gauss_newton", prior=None, bounds=None, lam0=1e-2,
                   max_iter=20, down=1.0 / 3.0, up=4.0, ftol=1e-10, xtol=0.0, is_gpu=True, precision=np.float64,
                   device=None, step_fn=None, return_cov=False, next_prior=None, return_A=False, emulator_unc=False,
                   bounds_mode="clamp", return_active=False):
    """Levenberg-Marquardt retrieval of M state vectors at once on E per-band emulators: minimises, row by row,

        F(x) = 1/2 sum_e w (mu_e(x) - obs[e])^2  (+ 1/2 (x - x0)^T P (x - x0) with ``prior=(x0 (D,), P (D, D))``)

    from ``X0`` (M, D), inside ``bounds=(lo (D,), hi (D,))`` when given.  ``obs`` and ``weights`` as in
    ``misfit_bands``: a weight of exactly 0 masks its band whatever ``obs`` holds there (a cloudy or missing band may
    be NaN or a fill value under it); a row with a NaN or an infinity in ``obs`` under a non-zero weight, in a weight or
    in ``X0`` is never accepted and comes back as it went in ("Invalid pixels in the retrievals").
    ``second_order`` is "gauss_newton" or "full" (the matrix A of the step).  An iteration is: the
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
    ignored: a component held at its bound gets the unconstrained variance (``return_active=True`` says which
    components those are).  ``C`` is a covariance only when
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
    ``False`` nothing changes.

    ``emulator_unc=True`` minimises the data term of ``misfit_bands(emulator_unc=True)`` instead: every emulator's
    predictive variance widens its observation's, ``A`` is the Fisher matrix, and ``cov``, ``sigma``, ``next_prec``, ``A``
    and the smoother of ``retrieve_bands_series`` then carry the emulators' share of the error.  The loop is the same;
    only the misfit it calls differs (``misfit_unc_device`` on a batch built with invQ; ``_misfit_unc_numpy``).
    ``second_order="full"`` raises ``ValueError``.  With ``False`` nothing changes.

    ``bounds_mode`` is "clamp" (the default: the step above, bit for bit what it always was) or "active_set": the trial
    is then ``x + delta`` with ``delta`` the exact minimiser of the damped model ``1/2 d^T (A + P + lambda diag) d + g'^T d``
    inside the box ``lo - x <= d <= hi - x`` (``gp_box_step_device``, a primal active-set method; ``_lib.box_step_numpy``
    on the numpy branch; DESIGN.md, "Bound-constrained step").  A row that sits on a bound with correlated parameters then
    takes a descent step where the clamped one is rejected.  It needs ``bounds``; the rest of the loop is unchanged.

    ``return_active=True`` (either mode; needs ``bounds``) appends, behind everything else, ``active (M, D) int8`` -- -1
    where ``X <= lo`` and ``g' > 0``, +1 where ``X >= hi`` and ``g' < 0``, 0 otherwise, ``g' = grad + P (X - x0)`` at the
    returned ``X`` -- and ``kkt (M,)``, the largest ``|g'_d| / sqrt((A + P)_dd)`` over the components with ``active == 0``:
    the scaled projected gradient, which tells whether a row flagged unconverged is in fact at a constrained minimum.
    Numpy arithmetic in both branches; on the GPU one more download, of the loop's gradient."""
    if second_order not in ("gauss_newton", "full"):
        raise ValueError("second_order must be 'gauss_newton' or 'full'")
    if emulator_unc:
        _check_unc_order(second_order)
    _retrieve.check_bounds_mode(bounds_mode, bounds, return_active)
    X0, inputs = _rows_and_inputs(gps, X0, "X0")
    E, (M, D) = len(gps), X0.shape
    obs = _em_broadcast(obs, E, M, "obs")
    if weights is not None:
        weights = _em_broadcast(weights, E, M, "weights")
    obs = _first_guess.mask_obs(obs, weights, precision if is_gpu and step_fn is None else np.float64)
    prior, bounds = _retrieve.prior_and_bounds(prior, bounds, D, M)
    max_iter = int(max_iter)

    if step_fn is not None or not is_gpu:
        step = step_fn if step_fn is not None else _retrieve.numpy_step(prior, bounds, bounds_mode)
        return _retrieve.lm_numpy(_data_term_numpy(gps, obs, weights, second_order, emulator_unc), step, X0, lam0,
                                  max_iter, down, up, ftol, xtol, prior, return_cov, next_prior, return_A,
                                  bounds if return_active else None)

    ctx = _lib.default_context(device)
    with _batch_model(ctx, gps, inputs, precision, bool(emulator_unc)) as batch, \
            _retrieve.Scratch(ctx, np.dtype(precision)) as scratch:
        misfit = _data_term_device(batch, scratch, obs, weights, M, second_order, emulator_unc)
        return _retrieve.lm_device(scratch, M, D, X0, lam0, prior, bounds, max_iter, down, up, ftol, xtol, return_cov,
                                   misfit, next_prior, return_A, bounds_mode, return_active)


def _data_term_numpy(gps, obs, weights, second_order, emulator_unc):
    """The data term of the retrievals on the host: ``X (R, D) -> (cost, grad, A)`` for ``obs`` and ``weights`` as
    ``_em_broadcast`` returns them for those R rows."""
    numpy_form = _misfit_unc_numpy if emulator_unc else _misfit_numpy
    return lambda X: numpy_form(gps, X, obs, weights, second_order, False)


def _data_term_device(batch, scratch, obs, weights, n_rows, second_order, emulator_unc):
    """The data term of the retrievals on the device: ``obs`` and ``weights`` (as ``_em_broadcast`` returns them for
    the ``n_rows`` rows) go up once, into ``scratch``; ``misfit(d_rows, d_cost, d_grad, d_A)`` enqueues
    ``misfit_device`` (``misfit_unc_device`` with ``emulator_unc``) on those rows."""
    M = n_rows

    def strides(a):
        return (1, 0) if a.shape[1] == 1 and M != 1 else (M, 1)
    d_obs = scratch.up(obs)
    d_w = scratch.up(weights) if weights is not None else None
    os_, ws = strides(obs), strides(weights) if weights is not None else (0, 0)

    def misfit(d_rows, c, g, a):
        if emulator_unc:
            return batch.misfit_unc_device(d_rows, d_obs, os_, d_w, ws, c, g, M, d_gn=a)
        batch.misfit_device(d_rows, d_obs, os_, d_w, ws, c, g, M, d_gn=a if second_order == "gauss_newton" else None,
                            d_hess=a if second_order == "full" else None)
    return misfit


def _joint_em_rows(a, T, E, M, name):
    """``a`` (T, E, M) -- or per date anything ``_em_broadcast`` takes -- as one float64 (E, T M) array, date-major
    along the rows: what a data-term call on the T M rows of a series reads."""
    if len(a) != T:
        raise ValueError("%s has %d dates, obs %d" % (name, len(a), T))
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(_em_broadcast(a[t], E, M, name), (E, M)) for t in range(T)], axis=1))


def retrieve_bands_joint(gps, X0, obs, weights, prior, noise, second_order="gauss_newton", bounds=None, lam0=1e-2,
                         max_iter=20, down=1.0 / 3.0, up=4.0, ftol=1e-10, xtol=0.0, is_gpu=True, precision=np.float64,
                         device=None, return_cov=False, emulator_unc=False, work_budget=None, bounds_mode="clamp"):
    """Joint maximum a posteriori retrieval of M trajectories of T dates on E per-band emulators: minimises, pixel by
    pixel and over all dates at once, the objective the series is built around,

        F(x_0 .. x_{T-1}) = sum_t J_t(x_t) + 1/2 (x_0 - xp)^T P (x_0 - xp) + 1/2 sum_{t>=1} (x_t - x_{t-1})^T W (x_t - x_{t-1})

    with ``J_t`` the data term of ``retrieve_bands`` on date t's ``obs[t]`` (E, M) and ``weights[t]``, ``prior = (xp,
    P)`` on date 0 (shared or per pixel; required) and ``W = Q^-1`` the inverse of the process noise ``noise`` (D, D) or
    (M, D, D).  The joint form needs a POSITIVE DEFINITE ``Q``: it is inverted once, before the loop; a shared ``Q``
    that does not factor raises ``ValueError``, a pixel's own that does not gives that pixel a NaN ``W``, a non-zero
    ``cov_status`` and no accepted step.  ``X0`` is (T, M, D); an (M, D) array is taken for every date.

    The loop is ``retrieve_bands``' (its schedule, constants and keywords) on whole trajectories: one data-term call on
    the T M rows of the trial trajectories, the accept / reject of every pixel's trajectory as a whole, then the
    block-tridiagonal damped Newton step (``gp_series_step_device``: block Cholesky over the dates).  Where the
    emulators are linear the minimiser is the smoothed trajectory of ``retrieve_bands_series(smooth=True)``; where they
    are not, it is the minimiser and the smoother is not.  ``second_order`` must be "gauss_newton" (the Hessian of F
    must stay positive definite: "full" raises ``ValueError``).  A weight of exactly 0 masks its band; a date with all
    weights 0 is an ordinary date; a pixel with a NaN or an infinity on any date -- in ``obs`` under a non-zero weight,
    in a weight, in ``X0`` or in its own prior -- is never accepted and comes back as it went in, and every other pixel
    is bit for bit the call without it.

    Returns ``(X (T, M, D), sigma (T, M, D), cost (T, M), F (M,), state (M,) int32, n_accepted (M,) int32, lam (M,),
    cov_status (M,) int32)``: ``sigma`` the square roots of the diagonals of the marginal posterior covariances (the
    diagonal blocks of the inverse of the undamped Hessian, ``gp_series_cov_device``), ``cost`` the data terms, ``F`` the
    joint objective at ``X`` (NaN for a pixel no decision was made for), ``cov_status`` 0 or t D + k + 1 for the first
    failed pivot (then the pixel's ``sigma`` is NaN).  ``return_cov=True`` appends ``cov (T, M, D, D)``.

    On the GPU the pixels are cut into runs whose work memory (the factors between the two sweeps, 8 (D (D + 1) / 2 +
    D (D | 1) + D) bytes per pixel and date) stays under ``work_budget`` bytes (default 1 GiB); the cut changes no
    bit.  ``is_gpu=False`` is the explicit numpy branch (``_retrieve.lm_series_numpy``); never a fallback.
    ``bounds_mode`` is "clamp" only: the box step of ``retrieve_bands`` has no block-tridiagonal form yet, and anything
    else raises ``ValueError``."""
    _retrieve.clamp_only(bounds_mode)
    if second_order != "gauss_newton":
        raise ValueError("the joint retrieval needs second_order='gauss_newton': the Hessian of F must stay positive definite")
    if prior is None:
        raise ValueError("a joint retrieval needs a prior")
    T, E = len(obs), len(gps)
    if T == 0:
        raise ValueError("obs has no dates")
    X0 = _retrieve.joint_start(X0, T)
    M, D = X0.shape[1:]
    _, inputs = _rows_and_inputs(gps, X0.reshape(T * M, D), "X0")
    obs = _joint_em_rows(obs, T, E, M, "obs")
    if weights is not None:
        weights = _joint_em_rows(weights, T, E, M, "weights")
    obs = _first_guess.mask_obs(obs, weights, precision if is_gpu else np.float64)
    loop = (bounds, lam0, max_iter, down, up, ftol, xtol, return_cov)

    def rows_of(a, m0, m1):           # the pixels m0 .. m1 of every date of an (E, T M) array
        return None if a is None else np.ascontiguousarray(a.reshape(E, T, M)[:, :, m0:m1].reshape(E, T * (m1 - m0)))
    if not is_gpu:
        def numpy_term(m0, m1):
            return _data_term_numpy(gps, rows_of(obs, m0, m1), rows_of(weights, m0, m1), second_order, emulator_unc)
        return _retrieve.retrieve_joint(X0, prior, noise, *loop, numpy_term=numpy_term)
    ctx = _lib.default_context(device)
    with _batch_model(ctx, gps, inputs, precision, bool(emulator_unc)) as batch:
        def device_term(scratch, m0, m1):
            return _data_term_device(batch, scratch, rows_of(obs, m0, m1), rows_of(weights, m0, m1), T * (m1 - m0),
                                     second_order, emulator_unc)
        return _retrieve.retrieve_joint(X0, prior, noise, *loop, device_term=device_term, context=ctx, precision=precision,
                                        work_budget=work_budget)


def candidate_table(gps, candidates=None, precision=np.float64, device=None):
    """The device table of ``first_guess_bands``: the E emulators' means at the ``candidates`` (L, D) -- None: the
    emulators' shared training inputs -- as the term-major ``(E, L)`` array ``predict_mean_grad_device`` writes, kept on
    the device.  A context manager (``_first_guess.DeviceTable``): pass it as ``table=`` so that repeated calls (dates,
    tiles) do not compute the means again; leaving the block frees it.  One ``BatchModel`` without invQ is built for the
    call and closed again; the candidates' gradients, which the kernel writes beside the means, are dropped."""
    inputs = _check_shared_inputs(gps)
    cand = _first_guess.check_candidates(inputs if candidates is None else candidates, inputs.shape[1])
    ctx, dt = _lib.default_context(device), _lib.precision_dtype(precision)
    E, (L, D) = len(gps), cand.shape
    d_mu = ctx.malloc(E * L * dt.itemsize)
    try:
        with _batch_model(ctx, gps, inputs, dt, False) as batch, _lib.Scratch(ctx, dt) as scratch:
            batch.predict_mean_grad_device(scratch.up(cand), d_mu, scratch.alloc(E * L * D * dt.itemsize), L)
            ctx.synchronize()
    except Exception:
        ctx.free(d_mu)
        raise
    return _first_guess.DeviceTable(ctx, dt, d_mu, (L, 1), E, cand, tuple(gps))


def _owner(tb, gps):
    return tb.owner if len(tb.owner) == len(gps) and all(a is b for a, b in zip(tb.owner, gps)) else None


def first_guess_bands(gps, candidates, obs, weights=None, prior=None, n_best=1, is_gpu=True, precision=np.float64,
                      device=None, table=None):
    """The starting states of ``retrieve_bands`` by look-up-table search: among the ``candidates`` (L, D) -- None: the
    emulators' shared training inputs, where the emulator error is smallest -- per row the ``n_best`` (1..8) of lowest

        J[m, l] = a[l] + 1/2 sum_e w[e, m] (mu_e(c_l) - obs[e, m])^2,     a[l] = 1/2 (c_l - x0)^T P (c_l - x0)

    with ``obs`` and ``weights`` as ``misfit_bands`` takes them -- (E,) or (E, M); M is 1 when both are (E,) -- and
    ``prior=(x0 (D,), P (D, D))`` shared by the rows (a per-row prior is a ``ValueError``: it is not an offset per
    candidate; ``a`` is formed on the host).  Returns ``(X0, cost0, index)``: ``index (M, n_best)`` int32 and
    ``cost0 (M, n_best)`` ascending by (cost, index), exact ties to the lower index, and ``X0 = candidates[index]``,
    (M, D) for ``n_best`` 1, else (M, n_best, D).  A weight of exactly 0 masks its band whatever ``obs`` holds there;
    a row with a NaN or an infinity in ``obs`` or in a non-zero weight gets index -1, cost NaN and a NaN state.

    On the GPU one ``BatchModel`` without invQ evaluates ``predict_mean_grad_device`` at the candidates, the (E, L)
    means stay on the device as the table, ``obs`` and ``weights`` go up once, ``gp_lut_search_device`` searches, and
    only ``index`` and ``cost`` come back; the gather of ``X0`` is numpy.  ``table=`` (a ``candidate_table``) reuses a
    table made earlier: ``candidates`` may then be None.  ``is_gpu=False`` is the explicit numpy branch, from each
    emulator's ``cpu_predict(do_unc=False)`` and ``_lib.lut_search_numpy``; never a fallback."""
    inputs = _check_shared_inputs(gps)
    E, D = len(gps), inputs.shape[1]
    if table is not None and candidates is None:
        cand = table.candidates
    else:
        cand = _first_guess.check_candidates(inputs if candidates is None else candidates, D)
    n_best = _first_guess.check_n_best(n_best, cand.shape[0])
    obs = np.asarray(obs, dtype=np.float64)
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float64)
    rows = [a.shape[1] for a in (obs, weights) if a is not None and a.ndim == 2]
    M = rows[0] if rows else 1
    obs = _em_broadcast(obs, E, M, "obs")
    if weights is not None:
        weights = _em_broadcast(weights, E, M, "weights")
    prior = _first_guess.shared_prior(prior, D)
    offset = _first_guess.prior_offset(cand, prior)
    if not is_gpu:
        S = np.stack([np.asarray(gp.cpu_predict(cand, do_unc=False)[0]) for gp in gps], axis=1)        # (L, E)
        index, cost = _lib.lut_search_numpy(S, np.broadcast_to(obs, (E, M)).T,
                                            None if weights is None else np.broadcast_to(weights, (E, M)).T, offset, n_best)
    else:
        tb = table if table is not None else candidate_table(gps, cand, precision, device)
        try:
            tb.check(_owner(tb, gps), precision, E)
            if tb.candidates.shape != cand.shape or (tb.candidates is not cand and not np.array_equal(tb.candidates, cand)):
                raise ValueError("table= was built for other candidates")

            def strides(a):
                return (1, 0) if a.shape[1] == 1 and M != 1 else (M, 1)
            index, cost = _first_guess.search_table(tb, obs, strides(obs), weights,
                                                    strides(weights) if weights is not None else (0, 0), offset, M, n_best)
        finally:
            if table is None:
                tb.close()
    return _first_guess.gather_starts(cand, index, n_best), cost, index


def posterior_bands(gps, candidates, obs, weights=None, prior=None, is_gpu=True, precision=np.float64, device=None,
                    table=None):
    """The Bayesian look-up-table posterior of every row: instead of the best candidates (``first_guess_bands``), every
    candidate (L, D) -- None: the emulators' shared training inputs -- weighted by its likelihood,

        w[m, l] = exp(-(J[m, l] - Jmin[m])),    J = first_guess_bands' J (``obs``, ``weights`` and ``prior`` as there)

    and the weighted moments of the candidate states.  Returns ``(mean (M, D), cov (M, D, D), info)`` in float64;
    ``info = dict(index (M,) int32, cost (M,), log_evidence (M,), ess (M,))``: the best candidate and its J (the search
    at ``n_best = 1``), ``log_evidence = log sum_l exp(-J) - log L`` (the Monte-Carlo estimate of the evidence for
    candidates drawn from the prior; for comparing priors, band sets or emulators on one observation) and the
    effective sample size ``(sum w)^2 / sum w^2`` (near 1: the table is too sparse for this row, and so is its first
    guess).  The sums are centred on the row's best candidate: a posterior on one candidate gives that candidate bit for
    bit, ``cov`` 0 and ``ess`` 1.  A row without a finite J gets index -1 and NaN.  Unlike ``retrieve_bands(return_cov=
    True)`` the moments see every basin of the data term, a parameter the bands do not constrain and a posterior that
    leans on the box.  On the GPU the table is ``candidate_table`` (``table=`` reuses one), the states go up once per
    call and ``gp_lut_posterior_device`` folds; ``is_gpu=False`` is the explicit numpy branch
    (``_lib.lut_posterior_numpy`` on ``cpu_predict`` means); never a fallback."""
    inputs = _check_shared_inputs(gps)
    E, D = len(gps), inputs.shape[1]
    if table is not None and candidates is None:
        cand = table.candidates
    else:
        cand = _first_guess.check_candidates(inputs if candidates is None else candidates, D)
    obs = np.asarray(obs, dtype=np.float64)
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float64)
    rows = [a.shape[1] for a in (obs, weights) if a is not None and a.ndim == 2]
    M = rows[0] if rows else 1
    obs = _em_broadcast(obs, E, M, "obs")
    if weights is not None:
        weights = _em_broadcast(weights, E, M, "weights")
    offset = _first_guess.prior_offset(cand, _first_guess.shared_prior(prior, D))
    if not is_gpu:
        S = np.stack([np.asarray(gp.cpu_predict(cand, do_unc=False)[0]) for gp in gps], axis=1)        # (L, E)
        out = _lib.lut_posterior_numpy(S, cand, np.broadcast_to(obs, (E, M)).T,
                                       None if weights is None else np.broadcast_to(weights, (E, M)).T, offset)
    else:
        tb = table if table is not None else candidate_table(gps, cand, precision, device)
        try:
            tb.check(_owner(tb, gps), precision, E)
            if tb.candidates.shape != cand.shape or (tb.candidates is not cand and not np.array_equal(tb.candidates, cand)):
                raise ValueError("table= was built for other candidates")

            def strides(a):
                return (1, 0) if a.shape[1] == 1 and M != 1 else (M, 1)
            out = _first_guess.posterior_table(tb, obs, strides(obs), weights,
                                               strides(weights) if weights is not None else (0, 0), offset, M)
        finally:
            if table is None:
                tb.close()
    return _first_guess.posterior_result(out, cand.shape[0])


def retrieve_bands_multistart(gps, candidates, obs, weights=None, n_starts=4, table=None, **loop_args):
    """``retrieve_bands`` from several starts per pixel: ``first_guess_bands`` with ``n_best = n_starts``, ranked with
    the loop's shared ``prior``; the starts clipped to ``bounds``; ONE ``retrieve_bands`` call on the ``M n_starts``
    rows (row-shaped ``obs``, ``weights`` and ``next_prior`` repeated, shared ones passed through); per pixel the start
    of lowest ``F = cost + prior term`` is kept (``_retrieve._prior_term``; ties to the lower start, a non-finite F
    loses; the selection is numpy on a few (M,) arrays).  ``loop_args`` are ``retrieve_bands``' keywords
    (``is_gpu``, ``precision`` and ``device`` also choose the first guess's branch); ``emulator_unc``, ``step_fn`` and
    per-row priors are not offered.  Returns ``(results, start (M,) int32, cost0 (M, n_starts))``: ``results`` is exactly
    the tuple ``retrieve_bands`` returns for M rows, every array gathered from the chosen start."""
    D = _check_shared_inputs(gps).shape[1]
    fg = {k: loop_args[k] for k in ("is_gpu", "precision", "device") if k in loop_args}

    def first_guess(prior, n_best):
        return first_guess_bands(gps, candidates, obs, weights, prior, n_best, table=table, **fg)

    def retrieve(X0, obs_r, w_r, **kw):
        return retrieve_bands(gps, X0, obs_r, w_r, **kw)
    return _first_guess.multistart(first_guess, retrieve, 1, obs, weights, n_starts, D, loop_args)


def retrieve_bands_series(gps, X0, obs, weights, prior, noise, smooth=False, joint=False, **loop_args):
    """A time series of ``retrieve_bands`` on the emulators ``gps``: ``obs`` (T, E, M) -- or anything ``retrieve_bands``
    takes, per date -- and ``weights`` the same or None, one retrieval per date, the posterior of a date propagated by
    the process noise ``noise`` (D, D) or (M, D, D) into the prior of the next (``_retrieve.retrieve_series``: what it
    returns, and why ``prior`` is required).  ``loop_args`` are ``retrieve_bands``' other keywords.

    ``smooth=True`` appends the Rauch-Tung-Striebel smoothed trajectory ``X_s (T, M, D)``, ``sigma_s (T, M, D)`` and
    ``smooth_status (T, M)``: every date then also carries the observations after it (a gap is filled from both
    sides).  On the GPU the backward pass is one ``rts_smooth_device`` call per date with the smoothed state and
    covariance of the later date resident on the device; with ``is_gpu=False`` (or a ``step_fn``) it is
    ``_lib.rts_smooth_numpy``; never a fallback.

    ``joint=True`` runs the filter and the smoother as ``smooth=True`` does, starts ``retrieve_bands_joint`` from the
    smoothed trajectory ``X_s`` and appends its eight values to the ten: the minimiser of the series' objective, which
    the smoother is on linear emulators only.  The loop's keywords go to both; ``step_fn`` has no joint form
    (``ValueError``).  With ``False`` nothing changes."""
    def retrieve(X, obs_t, weights_t, **kw):
        return retrieve_bands(gps, X, obs_t, weights_t, **kw)
    if joint:
        if loop_args.get("step_fn") is not None:
            raise ValueError("joint=True has no step_fn form")
        out = retrieve_bands_series(gps, X0, obs, weights, prior, noise, smooth=True, **loop_args)
        return out + retrieve_bands_joint(gps, out[7], obs, weights, prior, noise,
                                          **{k: v for k, v in loop_args.items() if k != "step_fn"})
    if not smooth:
        return _retrieve.retrieve_series(retrieve, X0, obs, weights, prior, noise, **loop_args)
    on_device = loop_args.get("is_gpu", True) and loop_args.get("step_fn") is None
    context = (lambda: _lib.default_context(loop_args.get("device"))) if on_device else None
    return _retrieve.retrieve_series(retrieve, X0, obs, weights, prior, noise, smooth=True, context=context, **loop_args)

