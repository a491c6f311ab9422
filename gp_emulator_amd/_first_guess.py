"""The first guess of a retrieval and the multi-start wrappers: what ``perband.first_guess_bands`` and
``MultivariateEmulator.first_guess_many`` share.  The callers build the table (the emulators' means at the candidate
states, on the device or in numpy) and lay out ``obs`` and ``weights``; the prior's offset, the search call, the gather
of the starting rows and the selection among several starts are stated here once."""
import numpy as np

from . import _lib, _retrieve


def shared_prior(prior, D):
    """``prior`` as float64 ``(x0 (D,), P (D, D))`` or None.  A per-row prior is a ``ValueError``: the search ranks by
    one offset per candidate."""
    if prior is None:
        return None
    x0, P = np.asarray(prior[0], dtype=np.float64), np.asarray(prior[1], dtype=np.float64)
    if x0.shape != (D,) or P.shape != (D, D):
        raise ValueError("the first guess takes a prior shared by the rows, x0 (%d,) and P (%d, %d): a per-row prior "
                         "is not an offset per candidate" % (D, D, D))
    return x0, P


def prior_offset(candidates, prior):
    """``a[l] = 1/2 (c_l - x0)^T P (c_l - x0)`` in float64 on the host (L D^2 operations), summed as the loop sums its
    prior term; None without a prior."""
    if prior is None:
        return None
    return _retrieve._prior_term(np.asarray(candidates, dtype=np.float64), prior)


def check_candidates(candidates, D):
    c = np.asarray(candidates, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != D:
        raise ValueError("candidates must be (n_candidates, %d), got %s" % (D, c.shape))
    return c


def gather_starts(candidates, index, n_best):
    """``candidates[index]``, NaN where ``index`` is -1: (M, D) for ``n_best`` 1, else (M, n_best, D)."""
    X0 = candidates[np.maximum(index, 0)]
    X0[index < 0] = np.nan
    return X0[:, 0] if n_best == 1 else X0


class DeviceTable(object):
    """A table of candidate means resident on the device: what ``candidate_table`` of either emulator type hands to
    ``table=``.  ``d_table`` holds element (term k, candidate l) at ``k * strides[0] + l * strides[1]``; ``close()``
    (or leaving the ``with`` block) frees it.  ``space`` tags what the terms are: "band" (the terms of the data term
    itself: bands, or per-band emulators) or "pc" (the per-PC means of a ``MultivariateEmulator``, searched by
    ``gp_lut_search_pc_device``)."""

    def __init__(self, ctx, dtype, d_table, strides, n_terms, candidates, owner, space="band"):
        self.ctx, self.dtype, self.d_table, self.strides = ctx, np.dtype(dtype), d_table, strides
        self.n_terms, self.candidates, self.owner, self.space = n_terms, candidates, owner, space

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.d_table is not None:
            self.ctx.free(self.d_table)
            self.d_table = None

    def check(self, owner, dtype, n_terms, space="band"):
        if self.d_table is None:
            raise ValueError("the candidate table has been closed")
        if self.space != space:
            raise ValueError("table= is a %r-space table, the call searches in %r space" % (self.space, space))
        if self.owner is not owner or self.dtype != np.dtype(dtype) or self.n_terms != n_terms:
            raise ValueError("table= was built for other emulators or another precision")


def search_table(tb, obs, obs_strides, weights, w_strides, offset, M, n_best):
    """The search of ``M`` rows against the device table ``tb``: ``obs`` and ``weights`` (host arrays laid out as
    their strides say) go up once, only ``index`` and ``cost`` come back."""
    ctx, dt = tb.ctx, tb.dtype
    with _lib.Scratch(ctx, dt) as scratch:
        d_o, d_w, d_a = scratch.up(obs), scratch.up(weights), scratch.up(offset)
        d_i, d_c = scratch.alloc(M * n_best * 4), scratch.alloc(M * n_best * dt.itemsize)
        ctx.lut_search_device(dt, tb.d_table, tb.strides, d_a, d_o, obs_strides, d_w, w_strides, d_i, d_c, M,
                              tb.candidates.shape[0], tb.n_terms, n_best)
        return _lib._download(ctx, d_i, (M, n_best), np.int32), _lib._download(ctx, d_c, (M, n_best), dt)


def posterior_table(tb, obs, obs_strides, weights, w_strides, offset, M):
    """The look-up-table posterior of ``M`` rows against the device table ``tb`` (``gp_lut_posterior_device``): ``obs``,
    ``weights``, the offset and the candidate states (as the table's dtype) go up once per call; ``index``, ``cost`` and
    the float64 ``mean``, ``cov``, ``lse`` and ``ess`` come back."""
    ctx, dt = tb.ctx, tb.dtype
    L, D = tb.candidates.shape
    with _lib.Scratch(ctx, dt) as scratch:
        d_o, d_w, d_a, d_x = scratch.up(obs), scratch.up(weights), scratch.up(offset), scratch.up(tb.candidates)
        d_i, d_c = scratch.alloc(M * 4), scratch.alloc(M * dt.itemsize)
        d_m, d_v, d_l, d_e = scratch.alloc(M * D * 8), scratch.alloc(M * D * D * 8), scratch.alloc(M * 8), scratch.alloc(M * 8)
        ctx.lut_posterior_device(dt, tb.d_table, tb.strides, d_a, d_o, obs_strides, d_w, w_strides, d_x, (D, 1), D, d_i, d_c,
                                 d_m, d_v, d_l, d_e, M, L, tb.n_terms)
        return (_lib._download(ctx, d_i, (M,), np.int32), _lib._download(ctx, d_c, (M,), dt),
                _lib._download(ctx, d_m, (M, D), np.float64), _lib._download(ctx, d_v, (M, D, D), np.float64),
                _lib._download(ctx, d_l, (M,), np.float64), _lib._download(ctx, d_e, (M,), np.float64))


def posterior_result(out, L):
    """``(mean, cov, info)`` from ``(index, cost, mean, cov, lse, ess)``: ``log_evidence = lse - log L``, the Monte-Carlo
    estimate of the evidence for ``L`` candidates drawn from the prior."""
    index, cost, mean, cov, lse, ess = out
    return mean, cov, dict(index=index, cost=cost, log_evidence=lse - np.log(L), ess=ess)


def rows_of(a, rows):
    """``a[rows]`` of a row-shaped array; a shared vector or None as it is."""
    return a if a is None or a.ndim == 1 else a[rows]


def search_table_rows(tb, obs, weights, offset, M, n_best):
    """``search_table`` for row-major host arrays: ``obs`` (K,) or (M, K), ``weights`` None, (K,) or (M, K)."""
    def strides(a):
        return (1, tb.n_terms) if a.ndim == 2 else (1, 0)
    return search_table(tb, obs, strides(obs), weights, strides(weights) if weights is not None else (0, 0), offset, M, n_best)


def route_rows(index, cost, status, band_search):
    """The rows the PC form could not centre (``status != 0``) searched in band space: ``band_search(rows)`` returns
    their ``(index, cost)``, which replace, in place, the empty slots the PC search left.  Returns how many there were."""
    rows = np.flatnonzero(status != 0)
    if rows.size:
        index[rows], cost[rows] = band_search(rows)
    return int(rows.size)


def mask_obs(obs, weights, dtype):
    """``obs`` with 0 selected in wherever the weight, rounded to the device ``dtype``, is exactly 0 (``obs`` itself
    without weights, or when no weight is 0): what the PC-space set-up, the misfits and the retrievals take, whose
    kernels and numpy forms multiply by the weight and do not select."""
    if weights is None:
        return obs
    masked = np.asarray(weights, dtype=dtype) == 0
    return np.where(masked, 0.0, obs) if masked.any() else obs


def search_table_pc(tb, d_basis, obs, weights, offset, M, n_best, n_bands, stages=None):
    """The PC-space search of ``M`` rows against the device table ``tb`` of per-PC means: ``obs`` (masked terms
    selected to 0 here) and ``weights`` go up once, ``gp_mv_lut_prepare_device`` and ``gp_lut_search_pc_device`` run on
    the context's stream, ``index``, ``cost`` and ``status`` come back.  ``stages``: a dict that receives the device
    times in ms of the set-up and of the search (HIP events), for the timing tool."""
    ctx, dt = tb.ctx, tb.dtype
    P, L, isz = tb.n_terms, tb.candidates.shape[0], tb.dtype.itemsize
    obs = mask_obs(obs, weights, dt)
    per_row = weights is not None and weights.ndim == 2
    with _lib.Scratch(ctx, dt) as scratch:
        d_o, d_w, d_a = scratch.up(obs), scratch.up(weights), scratch.up(offset)
        d_G = scratch.alloc((M if per_row else 1) * P * P * isz)
        d_c0, d_j0, d_g0, d_st = scratch.alloc(P * M * isz), scratch.alloc(M * isz), scratch.alloc(P * M * isz), scratch.alloc(M * 4)
        d_i, d_c = scratch.alloc(M * n_best * 4), scratch.alloc(M * n_best * isz)
        ev = [ctx.event() for _ in range(3)] if stages is not None else None
        if ev:
            ctx.record(ev[0])
        ctx.mv_lut_prepare_device(dt, d_basis, d_o, n_bands if obs.ndim == 2 else 0, d_w, n_bands if per_row else 0, d_G,
                                  P * P if per_row else 0, d_c0, d_j0, d_g0, d_st, M, P, n_bands)
        if ev:
            ctx.record(ev[1])
        ctx.lut_search_pc_device(dt, tb.d_table, tb.strides, d_a, d_c0, d_j0, d_g0, d_G, P * P if per_row else 0, d_st, d_i,
                                 d_c, M, L, P, n_best)
        if ev:
            ctx.record(ev[2])
        out = (_lib._download(ctx, d_i, (M, n_best), np.int32), _lib._download(ctx, d_c, (M, n_best), dt),
               _lib._download(ctx, d_st, (M,), np.int32))
        if ev:
            stages["prepare_ms"], stages["search_ms"] = ctx.elapsed_ms(ev[0], ev[1]), ctx.elapsed_ms(ev[1], ev[2])
            for e in ev:
                ctx.event_destroy(e)
        return out


def check_n_best(n_best, L):
    n_best = int(n_best)
    if not 1 <= n_best <= 8 or n_best > L:
        raise ValueError("n_best / n_starts must be in 1..8 and at most the %d candidates" % L)
    return n_best


def select_starts(flat, M, n_starts, prior):
    """Among the ``n_starts`` retrievals of every pixel (rows m * n_starts + s of every array of ``flat``, the tuple a
    retrieval returns) the one of lowest ``F = cost + prior term``: ties go to the lower start, a non-finite F loses.
    Returns ``(results, start (M,) int32)``, every array of ``results`` gathered from the chosen starts."""
    X, cost = np.asarray(flat[0], dtype=np.float64), np.asarray(flat[1], dtype=np.float64)
    F = cost + _retrieve._prior_term(X, prior)
    F = np.where(np.isfinite(F), F, np.inf).reshape(M, n_starts)
    start = np.argmin(F, axis=1).astype(np.int32)            # (the first of equal minima)
    pick = np.arange(M) * n_starts + start
    return tuple(np.asarray(a)[pick] for a in flat), start


def multistart(first_guess, retrieve, obs_axis, obs, weights, n_starts, D, loop_args):
    """The multi-start retrieval both emulator types offer.  ``first_guess(prior, n_best) -> (X0, cost0, index)``
    ranks the candidates with the loop's shared prior; the ``M n_starts`` starting rows, clipped to ``bounds``, go
    through ONE call of ``retrieve(X0, obs, weights, **loop_args)`` with the row-shaped ``obs``, ``weights`` and
    ``next_prior`` repeated (``obs_axis``: the axis of ``obs`` / ``weights`` the rows lie along when they are 2-D);
    ``select_starts`` keeps one start per pixel.  Returns ``(results, start (M,) int32, cost0 (M, n_starts))``."""
    if loop_args.get("emulator_unc"):
        raise ValueError("emulator_unc is not offered with multi-start: the first guess ranks by the plain data term")
    if loop_args.get("step_fn") is not None:
        raise ValueError("step_fn is not offered with multi-start")
    prior = shared_prior(loop_args.get("prior"), D)
    X0, cost0, index = first_guess(prior, n_starts)
    M = index.shape[0]
    X0 = X0.reshape(M * n_starts, D)
    bounds = loop_args.get("bounds")
    if bounds is not None:
        X0 = np.clip(X0, np.asarray(bounds[0], dtype=np.float64).reshape(D), np.asarray(bounds[1], dtype=np.float64).reshape(D))
    obs, weights = np.asarray(obs), None if weights is None else np.asarray(weights)
    obs_r = np.repeat(obs, n_starts, axis=obs_axis) if obs.ndim == 2 else obs
    w_r = np.repeat(weights, n_starts, axis=obs_axis) if weights is not None and weights.ndim == 2 else weights
    args = dict(loop_args)
    if args.get("next_prior") is not None and np.ndim(args["next_prior"]) == 3:
        args["next_prior"] = np.repeat(np.asarray(args["next_prior"]), n_starts, axis=0)
    flat = retrieve(X0, obs_r, w_r, **args)
    results, start = select_starts(flat, M, n_starts, prior)
    return results, start, cost0.reshape(M, n_starts)
