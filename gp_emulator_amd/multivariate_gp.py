"""Host-side mirror of the reference's ``MultivariateEmulator`` (predict side).

gp_emulator/multivariate_gp.py:38-222: a multivariate model output (e.g. a 2101-band
spectrum) is compressed onto ``n_pcs`` principal components and each PC weight is emulated
by its own ``GaussianProcess`` on the shared training parameters ``y``.  This mirror keeps
the constructor, ``compress``, ``predict`` and ``dump_emulator`` with the reference's
argument names and return shapes, and loads the reference's ``.npz`` dumps (:68-79,
e.g. data/prosail_30_0_30_0.npz) with ``allow_pickle=False``.

With ``hyperparams`` (given or from ``dump``) every per-PC emulator is only set up
(``_set_params``, reference :185-186); without, each one is trained with
``learn_hyperparameters(n_tries)`` (:180-184).  ``is_gpu=True`` -- a keyword the reference's
constructor does not have -- does either on the GPU: all n_pcs inverses in ONE launch of the
likelihood kernel (they share the training inputs), or the GPU training objective.
"""
import numpy as np

from . import _lib
from .GaussianProcess import GaussianProcess

__all__ = ["MultivariateEmulator"]


class MultivariateEmulator(object):

    def __init__(self, dump=None, X=None, y=None, hyperparams=None, thresh=0.98, n_tries=5,
                 basis_functions=None, n_pcs=None, is_gpu=False):
        # reference :40-122; basis_functions / n_pcs: a stored decomposition (what
        # save_emulators.py:93-98 tries to pass), is_gpu: set up or train on the GPU
        if dump is not None:
            if X is None and y is None:
                with np.load(dump, allow_pickle=False) as f:
                    X = f["X"]
                    y = f["y"]
                    hyperparams = f["hyperparams"]
                    thresh = float(f["thresh"])
                    if "basis_functions" in f.files:
                        basis_functions = f["basis_functions"]
                        n_pcs = int(f["n_pcs"])
            else:
                raise ValueError("You specified both a dump file and X and y")
        else:
            if X is None or y is None:
                raise ValueError("Need to specify both X and y")
            assert X.shape[0] == y.shape[0]
            assert X.ndim == 2
            assert y.ndim == 2

        self.X_train = X
        self.y_train = y
        self.thresh = thresh
        if basis_functions is None:
            self.calculate_decomposition(X, thresh)
            basis_functions = self.basis_functions
            n_pcs = self.n_pcs
        self.n_pcs = int(n_pcs)
        self.basis_functions = basis_functions
        if hyperparams is not None:
            assert (y.shape[1] + 2 == hyperparams.shape[0]) and (self.n_pcs == hyperparams.shape[1])
        self.train_emulators(X, y, hyperparams=hyperparams, n_tries=n_tries, is_gpu=is_gpu)

    def dump_emulator(self, fname):
        """Save in the reference's .npz layout (reference :124-137)."""
        np.savez_compressed(fname, X=self.X_train, y=self.y_train, hyperparams=self.hyperparams,
                            thresh=self.thresh, basis_functions=self.basis_functions,
                            n_pcs=self.n_pcs)

    def calculate_decomposition(self, X, thresh):
        """PCA by SVD; keep the PCs whose cumulative singular-value share is <= thresh
        (reference :139-160)."""
        U, s, V = np.linalg.svd(X, full_matrices=True)
        pcnt_var_explained = s.cumsum() / s.sum()
        # the reference indexes V (N_full rows) with a mask of len(s) = min(N_train, N_full)
        # entries (:158), which old numpy tolerated; select among the first len(s) rows
        self.basis_functions = V[:s.size][pcnt_var_explained <= thresh]
        self.n_pcs = int(np.sum(pcnt_var_explained <= thresh))

    def train_emulators(self, X, y, hyperparams, n_tries=2, is_gpu=False):
        """One GaussianProcess per PC on the shared inputs (reference :162-188)."""
        self.emulators = []
        train_data = self.compress(X)
        self.hyperparams = np.zeros((2 + y.shape[1], self.n_pcs))
        for i in range(self.n_pcs):
            self.emulators.append(GaussianProcess(np.atleast_2d(y), train_data[i]))
        if hyperparams is None:
            if is_gpu and self.n_pcs > 1:
                # all PCs and restarts together (same starting points as the loop below would draw)
                from . import perband
                costs, thetas, _ = perband.learn_bands(self.emulators, n_tries=n_tries)
                self.hyperparams[:, :] = thetas.T
                return
            for i, gp in enumerate(self.emulators):
                self.hyperparams[:, i] = gp.learn_hyperparameters(n_tries=n_tries, is_gpu=is_gpu)[1]
            return
        self.hyperparams[:, :] = np.asarray(hyperparams)[:, :self.n_pcs]
        if is_gpu and self.n_pcs > 0:
            # the emulators differ in targets and theta only: one launch, one workgroup each
            cost, grad, invQ, invQt = _lib.default_context().likelihood_batch(
                self.hyperparams.T, np.atleast_2d(y), train_data, want_inverse=True)
            bad = np.flatnonzero(~np.isfinite(cost))
            if bad.size:
                # a pivot of the elimination was <= 0: what the host branch (_set_params ->
                # numpy's Cholesky, reference :66) reports as LinAlgError
                raise np.linalg.LinAlgError("Matrix is not positive definite (principal component %d)"
                                            % int(bad[0]))
            for i, gp in enumerate(self.emulators):
                gp.theta = self.hyperparams[:, i].copy()
                gp.invQ, gp.invQt = invQ[i], invQt[i]
                gp.current_theta, gp.current_loglikelihood = gp.theta, float(cost[i])
            return
        for i, gp in enumerate(self.emulators):
            gp._set_params(hyperparams[:, i])

    def compress(self, X):
        """Project full-rank vectors onto the PC basis (reference :190-193)."""
        return X.dot(self.basis_functions.T).T

    def predict(self, y, do_deriv=True, is_gpu=False):
        """Reconstructed output and its Jacobian at ONE input vector ``y`` (reference
        :195-222): ``fwd (N_full,)`` and ``deriv (N_params, N_full)``.  The numpy branch is the
        reference's loop over the per-PC emulators.  ``is_gpu=True`` -- the call an optimiser makes
        once per state vector -- runs on the device-resident form of the whole emulator
        (``predict_many`` on one row: all PCs in one launch, reconstruction and Jacobian on the
        device) instead of handing the flag to each per-PC ``predict`` as the reference does
        (:215): same numbers, one round trip instead of ``n_pcs``."""
        y = np.atleast_2d(y)
        if is_gpu:
            if y.shape[0] != 1:
                raise ValueError("predict takes one input vector; predict_many takes rows")
            if do_deriv:
                fwd, jac = self.predict_many(y, is_gpu=True, do_deriv=True)
                return fwd[0], jac[0]
            return self.predict_many(y, is_gpu=True)[0]
        fwd = np.zeros(self.basis_functions[0].shape[0])
        if do_deriv:
            deriv = np.zeros((y.shape[1], self.basis_functions.shape[1]))
        for i in range(self.n_pcs):
            pred_mu, pred_var, grad = self.emulators[i].predict(y)
            fwd += pred_mu * self.basis_functions[i]
            if do_deriv:
                deriv += np.asarray(grad).T @ np.atleast_2d(self.basis_functions[i])
        if do_deriv:
            return fwd.squeeze(), deriv
        return fwd.squeeze()

    # ---- the emulator resident on the device ----------------------------------------------------
    def _host_arrays(self):
        """Everything the device-resident copy is made from: every emulator's constants and the basis."""
        out = []
        for gp in self.emulators:
            out += [gp.theta, gp.inputs, gp.invQt, gp.invQ]
        out.append(self.basis_functions)
        return out

    def _gpu_state(self, dt):
        """The device-resident form of the whole emulator (packed per-PC emulators + basis), rebuilt whenever
        the host data is no longer what it was made from.  The reference uploads every constant on every call
        (gpu/predict.cu:11-34), so a caller may replace OR edit in place theta, invQ, invQt, inputs or the basis
        between two calls and the next call computes with the new values; so it is here: the state remembers the
        array objects (cheap pre-filter) and a 64-bit digest of all their bytes (``_lib.HostBlocks``), and the
        digest is re-taken on EVERY call -- inside the library call, while the device works and the calling
        thread would only wait (``gp_mv_predict_host_checked``), so the latency path pays nothing for it; a
        mismatch discards that call's results, rebuilds the state and calls again."""
        from . import perband
        cache = self.__dict__.setdefault("_gpu", {})
        key = (dt.str, _lib.default_device())
        arrays = self._host_arrays()
        st = cache.get(key)
        if st is not None and st["blocks"].same_arrays(arrays):
            return st
        if st is not None:
            self._release(st)
            del cache[key]
        blocks = _lib.HostBlocks(arrays)           # (digest first: what the batch below is packed from)
        batch = perband.make_batch(self.emulators, dt)
        ctx = batch.ctx
        st = {"blocks": blocks, "batch": batch, "ctx": ctx,
              "d_basis": ctx.to_device(np.ascontiguousarray(self.basis_functions, dtype=dt))}
        cache[key] = st
        return st

    @staticmethod
    def _release(st):
        st["ctx"].free(st["d_basis"])
        st["batch"].close()

    def _rebuilt_gpu_state(self, dt, st):
        """The host arrays were edited in place since the resident copy ``st`` was made: discard it and build the
        state again from what they hold now."""
        self._release(st)
        del self.__dict__["_gpu"][(dt.str, _lib.default_device())]
        return self._gpu_state(dt)

    def release_gpu(self):
        """Free the device-resident copy (packed emulators, basis); the next
        ``is_gpu=True`` call rebuilds it."""
        for st in self.__dict__.get("_gpu", {}).values():
            self._release(st)
        self.__dict__["_gpu"] = {}

    def __del__(self):
        try:
            self.release_gpu()
        except Exception:
            pass

    def predict_many(self, Y, is_gpu=True, precision=np.float64, do_deriv=False):
        """Beyond the reference (whose predict breaks for more than one row, SURVEY.md
        section 3.3): reconstructed outputs ``(M, N_full)`` -- and with ``do_deriv`` the
        Jacobians ``(M, N_params, N_full)`` -- for M input rows.  On the GPU the n_pcs
        emulators run as ONE batched launch over the shared rows and the reconstruction
        ``sum_pc mu_pc * basis_pc`` is a second kernel on the resident outputs; only the
        reconstructed arrays cross PCIe.  The packed emulators and the basis stay on the device
        between calls (``release_gpu()`` frees them), and a call is one library call
        (``gp_mv_predict_host``): rows up, three launches, results down."""
        Y = np.atleast_2d(Y)
        M, D = Y.shape
        B = self.basis_functions.shape[1]
        if not is_gpu:
            out = [gp.predict(Y) for gp in self.emulators]
            fwd = np.stack([o[0] for o in out]).T @ self.basis_functions
            if not do_deriv:
                return fwd
            grads = np.stack([o[2] for o in out])                  # (P, M, D)
            return fwd, np.einsum("pmd,pb->mdb", grads, self.basis_functions)
        dt = np.dtype(precision)
        st = self._gpu_state(dt)
        ctx = st["ctx"]
        isz = dt.itemsize
        Yc = np.ascontiguousarray(Y, dtype=dt)
        # one library call per <= 1 GiB of results (rows up, three launches, results down, one
        # synchronisation): a single call for anything an optimiser asks for
        step = max(1, (1 << 30) // (B * (1 + (D if do_deriv else 0)) * isz))
        if do_deriv and M <= step:                         # one call: fwd and jac back to back, one copy down
            both = ctx.out_pool.take((M * B * (1 + D),), dt)   # >= 1 MB: recycled memory (see _lib.OutputPool)
            fwd, jac = both[:M * B].reshape(M, B), both[M * B:].reshape(M, D, B)
        else:
            fwd = ctx.out_pool.take((M, B), dt)
            jac = ctx.out_pool.take((M, D, B), dt) if do_deriv else None

        def call(st, ctx, blocks, r0, r1):
            return ctx.lib.gp_mv_predict_host_checked(ctx.h, st["batch"].h, st["d_basis"], _lib._ptr(Yc[r0:r1]), r1 - r0, B,
                                                      _lib._ptr(fwd[r0:r1]), _lib._ptr(jac[r0:r1]) if do_deriv else None,
                                                      blocks.ptrs, blocks.lens, blocks.n, blocks.expected)
        self._checked_row_blocks(dt, st, M, step, "gp_mv_predict_host_checked", call)
        return (fwd, jac) if do_deriv else fwd

    def _checked_row_blocks(self, dt, st, M, step, name, call, unpack=None):
        """The M rows of a checked library call on the resident state ``st``, in blocks ``[r0, r1)`` of at most ``step``
        rows: ``call(st, ctx, blocks, r0, r1)`` makes the call with the state's host-array table ``blocks``, refreshed,
        and returns its status; ``unpack(r0, r1)`` then takes the block's results.  On ``GP_STALE`` -- the host arrays
        were edited in place -- the state is rebuilt and the same rows run again: nothing of the stale call is kept.
        Returns the state as it is after the last block."""
        r0 = 0
        while r0 < M:
            r1 = min(M, r0 + step)
            rc = call(st, st["ctx"], st["blocks"].refresh(), r0, r1)
            if rc == _lib.GP_STALE:
                st = self._rebuilt_gpu_state(dt, st)
                continue
            _lib.check(rc, name)
            if unpack is not None:
                unpack(r0, r1)
            r0 = r1
        return st

    # ---- observation misfit: the data term of a variational retrieval -------------------------------
    def _misfit_args(self, Y, obs, weights, gauss_newton):
        Y = np.atleast_2d(Y)
        M = Y.shape[0]
        B = self.basis_functions.shape[1]
        obs = np.asarray(obs)
        if obs.shape not in ((B,), (M, B)):
            raise ValueError("obs must be (%d,) or (%d, %d), got %s" % (B, M, B, obs.shape))
        if weights is not None:
            weights = np.asarray(weights)
            if weights.shape not in ((B,), (M, B)):
                raise ValueError("weights must be (%d,) or (%d, %d), got %s" % (B, M, B, weights.shape))
            if gauss_newton and weights.ndim == 2:
                raise ValueError("gauss_newton=True needs weights shared by all rows: None or (%d,)" % B)
        return Y, obs, weights

    def _gauss_newton_matrix(self, weights):
        """``basis diag(w) basis^T`` (P, P) in float64, formed once per call on the host."""
        b64 = np.ascontiguousarray(self.basis_functions, dtype=np.float64)
        return (b64 if weights is None else b64 * np.asarray(weights, dtype=np.float64)) @ b64.T

    def misfit(self, y, obs, weights=None, is_gpu=False, precision=np.float64, do_deriv=True, gauss_newton=False,
               return_coef=False, emulator_unc=False):
        """``misfit_many`` at ONE state vector ``y`` -- the call an optimiser makes per iteration: the scalar
        cost, then (when asked for) ``grad (N_params,)``, ``gn (N_params, N_params)`` and ``coef (n_pcs,)``."""
        y = np.atleast_2d(y)
        if y.shape[0] != 1:
            raise ValueError("misfit takes one input vector; misfit_many takes rows")
        B = self.basis_functions.shape[1]
        if np.shape(obs) != (B,) or (weights is not None and np.shape(weights) != (B,)):
            raise ValueError("obs and weights must be (%d,)" % B)
        more = dict(emulator_unc=True) if emulator_unc else {}
        out = self.misfit_many(y, obs, weights=weights, is_gpu=is_gpu, precision=precision, do_deriv=do_deriv,
                               gauss_newton=gauss_newton, return_coef=return_coef, **more)
        if isinstance(out, tuple):
            return tuple(o[0] for o in out)
        return out[0]

    # ---- the emulators' own variance in the data term -------------------------------------------------
    @staticmethod
    def _unc_term_numpy(J0, c, G, v, dmu, dv, do_deriv=True, gauss_newton=True):
        """The data term with the per-PC emulators' variance from the plain term's ``J0 (M,)`` and ``c = basis (w o r)
        (M, P)``, ``G = basis diag(w) basis^T`` (P, P) or per row (M, P, P) (the lower triangle is read), the per-PC
        variances ``v (P, M)`` and the gradients ``dmu``, ``dv`` ``(P, M, D)``, in float64 -- exactly the formulas of
        ``misfit_many(emulator_unc=True)``.  Returns ``(cost (M,), ceff (M, P), Geff (M, P, P), grad (M, D) or None, gn
        (M, D, D) or None)``; a row whose ``K`` has a pivot that is not > 0 or not finite is NaN throughout."""
        from . import _dense_numpy
        J0, c = np.asarray(J0, dtype=np.float64), np.asarray(c, dtype=np.float64)
        v, dmu, dv = (np.asarray(a, dtype=np.float64) for a in (v, dmu, dv))
        M, P = c.shape
        idx = np.arange(P)
        Gm = _dense_numpy._mirror_lower(np.array(np.broadcast_to(np.asarray(G, dtype=np.float64), (M, P, P))))
        with np.errstate(all="ignore"):
            clamp = v <= 0                                      # (False for a NaN v: it goes through every formula)
            s = np.sqrt(np.where(clamp, 0.0, v)).T              # (M, P)
            dvp = np.where(clamp[:, :, None], 0.0, dv)
            K = s[:, :, None] * Gm * s[:, None, :]
            K[:, idx, idx] += 1.0
            Kinv, status = _dense_numpy._cholesky_inverse_numpy(K)      # (K now holds L)
            Kinv = _dense_numpy._mirror_lower(Kinv)
            z = s * c
            a = np.einsum("mij,mj->mi", Kinv, z)
            cost = J0 - 0.5 * np.sum(z * a, axis=1) + np.sum(np.log(K[:, idx, idx]), axis=1)
            ceff = c - np.einsum("mij,mj->mi", Gm, s * a)
            SG = s[:, :, None] * Gm                             # diag(s) G
            Geff = _dense_numpy._mirror_lower(Gm - np.einsum("mki,mkl,mlj->mij", SG, Kinv, SG))
            h = 0.5 * (Geff[:, idx, idx] - ceff * ceff)
            grad = gn = None
            if do_deriv:
                grad = np.einsum("mp,pmd->md", ceff, dmu) + np.einsum("mp,pmd->md", h, dvp)
            if gauss_newton:
                gn = (MultivariateEmulator._contract_numpy(dmu, Geff)
                      + MultivariateEmulator._contract_numpy(dvp, 0.5 * Geff * Geff))
        bad = status != 0
        for out in (cost, ceff, Geff, grad, gn):
            if out is not None:
                out[bad] = np.nan
        return cost, ceff, Geff, grad, gn

    def _data_term_unc_numpy(self, Y, obs, weights, G, do_deriv=True, gauss_newton=True):
        """The numpy branch of ``emulator_unc=True``: ``(cost, grad, gn)`` (None where not asked for) in float64 from
        ``cpu_predict(do_unc=True)`` and ``variance_gradient(is_gpu=False)`` of the per-PC emulators, ``G`` as
        ``_unc_term_numpy`` takes it."""
        basis = np.asarray(self.basis_functions, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        with np.errstate(all="ignore"):
            mu, v, dmu = (np.stack(a) for a in zip(*[gp.cpu_predict(Y, do_unc=True) for gp in self.emulators]))
            dv = np.stack([gp.variance_gradient(Y, is_gpu=False)[1] for gp in self.emulators])
            r = mu.T @ basis - obs
            wr = r if weights is None else weights * r
            J0 = 0.5 * np.sum(wr * r, axis=1)
            c = wr @ basis.T
        cost, _, _, grad, gn = self._unc_term_numpy(J0, c, G, v, dmu, dv, do_deriv, gauss_newton)
        return cost, grad, gn

    def _misfit_unc_gpu(self, Y, obs, weights, dt, do_deriv, gauss_newton):
        """The device path of ``misfit_many(emulator_unc=True)``: ``[cost, grad or None, gn or None]`` in ``dt``."""
        M, D = Y.shape
        P, B = self.n_pcs, self.basis_functions.shape[1]
        isz = dt.itemsize
        st = self._fresh_gpu_state(dt)
        ctx, batch, d_basis = st["ctx"], st["batch"], st["d_basis"]
        with np.errstate(over="ignore"):                   # (a far row may be infinite in float32: it comes out NaN)
            Yc = np.ascontiguousarray(Y, dtype=dt)
        per_obs, per_w = obs.ndim == 2, weights is not None and weights.ndim == 2
        step = max(1, (1 << 30) // (max(B, P * D, D * D, P * P) * isz))        # at most 1 GiB per device array
        n0 = min(M, step)
        cost = np.empty(M, dt)
        grad = np.empty((M, D), dt) if do_deriv else None
        gn = np.empty((M, D, D), dt) if gauss_newton else None
        with _lib.Scratch(ctx, dt) as scratch:
            up, alloc = scratch.up, scratch.alloc
            d_y = alloc(n0 * D * isz)
            d_obs = alloc(n0 * B * isz) if per_obs else up(obs)
            d_w = alloc(n0 * B * isz) if per_w else up(weights)
            d_G = alloc(n0 * P * P * isz) if per_w else up(self._gauss_newton_matrix(weights))
            d_mu, d_der, d_var, d_dvar = [alloc(n0 * k * isz) for k in (P, P * D, P, P * D)]
            d_cost, d_coef = alloc(n0 * isz), alloc(n0 * P * isz)
            d_grad = alloc(n0 * D * isz) if do_deriv else None
            d_gn = alloc(n0 * D * D * isz) if gauss_newton else None
            for r0 in range(0, M, step):
                n = min(M, r0 + step) - r0
                ctx.h2d(d_y, Yc[r0:r0 + n])
                if per_obs:
                    ctx.h2d(d_obs, np.ascontiguousarray(obs[r0:r0 + n], dtype=dt))
                if per_w:
                    ctx.h2d(d_w, np.ascontiguousarray(weights[r0:r0 + n], dtype=dt))
                batch.predict_mean_grad_device(d_y, d_mu, d_der, n)
                batch.predict_var_grad_device(d_y, d_var, d_dvar, n)
                ctx.mv_misfit_device(dt, d_basis, d_mu, d_der, d_obs, B if per_obs else 0, d_w, B if per_w else 0, d_cost,
                                     d_coef, None, n, P, B, D)
                if per_w:
                    ctx.mv_weight_gram_device(dt, d_basis, d_w, B, d_G, n, P, B)
                ctx.mv_misfit_unc_device(dt, d_cost, d_coef, d_G, P * P if per_w else 0, d_var, d_der, d_dvar, d_cost,
                                         d_grad, d_gn, n, P, D)
                cost[r0:r0 + n] = ctx.to_host(d_cost, (n,), dt)
                if do_deriv:
                    grad[r0:r0 + n] = ctx.to_host(d_grad, (n, D), dt)
                if gauss_newton:
                    gn[r0:r0 + n] = ctx.to_host(d_gn, (n, D, D), dt)
        return [cost, grad, gn]

    def misfit_many(self, Y, obs, weights=None, is_gpu=True, precision=np.float64, do_deriv=True, gauss_newton=False,
                    return_coef=False, emulator_unc=False):
        """Observation misfit ``J(y) = 1/2 sum_b w_b (f_b(y) - obs_b)^2`` of the reconstructed output ``f`` for M
        input rows: ``cost (M,)`` and then, in this order and when asked for, its gradient ``grad (M, N_params)``
        (``do_deriv``) ``= Jac (w * r)`` with ``r = f - obs``, the Gauss-Newton term ``gn (M, N_params, N_params)
        = Jac diag(w) Jac^T`` (``gauss_newton``; weights shared by all rows) and ``coef (M, n_pcs)``
        (``return_coef``) ``= basis (w * r)``, which ``hessian_many(Y, coef=coef)`` turns into the curvature term:
        ``gn + hessian_many(Y, coef=coef)`` is the full second-order data term.  ``obs`` is ``(N_full,)`` or
        ``(M, N_full)``; ``weights`` None (all 1), ``(N_full,)`` or ``(M, N_full)``.  A weight of exactly 0 (as rounded
        to the call's ``precision`` on the GPU, in float64 on the numpy branch) masks its band whatever ``obs`` holds
        there: 0 is selected into ``obs`` before the upload and before the numpy data term, which multiply by the
        weight and do not select; a NaN or an infinity in ``obs`` under a non-zero weight, or in a weight, makes the
        row's results NaN.  Not in the reference, whose caller contracts ``predict``'s Jacobian on the host.

        Nothing of size ``N_params x N_full`` is formed: ``coef[p] = sum_b basis[p, b] w_b r_b`` and ``grad[d] =
        sum_p coef[p] dmu_p/dy_d``.  The numpy branch states exactly that on the per-PC ``gp.predict`` outputs.  On
        the GPU a call is one library call (``gp_mv_misfit_host_checked``) on the device-resident emulator: rows,
        observations and weights up, the mean+gradient predict, the misfit kernel, ``1 + N_params + n_pcs``
        numbers per row down.

        ``emulator_unc=True`` adds the per-PC emulators' own predictive variances ``v_p(y)`` to the data term.  The
        PCs are shared by all bands, so the emulator's error is correlated across the spectrum with rank ``n_pcs``:
        ``obs = basis^T mu + eps``, ``eps ~ N(0, C)``, ``C = diag(1 / w) + basis^T diag(vp) basis``, and the term is
        the exact Gaussian one, ``cost = 1/2 r^T C^-1 r + 1/2 log det(C diag(w))`` (>= 0 up to rounding).  With ``J0``,
        ``c = basis (w * r)`` and ``G = basis diag(w) basis^T`` of the plain term, ``dmu`` and ``dv`` the gradients of the
        per-PC means and variances:

            vp = v if v > 0 else 0,  dvp = dv if v > 0 else 0  (a NaN v stays NaN),  s = sqrt(vp)
            K = I + diag(s) G diag(s) = L L^T,  z = s * c,  a = K^-1 z
            cost = J0 - 1/2 z^T a + sum_p log L_pp
            ceff = c - G (s * a),  Geff = G - (G diag(s)) K^-1 (diag(s) G),  h_p = 1/2 (Geff_pp - ceff_p^2)
            grad[d]  = sum_p ceff_p dmu[p][d] + sum_p h_p dvp[p][d]
            gn[d][e] = sum_pq dmu[p][d] Geff_pq dmu[q][e] + 1/2 sum_pq dvp[p][d] Geff_pq^2 dvp[q][e]

        ``gn`` is then the Fisher information matrix (positive semi-definite) and is offered with per-row weights too;
        the returns are ``cost``, then ``grad`` (``do_deriv``), then ``gn`` (``gauss_newton``).  ``return_coef=True``
        raises ``ValueError``: the full second order would need the Hessian of the variance.  A PC whose variance is
        not > 0 drops out exactly, and a row where that holds for every PC is the plain term's.  On the GPU, in row
        blocks on the device-resident emulator: rows, observations and weights up, ``predict_mean_grad_device``,
        ``predict_var_grad_device``, ``mv_misfit_device`` (``J0`` and ``c``), ``G`` from ``mv_weight_gram_device`` (per-row
        weights) or the host's matrix uploaded once, ``mv_misfit_unc_device``, results down.  ``is_gpu=False`` is the
        explicit float64 numpy branch of the same formulas from ``cpu_predict(do_unc=True)`` and
        ``variance_gradient(is_gpu=False)``; never a fallback.  With ``False`` nothing changes."""
        from . import _first_guess
        if emulator_unc and return_coef:
            raise ValueError("return_coef=True needs the Hessian of the variance: not available with emulator_unc=True")
        Y, obs, weights = self._misfit_args(Y, obs, weights, gauss_newton and not emulator_unc)
        obs = _first_guess.mask_obs(obs, weights, precision if is_gpu else np.float64)
        M, D = Y.shape
        P, B = self.n_pcs, self.basis_functions.shape[1]
        if emulator_unc:
            per_w = weights is not None and weights.ndim == 2
            if not is_gpu:
                w64 = None if weights is None else np.asarray(weights, dtype=np.float64)
                G = self.weight_gram(w64, is_gpu=False) if per_w else self._gauss_newton_matrix(w64)
                res = self._data_term_unc_numpy(Y, np.asarray(obs, dtype=np.float64), w64, G, do_deriv, gauss_newton)
            else:
                res = self._misfit_unc_gpu(Y, obs, weights, np.dtype(precision), do_deriv, gauss_newton)
            res = [a for a in res if a is not None]
            return tuple(res) if len(res) > 1 else res[0]
        A = self._gauss_newton_matrix(weights) if gauss_newton else None
        if not is_gpu:
            cost, coef, _, grad, gn = self._data_term_numpy(Y, obs, weights, do_deriv, A)
            res = [cost] + [a for a, asked in ((grad, do_deriv), (gn, gauss_newton), (coef, return_coef)) if asked]
            return tuple(res) if len(res) > 1 else cost
        dt = np.dtype(precision)
        isz = dt.itemsize
        st = self._gpu_state(dt)
        Yc = np.ascontiguousarray(Y, dtype=dt)
        obs_c = np.ascontiguousarray(obs, dtype=dt)
        w_c = None if weights is None else np.ascontiguousarray(weights, dtype=dt)
        A_c = None if A is None else np.ascontiguousarray(A, dtype=dt)
        per_obs, per_w = obs_c.ndim == 2, w_c is not None and w_c.ndim == 2
        # rows per library call: at most 1 GiB of per-row observations and weights up, 1 GiB of results down
        n_row = 1 + D + P + (D * D if gauss_newton else 0)
        step = (1 << 30) // (n_row * isz)
        if per_obs or per_w:
            step = min(step, (1 << 30) // ((per_obs + per_w) * B * isz))
        step = max(1, step)
        cost = np.empty(M, dt)
        grad = np.empty((M, D), dt)
        coef = np.empty((M, P), dt)
        gn = np.empty((M, D, D), dt) if gauss_newton else None
        buf = np.empty(min(M, step) * n_row, dt)

        def call(st, ctx, blocks, r0, r1):
            return ctx.lib.gp_mv_misfit_host_checked(
                ctx.h, st["batch"].h, st["d_basis"], _lib._ptr(Yc[r0:r1]), D,
                _lib._ptr(obs_c[r0:r1] if per_obs else obs_c), B if per_obs else 0,
                None if w_c is None else _lib._ptr(w_c[r0:r1] if per_w else w_c), B if per_w else 0,
                None if A_c is None else _lib._ptr(A_c), r1 - r0, B, _lib._ptr(buf),
                blocks.ptrs, blocks.lens, blocks.n, blocks.expected)

        def unpack(r0, r1):
            n = r1 - r0
            cost[r0:r1] = buf[:n]
            grad[r0:r1] = buf[n:n * (1 + D)].reshape(n, D)
            coef[r0:r1] = buf[n * (1 + D):n * (1 + D + P)].reshape(P, n).T
            if gauss_newton:
                gn[r0:r1] = buf[n * (1 + D + P):n * n_row].reshape(n, D, D)
        self._checked_row_blocks(dt, st, M, step, "gp_mv_misfit_host_checked", call, unpack)
        res = [cost]
        if do_deriv:
            res.append(grad)
        if gauss_newton:
            res.append(gn)
        if return_coef:
            res.append(coef)
        return tuple(res) if len(res) > 1 else cost

    # ---- per-row weights and the retrieval ---------------------------------------------------------
    def _fresh_gpu_state(self, dt):
        """``_gpu_state`` under the staleness contract of ``hessian_many``: the host arrays are digested before use
        and the resident copy rebuilt when they were edited in place."""
        st = self._gpu_state(dt)
        return st if st["blocks"].unchanged() else self._rebuilt_gpu_state(dt, st)

    def weight_gram(self, weights, is_gpu=True, precision=np.float64):
        """``G[m] = basis diag(weights[m]) basis^T``, ``(M, n_pcs, n_pcs)`` for weights ``(M, N_full)``: the matrix of
        the Gauss-Newton term of row m when the weights (per-pixel uncertainties, masks) differ from row to row.  It
        depends on the weights and the basis only, not on the state.  The numpy branch is, row by row,
        ``(basis * weights[m]) @ basis.T`` in float64 -- row by row for the reason ``hessian_many`` gives: a row's
        result must not depend on M.  On the GPU it is ``weight_gram_kernel`` on the device-resident basis (weights
        up, matrices down), every ``G[m]`` symmetric bit for bit."""
        weights = np.asarray(weights)
        P, B = self.n_pcs, self.basis_functions.shape[1]
        if weights.ndim != 2 or weights.shape[1] != B:
            raise ValueError("weights must be (n_rows, %d), got %s" % (B, weights.shape))
        M = weights.shape[0]
        if not is_gpu:
            b64 = np.ascontiguousarray(self.basis_functions, dtype=np.float64)
            w64 = np.asarray(weights, dtype=np.float64)
            return np.stack([(b64 * w64[m]) @ b64.T for m in range(M)]) if M else np.zeros((0, P, P))
        dt = np.dtype(precision)
        isz = dt.itemsize
        st = self._fresh_gpu_state(dt)
        ctx = st["ctx"]
        out = np.empty((M, P, P), dt)
        step = max(1, (1 << 30) // (B * isz))                  # at most 1 GiB of weights on the device
        with _lib.Scratch(ctx, dt) as scratch:
            d_w, d_g = scratch.alloc(min(M, step) * B * isz), scratch.alloc(min(M, step) * P * P * isz)
            for r0 in range(0, M, step):
                n = min(M, r0 + step) - r0
                ctx.h2d(d_w, np.ascontiguousarray(weights[r0:r0 + n], dtype=dt))
                ctx.mv_weight_gram_device(dt, st["d_basis"], d_w, B, d_g, n, P, B)
                out[r0:r0 + n] = ctx.to_host(d_g, (n, P, P), dt)
        return out

    @staticmethod
    def _contract_numpy(grads, G):
        """``gn[m] = grads[:, m].T @ G[m] @ grads[:, m]`` for ``G`` (M, P, P), or (P, P) shared by the rows; the upper
        triangle mirrored: exactly symmetric."""
        gn = np.triu(np.einsum("pmd,mpq,qme->mde" if G.ndim == 3 else "pmd,pq,qme->mde", grads, G, grads))
        return gn + np.swapaxes(np.triu(gn, 1), 1, 2)

    def gauss_newton_many(self, Y, weights=None, is_gpu=True, precision=np.float64):
        """The Gauss-Newton term ``gn (M, N_params, N_params) = Jac diag(w) Jac^T`` of the observation misfit for M
        input rows, exactly symmetric; ``weights`` None (all 1), ``(N_full,)`` or ``(M, N_full)``.  For None and shared
        weights it is ``misfit_many(..., gauss_newton=True)``'s ``gn``, bit for bit, on both branches.  For per-row
        weights, which ``misfit_many`` does not take, ``gn[m] = dmu[:, m].T @ G[m] @ dmu[:, m]`` with ``G =
        weight_gram(weights)``: on the GPU rows and weights up, the mean+gradient predict, the Gram kernel, the
        strided contraction (``gp_mv_gauss_newton_rows_device``), ``gn`` down, on the device-resident emulator under
        the staleness contract of ``hessian_many``; the numpy branch is ``einsum("pmd,mpq,qme->mde")`` on the per-PC
        ``gp.predict`` gradients and ``weight_gram``'s numpy result, the upper triangle mirrored."""
        Y = np.atleast_2d(Y)
        M, D = Y.shape
        P, B = self.n_pcs, self.basis_functions.shape[1]
        if weights is None or np.ndim(weights) == 1:
            return self.misfit_many(Y, np.zeros(B), weights=weights, is_gpu=is_gpu, precision=precision,
                                    do_deriv=False, gauss_newton=True)[1]
        weights = np.asarray(weights)
        if weights.shape != (M, B):
            raise ValueError("weights must be (%d,) or (%d, %d), got %s" % (B, M, B, weights.shape))
        if not is_gpu:
            grads = np.stack([gp.predict(Y)[2] for gp in self.emulators])      # (P, M, D)
            return self._contract_numpy(grads, self.weight_gram(weights, is_gpu=False))
        dt = np.dtype(precision)
        isz = dt.itemsize
        st = self._fresh_gpu_state(dt)
        ctx, batch = st["ctx"], st["batch"]
        Yc = np.ascontiguousarray(Y, dtype=dt)
        out = np.empty((M, D, D), dt)
        step = max(1, (1 << 30) // (max(B, P * D, D * D) * isz))      # at most 1 GiB per device array
        n0 = min(M, step)
        with _lib.Scratch(ctx, dt) as scratch:
            d_y, d_w, d_mu, d_der, d_g, d_gn = [scratch.alloc(n0 * k * isz) for k in (D, B, P, P * D, P * P, D * D)]
            for r0 in range(0, M, step):
                n = min(M, r0 + step) - r0
                ctx.h2d(d_y, Yc[r0:r0 + n])
                ctx.h2d(d_w, np.ascontiguousarray(weights[r0:r0 + n], dtype=dt))
                batch.predict_mean_grad_device(d_y, d_mu, d_der, n)
                ctx.mv_weight_gram_device(dt, st["d_basis"], d_w, B, d_g, n, P, B)
                ctx.mv_gauss_newton_rows_device(dt, d_der, d_g, P * P, d_gn, n, P, D)
                out[r0:r0 + n] = ctx.to_host(d_gn, (n, D, D), dt)
        return out

    def _data_term_numpy(self, Y, obs, weights, do_deriv=True, G=None):
        """The numpy branches' data term from ONE pass over the per-PC emulators' ``gp.predict``: ``cost (M,)``, ``coef
        (M, P)``, the per-PC gradients ``grads (P, M, D)``, then ``grad (M, D)`` with ``do_deriv`` and ``gn (M, D, D)``
        with ``G`` -- the (P, P) matrix of shared weights or ``weight_gram``'s (M, P, P) -- else None."""
        basis = np.asarray(self.basis_functions, dtype=np.float64)
        out = [gp.predict(Y) for gp in self.emulators]
        mu = np.stack([o[0] for o in out])                      # (P, M)
        grads = np.stack([o[2] for o in out])                   # (P, M, D)
        r = mu.T @ basis - obs
        wr = r if weights is None else weights * r
        cost = 0.5 * np.sum(wr * r, axis=1)
        coef = wr @ basis.T                                      # (M, P)
        grad = np.einsum("mp,pmd->md", coef, grads) if do_deriv else None
        return cost, coef, grads, grad, None if G is None else self._contract_numpy(grads, G)

    def retrieve_many(self, Y0, obs, weights=None, prior=None, bounds=None, lam0=1e-2, max_iter=20, down=1.0 / 3.0,
                      up=4.0, ftol=1e-10, xtol=0.0, is_gpu=True, precision=np.float64, return_cov=False, next_prior=None,
                      return_A=False, emulator_unc=False, bounds_mode="clamp", return_active=False):
        """Levenberg-Marquardt retrieval of M state vectors at once on this emulator: minimises, row by row,

            F(y) = 1/2 sum_b w_b (f_b(y) - obs_b)^2  (+ 1/2 (y - y0)^T P (y - y0) with ``prior=(y0 (D,), P (D, D))``)

        from ``Y0`` (M, D), inside ``bounds=(lo (D,), hi (D,))`` when given.  ``obs`` is ``(N_full,)`` or
        ``(M, N_full)``; ``weights`` None (all 1), ``(N_full,)`` or ``(M, N_full)`` -- per-row weights are per-pixel
        uncertainties and masks: weight 0 marks a missing or contaminated band, and a weight of exactly 0 masks its band
        whatever ``obs`` holds there (NaN or a fill value); a row with a NaN or an infinity in ``obs`` under a non-zero
        weight, in a weight or in ``Y0`` is never accepted and comes back as it went in ("Invalid pixels in
        the retrievals").  The loop, its arguments and what it
        returns are ``perband.retrieve_bands``': an iteration is the misfit at the trial rows, the accept / reject
        update (a trial that lowers F is taken and lambda multiplied by ``down``, any other is dropped and lambda
        multiplied by ``up``, between ``perband.LAMBDA_MIN`` and ``LAMBDA_MAX``; a row whose accepted step gains no
        more than ``ftol * F`` or moves no more than ``xtol`` is converged and frozen), then the damped Newton step
        ``(A + P + lambda diag(A + P)) step = -(grad + P (y - y0))``, ``trial = clip(y + step)``.  At most ``max_iter``
        trials per row.  ``A`` is the Gauss-Newton term ``Jac diag(w) Jac^T`` (``gauss_newton_many``) ONLY: the full
        second-order matrix (``hessian_many(coef=)`` added to it) is not offered here.

        Returns ``(Y (M, D), cost (M,), state (M,) int32, n_accepted (M,) int32, lam (M,))``: ``cost`` is the DATA term
        at ``Y`` (the prior term is not included), ``state`` 1 for converged rows, ``n_accepted`` the trials taken.
        ``return_cov=True`` appends ``cov (M, D, D)``, ``sigma (M, D)`` and ``cov_status (M,) int32``, the posterior
        covariance ``(A + P)^-1`` at the returned rows exactly as ``retrieve_bands`` defines it; the five are
        unchanged by it.

        On the GPU ``Y0``, ``obs`` and ``weights`` go up once to the device-resident emulator; with per-row weights one
        launch of the Gram kernel forms every row's ``basis diag(w) basis^T`` before the loop (it does not depend on
        the state).  Every iteration is ``predict_mean_grad_device``, ``mv_misfit_device``, the Gauss-Newton
        contraction (``mv_gauss_newton_device`` with the host's matrix, or ``mv_gauss_newton_rows_device`` with the
        per-row ones), ``lm_update_device`` and ``newton_step_device`` on the one stream, and nothing comes back
        inside the loop but ``state``, every fourth iteration, to stop when every row has converged; after it,
        ``posterior_cov_device`` on the loop's own arrays.  ``is_gpu=False`` is the explicit numpy branch, the same loop
        from the numpy forms of ``misfit_many`` / ``gauss_newton_many`` and ``_lib.newton_step_numpy``; never a
        fallback.

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

        ``return_A=True`` appends, as the last element, the loop's final data-term matrix ``A (M, D, D)`` (the
        Gauss-Newton term whose ``(A + P)^-1`` is ``cov``), as ``retrieve_bands`` does.  With ``False`` nothing changes.

        ``emulator_unc=True`` minimises the data term of ``misfit_many(emulator_unc=True)`` instead: the per-PC emulators'
        predictive variances enter the observation's covariance with their rank-``n_pcs`` correlation across the bands, and
        ``A`` is that term's Fisher matrix, so ``cov``, ``sigma``, ``next_prec`` and the returned ``A`` include the
        emulators' share of the error.  On the GPU an iteration is then ``predict_mean_grad_device``,
        ``predict_var_grad_device``, ``mv_misfit_device`` (cost and ``basis (w * r)``, no gradient) and
        ``mv_misfit_unc_device`` with the matrix formed once before the loop, then the same update and step; the numpy
        branch hands the loop the numpy form of that term.  With ``False`` nothing changes.

        ``bounds_mode="active_set"`` (default "clamp": nothing changes) replaces the clamped step by the exact minimiser of
        the damped model inside the box, and ``return_active=True`` appends ``active (M, D) int8`` and ``kkt (M,)`` behind
        everything else; both need ``bounds`` and are ``retrieve_bands``' arguments word for word."""
        from . import _first_guess, _retrieve
        _retrieve.check_bounds_mode(bounds_mode, bounds, return_active)
        Y0 = np.asarray(Y0)
        if Y0.ndim != 2:
            raise ValueError("Y0 must be (n_rows, n_inputs)")
        M, D = Y0.shape
        P, B = self.n_pcs, self.basis_functions.shape[1]
        if D != self.emulators[0].inputs.shape[1]:
            raise ValueError("Y0 has %d columns, the emulators have %d inputs" % (D, self.emulators[0].inputs.shape[1]))
        _, obs, weights = self._misfit_args(Y0, obs, weights, False)
        obs = _first_guess.mask_obs(obs, weights, precision if is_gpu else np.float64)
        prior, bounds = _retrieve.prior_and_bounds(prior, bounds, D, M)
        max_iter = int(max_iter)

        if not is_gpu:
            step = _retrieve.numpy_step(prior, bounds, bounds_mode)
            return _retrieve.lm_numpy(self._retrieval_term_numpy(obs, weights, emulator_unc), step, Y0, lam0, max_iter, down,
                                      up, ftol, xtol, prior, return_cov, next_prior, return_A,
                                      bounds if return_active else None)

        dt = np.dtype(precision)
        st = self._fresh_gpu_state(dt)
        with _retrieve.Scratch(st["ctx"], dt) as scratch:
            misfit = self._retrieval_term_device(scratch, st, obs, weights, M, D, emulator_unc)
            return _retrieve.lm_device(scratch, M, D, Y0, lam0, prior, bounds, max_iter, down, up, ftol, xtol, return_cov,
                                       misfit, next_prior, return_A, bounds_mode, return_active)

    def _retrieval_term_numpy(self, obs, weights, emulator_unc):
        """The data term of the retrievals on the host: ``X (R, D) -> (cost, grad, A)`` for ``obs`` and ``weights`` as
        ``_misfit_args`` returns them for those R rows; the weights' matrix is formed once."""
        per_row = weights is not None and weights.ndim == 2
        obs64 = np.asarray(obs, dtype=np.float64)
        w64 = None if weights is None else np.asarray(weights, dtype=np.float64)
        G = self.weight_gram(w64, is_gpu=False) if per_row else self._gauss_newton_matrix(w64)

        def data_term(X):
            if emulator_unc:
                return self._data_term_unc_numpy(X, obs64, w64, G)
            cost, _, _, grad, gn = self._data_term_numpy(X, obs64, w64, True, G)
            return cost, grad, gn
        return data_term

    def _retrieval_term_device(self, scratch, st, obs, weights, M, D, emulator_unc):
        """The data term of the retrievals on the device, for the ``M`` rows ``obs`` and ``weights`` are given for: they
        go up once into ``scratch`` (on the resident emulator ``st``), with per-row weights one launch of the Gram kernel
        forms every row's matrix; ``misfit(d_rows, d_cost, d_grad, d_A)`` enqueues the term on those rows."""
        ctx, batch, d_basis = st["ctx"], st["batch"], st["d_basis"]
        dt = scratch.dt
        isz = dt.itemsize
        P, B = self.n_pcs, self.basis_functions.shape[1]
        per_row = weights is not None and weights.ndim == 2
        d_obs = scratch.up(obs)
        d_w = scratch.up(weights) if weights is not None else None
        d_mu, d_der = scratch.alloc(P * M * isz), scratch.alloc(P * M * D * isz)
        os_, ws = B if obs.ndim == 2 else 0, B if per_row else 0
        if per_row:                                # every row's matrix, once: it does not depend on the state
            d_G = scratch.alloc(M * P * P * isz)
            ctx.mv_weight_gram_device(dt, d_basis, d_w, B, d_G, M, P, B)
        else:
            d_G = scratch.up(self._gauss_newton_matrix(weights))
        if emulator_unc:
            d_var, d_dvar, d_coef = scratch.alloc(P * M * isz), scratch.alloc(P * M * D * isz), scratch.alloc(P * M * isz)

        def misfit_unc(d_rows, c, g, a):
            batch.predict_mean_grad_device(d_rows, d_mu, d_der, M)
            batch.predict_var_grad_device(d_rows, d_var, d_dvar, M)
            ctx.mv_misfit_device(dt, d_basis, d_mu, d_der, d_obs, os_, d_w, ws, c, d_coef, None, M, P, B, D)
            ctx.mv_misfit_unc_device(dt, c, d_coef, d_G, P * P if per_row else 0, d_var, d_der, d_dvar, c, g, a, M, P, D)

        def misfit(d_rows, c, g, a):
            batch.predict_mean_grad_device(d_rows, d_mu, d_der, M)
            ctx.mv_misfit_device(dt, d_basis, d_mu, d_der, d_obs, os_, d_w, ws, c, None, g, M, P, B, D)
            if per_row:
                ctx.mv_gauss_newton_rows_device(dt, d_der, d_G, P * P, a, M, P, D)
            else:
                ctx.mv_gauss_newton_device(dt, d_der, d_G, a, M, P, D)
        return misfit_unc if emulator_unc else misfit

    def retrieve_joint(self, Y0, obs, weights, prior, noise, bounds=None, lam0=1e-2, max_iter=20, down=1.0 / 3.0, up=4.0,
                       ftol=1e-10, xtol=0.0, is_gpu=True, precision=np.float64, return_cov=False, emulator_unc=False,
                       second_order="gauss_newton", work_budget=None, bounds_mode="clamp"):
        """Joint maximum a posteriori retrieval of M trajectories of T dates on this emulator: what
        ``perband.retrieve_bands_joint`` is to ``retrieve_bands`` (the objective, the loop, the keywords, the returned
        ``(Y (T, M, D), sigma (T, M, D), cost (T, M), F (M,), state, n_accepted, lam, cov_status)`` and ``cov (T, M, D,
        D)`` with ``return_cov=True``, the positive definite ``noise`` it needs, the invalid pixels), with the data term
        of ``retrieve_many`` on every date.  ``obs`` is (T, N_full) or (T, M, N_full), ``weights`` None, (N_full,) for
        every date and pixel, (T, N_full) or (T, M, N_full); ``Y0`` (T, M, D), or (M, D) taken for every date; ``prior`` is
        date 0's, required.  One data-term call runs on the T M rows of all dates; with anything but one weight vector
        for all of them the per-row Gram matrices are formed for those rows, once.  ``second_order`` is "gauss_newton"
        only.  ``is_gpu=False`` is the explicit numpy branch; never a fallback.  ``bounds_mode`` is "clamp"
        only (``ValueError`` otherwise): the box step has no block-tridiagonal form yet."""
        from . import _first_guess, _retrieve
        _retrieve.clamp_only(bounds_mode)
        if second_order != "gauss_newton":
            raise ValueError("the joint retrieval needs second_order='gauss_newton': the Hessian of F must stay positive definite")
        if prior is None:
            raise ValueError("a joint retrieval needs a prior")
        obs = np.asarray(obs)
        T = len(obs)
        if T == 0:
            raise ValueError("obs has no dates")
        Y0 = _retrieve.joint_start(Y0, T, "Y0")
        M, D = Y0.shape[1:]
        B = self.basis_functions.shape[1]
        if D != self.emulators[0].inputs.shape[1]:
            raise ValueError("Y0 has %d columns, the emulators have %d inputs" % (D, self.emulators[0].inputs.shape[1]))

        def rows(a, name):             # per date (N_full,) or (M, N_full): (T, M, N_full)
            a = np.asarray(a, dtype=np.float64)
            if a.shape not in ((T, B), (T, M, B)):
                raise ValueError("%s must be (%d, %d) or (%d, %d, %d), got %s" % (name, T, B, T, M, B, a.shape))
            return np.broadcast_to(a[:, None, :] if a.ndim == 2 else a, (T, M, B))
        obs = rows(obs, "obs")
        if weights is not None and np.ndim(weights) != 1:
            weights = rows(weights, "weights")
        flat = Y0.reshape(T * M, D)
        _, obs_f, w_f = self._misfit_args(flat, np.ascontiguousarray(obs.reshape(T * M, B)),
                                          weights if weights is None or np.ndim(weights) == 1 else
                                          np.ascontiguousarray(weights.reshape(T * M, B)), False)
        obs_f = _first_guess.mask_obs(obs_f, w_f, precision if is_gpu else np.float64)
        loop = (bounds, lam0, max_iter, down, up, ftol, xtol, return_cov)

        def cut(a, m0, m1):            # the pixels m0 .. m1 of every date of a (T M, N_full) array
            if a is None or a.ndim == 1:
                return a
            return np.ascontiguousarray(a.reshape(T, M, B)[:, m0:m1].reshape(T * (m1 - m0), B))
        if not is_gpu:
            def numpy_term(m0, m1):
                return self._retrieval_term_numpy(cut(obs_f, m0, m1), cut(w_f, m0, m1), emulator_unc)
            return _retrieve.retrieve_joint(Y0, prior, noise, *loop, numpy_term=numpy_term)
        dt = np.dtype(precision)
        st = self._fresh_gpu_state(dt)

        def device_term(scratch, m0, m1):
            return self._retrieval_term_device(scratch, st, cut(obs_f, m0, m1), cut(w_f, m0, m1), T * (m1 - m0), D, emulator_unc)
        return _retrieve.retrieve_joint(Y0, prior, noise, *loop, device_term=device_term, context=st["ctx"], precision=precision,
                                        work_budget=work_budget)

    # ---- the first guess: look-up-table search in band space --------------------------------------
    def candidate_table(self, candidates, precision=np.float64, space="band"):
        """The device table of ``first_guess_many``: the spectra of the ``candidates`` (L, D), row-major
        ``(L, N_full)``, from ``predict_mean_grad_device`` and ``gp_reconstruct_device`` on the resident emulator; it
        never crosses PCIe.  A context manager (``_first_guess.DeviceTable``): pass it as ``table=`` so that repeated
        calls (dates, tiles) do not compute the spectra again; leaving the block frees it.  ``space="pc"`` keeps only
        the ``(n_pcs, L)`` per-PC means, PC-major as ``predict_mean_grad_device`` writes them, for
        ``first_guess_many(space="pc")``: nothing is reconstructed, and the table is ``N_full / n_pcs`` times smaller."""
        from . import _first_guess
        if space not in ("band", "pc"):
            raise ValueError("space must be 'band' or 'pc'")
        dt = _lib.precision_dtype(precision)
        cand = _first_guess.check_candidates(candidates, self.emulators[0].inputs.shape[1])
        st = self._fresh_gpu_state(dt)
        ctx, batch, d_basis = st["ctx"], st["batch"], st["d_basis"]
        P, B, (L, D) = self.n_pcs, self.basis_functions.shape[1], cand.shape
        if space == "pc" and P > _lib.lut_pc_max_pcs:
            raise ValueError("the PC-space search serves n_pcs <= %d" % _lib.lut_pc_max_pcs)
        d_table = ctx.malloc(L * (B if space == "band" else P) * dt.itemsize)
        try:
            with _lib.Scratch(ctx, dt) as scratch:
                d_mu = scratch.alloc(P * L * dt.itemsize) if space == "band" else d_table
                batch.predict_mean_grad_device(scratch.up(cand), d_mu, scratch.alloc(P * L * D * dt.itemsize), L)
                if space == "band":
                    ctx.reconstruct_device(dt, d_basis, d_mu, d_table, L, P, B)
                ctx.synchronize()
        except Exception:
            ctx.free(d_table)
            raise
        if space == "pc":
            return _first_guess.DeviceTable(ctx, dt, d_table, (L, 1), P, cand, self, space="pc")
        return _first_guess.DeviceTable(ctx, dt, d_table, (1, B), B, cand, self)

    def first_guess_many(self, candidates, obs, weights=None, prior=None, n_best=1, is_gpu=True, precision=np.float64,
                         table=None, space="band"):
        """The starting states of ``retrieve_many`` by look-up-table search in band space: among the ``candidates``
        (L, D) per row the ``n_best`` (1..8) of lowest

            J[m, l] = a[l] + 1/2 sum_b w[m, b] (f_b(c_l) - obs[m, b])^2,     a[l] = 1/2 (c_l - y0)^T P (c_l - y0)

        with ``obs`` ``(N_full,)`` or ``(M, N_full)``, ``weights`` None, ``(N_full,)`` or ``(M, N_full)`` (M is 1 when
        neither has rows) and ``prior=(y0 (D,), P (D, D))`` shared by the rows (a per-row prior is a ``ValueError``).
        Returns ``(Y0, cost0, index)`` exactly as ``perband.first_guess_bands`` does, with its tie, zero-weight and NaN
        rules.  On the GPU the table is the candidates' spectra on the device (``candidate_table``; ``table=`` reuses
        one, ``candidates`` may then be None), ``obs`` and ``weights`` go up once and only ``index`` and ``cost`` come
        back.  ``is_gpu=False`` is the explicit numpy branch (``predict_many(is_gpu=False)`` and
        ``_lib.lut_search_numpy``); never a fallback.

        ``space="pc"`` ranks by the same J evaluated in PC space: with the row's weighted least-squares centre ``c0``
        (``G c0 = B W obs``, ``G = B W B^T``), ``J = a + J0 + g0^T d + 1/2 d^T G d`` for ``d = mu(c_l) - c0``, ``J0`` and
        ``g0`` the misfit and its coefficient at ``c0`` -- exact for any ``c0``, a sum of non-negative terms and a tiny
        signed one, ``n_pcs (n_pcs + 1) / 2 + 3 n_pcs + 2`` operations per (row, candidate) instead of ``3 N_full``.
        The table is the ``(n_pcs, L)`` means (``candidate_table(space="pc")``); ``gp_mv_lut_prepare_device`` and
        ``gp_lut_search_pc_device`` run on the device; same ``(Y0, cost0, index)``, same tie, zero-weight and NaN rules;
        a ``table=`` of the other space is a ``ValueError``.  ``is_gpu=False, space="pc"`` is the explicit numpy branch
        (``_lib.lut_search_pc_numpy``).  Rows the PC form cannot centre -- fewer informative bands than PCs, all masked,
        non-finite input, or a ``G`` that is ill-conditioned at the search's precision: a Cholesky pivot not above
        ``(N_full + n_pcs) eps G_kk``, ``eps`` of the device dtype (2.5e-4 of the diagonal in float32 at 2 101 bands,
        4.7e-13 in float64), below which a pivot of a matrix summed over the bands is not told from zero; the set-up
        reports them -- are searched in band space, with a band table built only when such rows exist, at the band
        search's cost per row, and their results are bit for bit ``space="band"`` results: a routing rule by row,
        stated here, not a fallback of precision.  ``self.last_routed_rows`` holds the number of rows the last
        ``space="pc"`` call routed."""
        from . import _first_guess
        if space not in ("band", "pc"):
            raise ValueError("space must be 'band' or 'pc'")
        D, B = self.emulators[0].inputs.shape[1], self.basis_functions.shape[1]
        cand = table.candidates if table is not None and candidates is None else _first_guess.check_candidates(candidates, D)
        n_best = _first_guess.check_n_best(n_best, cand.shape[0])
        obs = np.asarray(obs, dtype=np.float64)
        weights = None if weights is None else np.asarray(weights, dtype=np.float64)
        for name, a in (("obs", obs), ("weights", weights)):
            if a is not None and (a.ndim not in (1, 2) or a.shape[-1] != B):
                raise ValueError("%s must be (%d,) or (n_rows, %d), got %s" % (name, B, B, a.shape))
        rows = [a.shape[0] for a in (obs, weights) if a is not None and a.ndim == 2]
        M = rows[0] if rows else 1
        if any(r != M for r in rows):
            raise ValueError("obs and weights disagree on the number of rows")
        prior = _first_guess.shared_prior(prior, D)
        offset = _first_guess.prior_offset(cand, prior)
        if not is_gpu:
            if space == "pc":
                if self.n_pcs > _lib.lut_pc_max_pcs:
                    raise ValueError("the PC-space search serves n_pcs <= %d" % _lib.lut_pc_max_pcs)
                mu = np.stack([gp.predict(cand)[0] for gp in self.emulators])                       # (P, L)
                index, cost, status = _lib.lut_search_pc_numpy(mu, self.basis_functions, obs, weights, offset, n_best)
                self.last_routed_rows = _first_guess.route_rows(index, cost, status, lambda rows: _lib.lut_search_numpy(
                    mu.T @ self.basis_functions, np.broadcast_to(obs, (M, B))[rows], _first_guess.rows_of(weights, rows),
                    offset, n_best))
            else:
                index, cost = _lib.lut_search_numpy(self.predict_many(cand, is_gpu=False), obs, weights, offset, n_best)
        else:
            tb = table if table is not None else self.candidate_table(cand, precision, space)
            try:
                tb.check(self, precision, B if space == "band" else self.n_pcs, space)
                if tb.candidates.shape != cand.shape or (tb.candidates is not cand and not np.array_equal(tb.candidates, cand)):
                    raise ValueError("table= was built for other candidates")
                if space == "pc":
                    d_basis = self._fresh_gpu_state(tb.dtype)["d_basis"]
                    index, cost, status = _first_guess.search_table_pc(tb, d_basis, obs, weights, offset, M, n_best, B)

                    def band_rows(rows):
                        with self.candidate_table(cand, precision) as band:
                            return _first_guess.search_table_rows(band, np.ascontiguousarray(np.broadcast_to(obs, (M, B))[rows]),
                                                                  _first_guess.rows_of(weights, rows), offset, rows.size, n_best)
                    self.last_routed_rows = _first_guess.route_rows(index, cost, status, band_rows)
                else:
                    index, cost = _first_guess.search_table_rows(tb, obs, weights, offset, M, n_best)
            finally:
                if table is None:
                    tb.close()
        return _first_guess.gather_starts(cand, index, n_best), cost, index

    def posterior_many(self, candidates, obs, weights=None, prior=None, is_gpu=True, precision=np.float64, table=None,
                       space="band"):
        """The Bayesian look-up-table posterior in band space, as ``perband.posterior_bands``: every candidate (L, D) --
        None: the emulators' shared training inputs, or the candidates of ``table=`` -- weighted by
        ``exp(-(J - Jmin))`` with ``first_guess_many``'s J (``obs``, ``weights`` and the shared ``prior`` as there), on the
        ``(L, N_full)`` spectra table (``candidate_table``; ``table=`` reuses one).  Returns ``(mean (M, D), cov (M, D,
        D), info)`` in float64, ``info = dict(index, cost, log_evidence, ess)`` with ``log_evidence = lse - log L``.
        ``is_gpu=False`` is the explicit numpy branch (``predict_many(is_gpu=False)`` and ``_lib.lut_posterior_numpy``);
        never a fallback.  ``space="pc"`` is a ``ValueError``: the fold has no PC-space form."""
        from . import _first_guess
        if space != "band":
            raise ValueError("posterior_many folds in band space only (space=%r)" % (space,))
        D, B = self.emulators[0].inputs.shape[1], self.basis_functions.shape[1]
        if table is not None and candidates is None:
            cand = table.candidates
        else:
            cand = _first_guess.check_candidates(self.emulators[0].inputs if candidates is None else candidates, D)
        obs = np.asarray(obs, dtype=np.float64)
        weights = None if weights is None else np.asarray(weights, dtype=np.float64)
        for name, a in (("obs", obs), ("weights", weights)):
            if a is not None and (a.ndim not in (1, 2) or a.shape[-1] != B):
                raise ValueError("%s must be (%d,) or (n_rows, %d), got %s" % (name, B, B, a.shape))
        rows = [a.shape[0] for a in (obs, weights) if a is not None and a.ndim == 2]
        M = rows[0] if rows else 1
        if any(r != M for r in rows):
            raise ValueError("obs and weights disagree on the number of rows")
        offset = _first_guess.prior_offset(cand, _first_guess.shared_prior(prior, D))
        if not is_gpu:
            out = _lib.lut_posterior_numpy(self.predict_many(cand, is_gpu=False), cand, obs, weights, offset)
        else:
            tb = table if table is not None else self.candidate_table(cand, precision)
            try:
                tb.check(self, precision, B, "band")
                if tb.candidates.shape != cand.shape or (tb.candidates is not cand and not np.array_equal(tb.candidates, cand)):
                    raise ValueError("table= was built for other candidates")

                def strides(a):
                    return (1, B) if a.ndim == 2 else (1, 0)
                out = _first_guess.posterior_table(tb, obs, strides(obs), weights,
                                                   strides(weights) if weights is not None else (0, 0), offset, M)
            finally:
                if table is None:
                    tb.close()
        return _first_guess.posterior_result(out, cand.shape[0])

    def retrieve_many_multistart(self, candidates, obs, weights=None, n_starts=4, table=None, space="band", **loop_args):
        """``retrieve_many`` from several starts per pixel, as ``perband.retrieve_bands_multistart``: ``first_guess_many``
        with ``n_best = n_starts`` ranked with the loop's shared ``prior``, the starts clipped to ``bounds``, ONE
        ``retrieve_many`` call on the ``M n_starts`` rows (row-shaped ``obs``, ``weights`` and ``next_prior`` repeated),
        per pixel the start of lowest ``F = cost + prior term`` kept (ties to the lower start, a non-finite F loses).
        Returns ``(results, start (M,) int32, cost0 (M, n_starts))``, ``results`` exactly the tuple ``retrieve_many``
        returns for M rows.  ``emulator_unc`` and per-row priors are not offered.  ``space`` is ``first_guess_many``'s:
        "pc" ranks the candidates in PC space (``table=`` must then be a ``candidate_table(space="pc")``)."""
        from . import _first_guess
        D = self.emulators[0].inputs.shape[1]
        fg = {k: loop_args[k] for k in ("is_gpu", "precision") if k in loop_args}

        def first_guess(prior, n_best):
            return self.first_guess_many(candidates, obs, weights, prior, n_best, table=table, space=space, **fg)
        return _first_guess.multistart(first_guess, self.retrieve_many, 0, obs, weights, n_starts, D, loop_args)

    def retrieve_series(self, Y0, obs, weights, prior, noise, smooth=False, joint=False, **loop_args):
        """A time series of ``retrieve_many`` on this emulator: ``obs`` (T, N_full) or (T, M, N_full) and ``weights``
        the same or None, one retrieval per date, the posterior of a date propagated by the process noise ``noise``
        (D, D) or (M, D, D) into the prior of the next (``_retrieve.retrieve_series``: what it returns, and why
        ``prior`` is required).  ``loop_args`` are ``retrieve_many``'s other keywords, ``emulator_unc=True`` among them:
        every date's retrieval, and with it the propagated prior and the smoother, then carries the emulators' variance.

        ``smooth=True`` appends the Rauch-Tung-Striebel smoothed trajectory ``X_s (T, M, D)``, ``sigma_s (T, M, D)``
        and ``smooth_status (T, M)``, as ``perband.retrieve_bands_series`` does: on the GPU one ``rts_smooth_device``
        call per date on this emulator's context, with ``is_gpu=False`` ``_lib.rts_smooth_numpy``; never a fallback.

        ``joint=True`` runs the filter and the smoother as ``smooth=True`` does, starts ``retrieve_joint`` from the
        smoothed trajectory ``X_s`` and appends its eight values to the ten, as ``perband.retrieve_bands_series`` does.
        With ``False`` nothing changes."""
        from . import _retrieve
        if joint:
            out = self.retrieve_series(Y0, obs, weights, prior, noise, smooth=True, **loop_args)
            return out + self.retrieve_joint(out[7], obs, weights, prior, noise, **loop_args)
        if not smooth:
            return _retrieve.retrieve_series(self.retrieve_many, Y0, obs, weights, prior, noise, **loop_args)
        context = None
        if loop_args.get("is_gpu", True):
            dt = np.dtype(loop_args.get("precision", np.float64))
            context = lambda: self._fresh_gpu_state(dt)["ctx"]
        return _retrieve.retrieve_series(self.retrieve_many, Y0, obs, weights, prior, noise, smooth=True, context=context,
                                         **loop_args)

    # ---- global sensitivity ---------------------------------------------------------------------
    def sobol(self, bounds, is_gpu=True):
        """Sobol sensitivity indices of every band of the reconstructed output ``f_k = sum_p basis[p, k] mu_p`` for
        independent uniform inputs on ``bounds = (lo, hi)``, each (D,) or (n_boxes, D): ``SobolIndices(first
        (D, N_full), total (D, N_full), variance (N_full,), mean (N_full,))``, with a leading ``n_boxes`` axis for 2-D
        bounds.  The covariances of all ``P (P + 1) / 2`` pairs of PCs come from one ``gp_sobol_batch_f64`` call
        (``is_gpu=False``: the numpy branch), mirrored into (P, P) matrices; a band's indices are the quadratic forms
        ``beta_k' Vm^i beta_k / beta_k' V beta_k`` with ``beta_k = basis[:, k]``.  Nothing of size ``N_full`` is
        emulated.  Not in the reference."""
        from . import _sobol_numpy, perband
        P = self.n_pcs
        mean, cov = perband.sobol_pairs(*perband._sobol_constants(self.emulators), bounds,
                                        pairs=_sobol_numpy.upper_pairs(P), is_gpu=is_gpu)
        return _sobol_numpy.spectral(np.asarray(self.basis_functions)[:P], mean, _sobol_numpy.mirror(cov, P))

    def sobol_interactions(self, bounds, is_gpu=True):
        """Second-order Sobol indices of every band of the reconstructed output on ``bounds`` as ``sobol`` takes them:
        ``SobolInteractions(second (D, D, N_full), higher (N_full,), first (D, N_full), total (D, N_full), variance
        (N_full,), mean (N_full,))``; ``second[i, k, n] = beta_n' V2^{ik} beta_n / beta_n' V beta_n`` off the diagonal
        (symmetric in i, k) and ``first`` on it, ``higher`` the share of the interactions of order three and more.  The
        interaction covariances of all ``P (P + 1) / 2`` pairs of PCs come from one ``gp_sobol_interactions_f64`` call
        and the last four fields from the ``gp_sobol_batch_f64`` call of ``sobol`` (``is_gpu=False``: the numpy
        branch).  Not in the reference."""
        from . import _sobol_numpy, perband
        P = self.n_pcs
        consts, pairs = perband._sobol_constants(self.emulators), _sobol_numpy.upper_pairs(P)
        mean, cov = perband.sobol_pairs(*consts, bounds, pairs=pairs, is_gpu=is_gpu)
        inter = perband.sobol_interaction_pairs(*consts, bounds, pairs=pairs, is_gpu=is_gpu)
        basis = np.asarray(self.basis_functions)[:P]
        covm = _sobol_numpy.mirror(cov, P)
        r = _sobol_numpy.spectral(basis, mean, covm)
        second, higher = _sobol_numpy.spectral_second(basis, covm, _sobol_numpy.mirror(inter, P))
        return _sobol_numpy.SobolInteractions(second, higher, r.first, r.total, r.variance, r.mean)

    def main_effects(self, bounds, grid=None, n_grid=33, is_gpu=True):
        """Main-effect curves of every band of the reconstructed output: ``MainEffects(grid (D, G), effect
        (D, G, N_full), mean (N_full,))`` with ``effect[d, g, n] = E[f_n | t_d = grid[d, g]] - E[f_n]``.  The curve is
        linear in the emulator: the PCs' curves from one ``gp_sobol_main_effects_f64`` call (``is_gpu=False``: the numpy
        branch) times the basis, on the host like the band means.  ``grid`` and ``n_grid`` as
        ``GaussianProcess.main_effects``; a leading ``n_boxes`` axis for 2-D bounds.  Not in the reference."""
        from . import perband
        P = self.n_pcs
        r = perband.main_effects_bands(self.emulators[:P], bounds, grid=grid, n_grid=n_grid, is_gpu=is_gpu)
        basis = np.asarray(self.basis_functions, dtype=np.float64)[:P]
        return r._replace(effect=np.einsum("...pdg,pn->...dgn", r.effect, basis), mean=r.mean @ basis)

    # ---- Gaussian input uncertainty ----------------------------------------------------------------
    def predict_uncertain(self, Y, cov, is_gpu=True, return_pc=False):
        """The reconstructed spectrum ``f_k = sum_p basis[p, k] mu_p`` under Gaussian inputs ``y_m ~ N(Y[m], cov[m])``
        -- ``Y`` (M, D), ``cov`` (D, D) or (M, D, D), positive semi-definite -- by exact moment matching:
        ``UncertainSpectrum(mean (M, N_full), var_state (M, N_full), var_emulator (M, N_full), info (M,))``.  One
        ``gp_moments_batch_f64`` call (``is_gpu=False``: the numpy branch) gives the PCs' means ``M_p``, the covariances
        ``V`` of all ``P (P + 1) / 2`` pairs and the expected emulator variances ``Ev_p``; the mean is reconstructed
        from ``M_p`` as ``predict_many`` reconstructs a spectrum, ``var_state[m, k] = beta_k' V[m] beta_k`` and
        ``var_emulator[m, k] = sum_p beta_pk^2 Ev_p[m]`` with ``beta_k = basis[:, k]``, on the host.  Nothing of size
        ``N_full`` is emulated.  ``return_pc=True`` appends ``pc_mean (M, P)`` and ``pc_cov (M, P, P)``.  ``info`` as
        ``GaussianProcess.predict_uncertain``::

            y, *_, cov, sigma, status = mv.retrieve_many(Y0, obs, return_cov=True)
            s = mv.predict_uncertain(y, cov)          # the predicted-observation distribution of the retrieved states

        Not in the reference."""
        from . import _moments_numpy, perband
        P = self.n_pcs
        mean, _, V, evar, info = perband.moments_pairs(*perband._moments_constants(self.emulators[:P]), Y, cov,
                                                        pairs=_moments_numpy.upper_pairs(P), is_gpu=is_gpu)
        basis = np.asarray(self.basis_functions, dtype=np.float64)[:P]
        pc_cov = _moments_numpy.mirror(V[..., None], P)[..., 0]
        evar = np.full(mean.shape, np.nan) if evar is None else evar
        var_state, var_emulator = _moments_numpy.spectral_variances(basis, pc_cov, evar)
        if return_pc:
            return _moments_numpy.UncertainSpectrumPC(mean @ basis, var_state, var_emulator, info, mean, pc_cov)
        return _moments_numpy.UncertainSpectrum(mean @ basis, var_state, var_emulator, info)

    # ---- second derivatives ---------------------------------------------------------------------
    def hessian(self, y, is_gpu=False, weights=None):
        """Hessian of the reconstructed output at ONE input vector ``y``: ``(N_params, N_params, N_full)`` (axes
        as ``predict``'s ``(N_params, N_full)`` Jacobian), or with ``weights (N_full,)`` the weighted sum over
        the output ``sum_b weights[b] * d2 f_b / dy dy``, ``(N_params, N_params)`` -- the curvature term of a
        cost function with residuals ``weights``.  Not in the reference (which has ``GaussianProcess.hessian``
        only).  ``hessian_many`` on one row."""
        y = np.atleast_2d(y)
        if y.shape[0] != 1:
            raise ValueError("hessian takes one input vector; hessian_many takes rows")
        if weights is not None:
            weights = np.atleast_2d(weights)
        return self.hessian_many(y, is_gpu=is_gpu, weights=weights)[0]

    def hessian_many(self, Y, is_gpu=True, precision=np.float64, weights=None, coef=None):
        """``(M, N_params, N_params, N_full)`` Hessians of the reconstructed outputs for M input rows, or with
        ``weights (M, N_full)`` their weighted sums over the output ``(M, N_params, N_params)``.  The numpy
        branch is ``sum_p basis[p] * emulators[p].hessian(Y)``.  On the GPU all per-PC Hessians are ONE batched
        launch on the device-resident emulator (``_gpu_state``; the host arrays are digested before use and
        the resident copy rebuilt when they were edited in place); the full form is then the reconstruction
        kernel over rows ``(m, d, d2)``, the weighted form ``c[p, m] = sum_b basis[p, b] weights[m, b]`` and the
        device's weighted sum over the PCs -- only the result crosses PCIe.  ``coef (M, n_pcs)`` is an
        alternative to ``weights`` (the two exclude each other): the projection ``basis @ weights[m]`` itself, as
        ``misfit_many(return_coef=True)`` returns it from the device, so that nothing of size ``N_full`` is
        touched on the host."""
        Y = np.atleast_2d(Y)
        M, D = Y.shape
        B = self.basis_functions.shape[1]
        basis = np.asarray(self.basis_functions)
        if coef is not None:
            if weights is not None:
                raise ValueError("give weights or coef, not both")
            coef = np.asarray(coef, dtype=np.float64)
            if coef.shape != (M, self.n_pcs):
                raise ValueError("coef must be (%d, %d), got %s" % (M, self.n_pcs, coef.shape))
            coef = coef.T                                          # (P, M), as the projection below
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.shape != (M, B):
                raise ValueError("weights must be (%d, %d), got %s" % (M, B, weights.shape))
            # (P, M), one matrix-vector product per row: a row's coefficients -- and so its result -- do not depend
            # on how many rows the call has (a matrix-matrix product rounds a column differently per shape)
            b64 = np.ascontiguousarray(basis, dtype=np.float64)
            coef = np.stack([b64 @ weights[m] for m in range(M)], axis=1) if M else np.zeros((self.n_pcs, 0))
        if not is_gpu:
            hp = np.stack([gp.hessian(Y) for gp in self.emulators])           # (P, M, D, D)
            if coef is None:
                return np.einsum("pmde,pb->mdeb", hp, basis)
            return np.einsum("pmde,pm->mde", hp, coef)
        dt = np.dtype(precision)
        st = self._fresh_gpu_state(dt)
        ctx, batch = st["ctx"], st["batch"]
        Yc = np.ascontiguousarray(Y, dtype=dt)
        if coef is not None:
            return np.array(batch.hessian_weighted(Yc, np.ascontiguousarray(coef, dtype=dt)))
        P, isz = self.n_pcs, dt.itemsize
        # rows per round: at most 1 GiB of results on the device (as gp_mv_predict_host)
        step = max(1, (1 << 30) // (D * D * B * isz))
        out = ctx.out_pool.take((M, D, D, B), dt)
        n0 = min(M, step)
        with _lib.Scratch(ctx, dt) as scratch:
            d_y, d_h, d_o = [scratch.alloc(n0 * k * isz) for k in (D, P * D * D, D * D * B)]
            for r0 in range(0, M, step):
                n = min(M, r0 + step) - r0
                ctx.h2d(d_y, Yc[r0:r0 + n])
                batch.hessian_device(d_y, d_h, n)                              # [P][n][D][D]
                ctx.reconstruct_device(dt, st["d_basis"], d_h, d_o, n * D * D, P, B)
                _lib.check(ctx.lib.gp_memcpy_d2h(ctx.h, _lib._ptr(out[r0:r0 + n]), d_o, n * D * D * B * isz),
                           "gp_memcpy_d2h")
        return out
