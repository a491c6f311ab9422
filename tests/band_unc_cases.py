"""Emulators, inputs, the 80-bit truth and the a-priori bound of the per-band misfit with the emulators' variance in the
data term, shared by test_band_unc_cpu.py and test_band_unc_gpu.py (not a test module).

Emulators: E of them on shared inputs X uniform on [0, 1]^D (seeded by the shape), emulator e with targets
sin(X w_e) + 1/2 X_0 X_-1, w_e standard normal, length scales exp(U(log 0.25, log 2)) sqrt(D / 2), b = U(0.5, 4) and
theta = [log(1 / ls^2), log b, log nugget]; invQ and invQt from ``gp_oracle.prepare_likelihood`` in float64 (as
``trained_cases.emulator``, with the nugget an argument).  Nugget 1e-1: well conditioned; 1e-2: moderate; 1e-5: the
variance cancels (a float32 slab holds negative variances).

Inputs: rows uniform in the unit box, the last four in [1, 1.5]^D; obs = the emulators' own means at a second set of
rows; weights = U[0.5, 1.5) / (nugget b_e), which puts w v at order 1.

The truth is evaluated in np.longdouble from per-emulator arrays mu, dmu, v, dv (the slab, or longdouble terms of the
emulators themselves), with the magnitude sums the bound is stated in:

    S_cost = sum_e |a r| + log1p(w vp)            S_grad = sum_e |a| |dmu| + 1/2 weff (1 + |a r|) |dvp|
    S_gn   = sum_e weff |dmu_d| |dmu_d2| + q |dvp_d| |dvp_d2|          S_wr = |a|,  S_weff = weff

    |got - ref| <= 2 (E + K) 2^-53 S   (+ 2^-24 |ref| for a float32 model),   K = 12

K is the largest number of roundings a term carries in band_unc_fold_kernel as written (counted in the header comment of
gp_band_unc_kernel.hpp: cost 10, grad 12, gn 10)."""
import numpy as np

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess

LD = np.longdouble
K_ROUNDINGS = 12
# (n, d, E, nugget): every shape of the GPU tests
GPU_CASES = [(29, 2, 3, 1e-1), (40, 3, 5, 1e-1), (100, 12, 2, 1e-2), (250, 10, 7, 1e-1), (320, 16, 1, 1e-2),
             (33, 13, 37, 1e-1)]
CLAMPED_CASE = (40, 3, 5, 1e-5)              # float32: clamped and unclamped pairs mixed
ROWS = [1, 15, 16, 17, 63, 64, 65, 83, 1000]
M_MAX = max(ROWS)

_emulators = {}


def emulators(n, d, E, nugget):
    """The list of E GaussianProcess objects of a case (kept; the tests leave them unchanged) and their b (E,)."""
    key = (n, d, E, nugget)
    if key not in _emulators:
        X = np.random.RandomState(7000 + 31 * n + d).uniform(size=(n, d))
        gps, bs = [], []
        for e in range(E):
            rs = np.random.RandomState(900000 + 1000 * e + 31 * n + d)
            w = rs.standard_normal(d)
            ls = np.exp(rs.uniform(np.log(0.25), np.log(2.0), d)) * np.sqrt(d / 2.0)
            b = rs.uniform(0.5, 4.0)
            y = np.sin(X @ w) + 0.5 * X[:, 0] * X[:, -1]
            theta = np.concatenate([np.log(1.0 / ls ** 2), [np.log(b), np.log(nugget)]])
            pl = gp_oracle.prepare_likelihood(X, y, theta)
            gp = GaussianProcess(X, y)
            gp.theta, gp.invQ, gp.invQt = theta, pl["invQ"], pl["invQt"]
            gps.append(gp)
            bs.append(np.exp(theta[d]))
        _emulators[key] = (gps, np.array(bs))
    return _emulators[key]


def rows(d, M, seed):
    """M rows in the unit box, the last min(4, M - 1) of them in [1, 1.5]^D."""
    rs = np.random.RandomState(seed)
    t = rs.random_sample((M, d))
    k = min(4, M - 1)
    if k:
        t[M - k:] = 1.0 + 0.5 * rs.random_sample((k, d))
    return t


_inputs = {}


def inputs(n, d, E, nugget, M=M_MAX):
    """(gps, t (M, d), obs (E, M), w (E, M)) in float64 (kept)."""
    key = (n, d, E, nugget, M)
    if key not in _inputs:
        gps, b = emulators(n, d, E, nugget)
        t = rows(d, M, 100 * n + d)
        t2 = np.random.RandomState(n + d + E).random_sample((M, d))
        obs = np.stack([gp.cpu_predict(t2, do_unc=False)[0] for gp in gps])
        w = (0.5 + np.random.RandomState(E).random_sample((E, M))) / (nugget * b[:, None])
        _inputs[key] = (gps, t, obs, w)
    return _inputs[key]


def retrieval_inputs(n, d, E, M=33):
    """x_true in the box, obs the means there, X0 beside it, weights of inputs: for retrieve_bands."""
    gps, _, _, w = inputs(n, d, E, 1e-1)
    x_true = np.random.RandomState(n + d).uniform(0.1, 0.9, (M, d))
    obs = np.stack([gp.cpu_predict(x_true, do_unc=False)[0] for gp in gps])
    X0 = np.clip(x_true + 0.05 * np.random.RandomState(n + E).uniform(-1.0, 1.0, (M, d)), 0.0, 1.0)
    return gps, X0, obs, np.ascontiguousarray(w[:, :M]), (np.zeros(d), np.ones(d))


def terms_ld(gps, X):
    """mu (E, M), dmu (E, M, D), v (E, M), dv (E, M, D) of the emulators in longdouble from their float64 arrays."""
    X = np.asarray(X).astype(LD)
    out = [[], [], [], []]
    for gp in gps:
        inp, D = np.asarray(gp.inputs).astype(LD), X.shape[1]
        expX = np.exp(np.asarray(gp.theta, dtype=np.float64)).astype(LD)
        e, b = expX[:D], expX[D]
        diff = inp[:, None, :] - X[None, :, :]                                  # (N, M, D)
        k = b * np.exp(LD(-0.5) * ((diff * diff) @ e))                          # (N, M)
        wq = k * np.asarray(gp.invQt).astype(LD)[:, None]
        Q = np.asarray(gp.invQ).astype(LD)
        W = ((Q + Q.T) @ k) * k
        out[0].append(wq.sum(0))
        out[1].append(e * np.einsum("nm,nmd->md", wq, diff))
        out[2].append(b - LD(0.5) * W.sum(0))
        out[3].append(-e * np.einsum("nm,nmd->md", W, diff))
    return tuple(np.stack(a) for a in out)


def terms_f64(gps, X):
    """The same four arrays from the numpy branches (float64): a stand-in for the device's slab on a machine without one."""
    X = np.asarray(X, dtype=np.float64)
    mu, v, dmu = (np.stack(a) for a in zip(*[gp.cpu_predict(X, do_unc=True) for gp in gps]))
    dv = np.stack([gp.variance_gradient(X, is_gpu=False)[1] for gp in gps])
    return mu, dmu, v, dv


def _em(a, E, M):
    a = np.asarray(a)
    return np.broadcast_to(a if a.ndim == 2 else a[:, None], (E, M))


def truth(mu, dmu, v, dv, obs, w):
    """dict name -> (ref, S) in longdouble for cost, grad, gn, wr, weff, from per-emulator arrays of any dtype."""
    E, M = mu.shape
    mu, dmu, v, dv = (np.asarray(a).astype(LD) for a in (mu, dmu, v, dv))
    o = _em(obs, E, M).astype(LD)
    ww = np.ones((E, M), LD) if w is None else _em(w, E, M).astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        r = mu - o
        clamp = v <= 0
        vp = np.where(clamp, LD(0), v)
        dvp = np.where(clamp[:, :, None], LD(0), dv)
        weff = ww / (1 + ww * vp)
        a = weff * r
        c = np.where(clamp, LD(0), LD(0.5) * weff * (1 - a * r))
        q = np.where(clamp, LD(0), LD(0.5) * weff * weff)
        lg = np.log1p(ww * vp)
        cost = LD(0.5) * (a * r + lg).sum(0)
        S_cost = LD(0.5) * (np.abs(a * r) + lg).sum(0)
        grad = (a[:, :, None] * dmu + c[:, :, None] * dvp).sum(0)
        cabs = np.where(clamp, LD(0), LD(0.5) * weff * (1 + np.abs(a * r)))
        S_grad = (np.abs(a)[:, :, None] * np.abs(dmu) + cabs[:, :, None] * np.abs(dvp)).sum(0)
        gn = np.einsum("em,emd,emf->mdf", weff, dmu, dmu) + np.einsum("em,emd,emf->mdf", q, dvp, dvp)
        am, av = np.abs(dmu), np.abs(dvp)
        S_gn = np.einsum("em,emd,emf->mdf", weff, am, am) + np.einsum("em,emd,emf->mdf", q, av, av)
    return {"cost": (cost, S_cost), "grad": (grad, S_grad), "gn": (gn, S_gn), "wr": (a, np.abs(a)), "weff": (weff, weff)}


def fold_bound(ref, S, E, prec, scale=1):
    """The bound; ``scale`` multiplies the chain's part only (the rounding of a float32 store is 2^-24 |ref| whatever
    the chain did)."""
    bound = scale * 2 * (E + K_ROUNDINGS) * LD(2) ** -53 * S
    if np.dtype(prec) == np.float32:
        bound = bound + LD(2) ** -24 * np.abs(ref)
    return bound


def excess(got, ref, S, E, prec, scale=1):
    """max of |got - ref| / bound (the chain's part of it times ``scale``) over the elements (0 where both the error and the bound are 0); <= 1 passes.
    Elements whose reference is not finite must be not finite in ``got`` as well."""
    got = np.asarray(got).astype(LD)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    if not fin.any():
        return 0.0
    err, bound = np.abs(got - ref)[fin], fold_bound(ref, S, E, prec, scale)[fin]
    ok = err <= bound
    return float(np.max(np.where(ok & (bound == 0), LD(0), err / np.maximum(bound, LD(1e-4000)))))


def chain(mu, dmu, v, dv, obs, w, out_dtype, work=np.float64):
    """A restatement of band_unc_fold_kernel's chain in the dtype ``work`` (float64: the kernel's): the emulators in
    order, the coefficient formulas as written, two accumulations per emulator, one rounding to ``out_dtype`` at the end.
    dict as ``truth``'s, values only."""
    E, M = mu.shape
    D = dmu.shape[2]
    mu, dmu, v, dv = (np.asarray(a).astype(work) for a in (mu, dmu, v, dv))
    o = _em(obs, E, M).astype(work)
    ww = np.ones((E, M), work) if w is None else _em(w, E, M).astype(work)
    zero, half, one = work(0), work(0.5), work(1)
    cost, grad, gn = np.zeros(M, work), np.zeros((M, D), work), np.zeros((M, D, D), work)
    wr, weffs = np.empty((E, M), work), np.empty((E, M), work)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(E):
            r = mu[e] - o[e]
            clamp = v[e] <= 0
            vp = np.where(clamp, zero, v[e])
            dvp = np.where(clamp[:, None], zero, dv[e])
            wv = ww[e] * vp
            weff = ww[e] / (one + wv)
            a = weff * r
            ar = a * r
            c = np.where(clamp, zero, (half * weff) * (one - ar))
            q = np.where(clamp, zero, half * (weff * weff))
            cost = cost + (ar + np.log1p(wv))
            grad = grad + a[:, None] * dmu[e]
            grad = grad + c[:, None] * dvp
            gn = gn + weff[:, None, None] * (dmu[e][:, :, None] * dmu[e][:, None, :])
            gn = gn + q[:, None, None] * (dvp[:, :, None] * dvp[:, None, :])
            wr[e], weffs[e] = a, weff
    assert cost.dtype == gn.dtype == np.dtype(work)
    return {k: a.astype(out_dtype) for k, a in (("cost", half * cost), ("grad", grad), ("gn", gn), ("wr", wr), ("weff", weffs))}


def terms_f32(gps, X):
    """mu, dmu, v, dv evaluated entirely in float32 (the difference form on the raw coordinates, every array rounded to
    float32 first): with ``chain(..., work=np.float32)`` the yardstick of the float32 end-to-end gate."""
    F = np.float32
    X = np.asarray(X).astype(F)
    out = [[], [], [], []]
    for gp in gps:
        inp, D = np.asarray(gp.inputs).astype(F), X.shape[1]
        expX = np.exp(np.asarray(gp.theta, dtype=np.float64)).astype(F)
        e, b = expX[:D], expX[D]
        diff = inp[:, None, :] - X[None, :, :]
        k = b * np.exp(F(-0.5) * ((diff * diff) @ e))
        alpha, Q = np.asarray(gp.invQt).astype(F), np.asarray(gp.invQ).astype(F)
        wq = k * alpha[:, None]
        W = ((Q + Q.T) @ k) * k
        out[0].append(wq.sum(0))
        out[1].append(e * np.einsum("nm,nmd->md", wq, diff))
        out[2].append(b - F(0.5) * W.sum(0))
        out[3].append(-e * np.einsum("nm,nmd->md", W, diff))
    res = tuple(np.stack(a) for a in out)
    assert all(a.dtype == F for a in res)
    return res
