"""Cases, the 80-bit truth and the error measure shared by test_likelihood_truth_cpu.py and test_likelihood_gpu.py
(not a test module).

``truth`` evaluates the training objective of gp_train_kernel.hpp's header in np.longdouble (64-bit significand on
x86, eps 1.08e-19) from the float64 inputs as the kernels get them: Z and Q with longdouble exp, Q = L L^T by a column
Cholesky with vectorised rank-1 updates, L^-1 by a vectorised forward substitution, invQ = L^-T L^-1, then invQt,
cost (logdet = 2 sum log L_kk) and the D + 2 gradient components

    g_d = e_d / 4 sum_ij c_ij (x_id - x_jd)^2,  g_D = -1/2 sum_ij c_ij,  g_D+1 = 1/2 e_D+1 (tr invQ - a.a),
    c_ij = (a_i a_j - invQ_ij) Z_ij,  a = invQt,

together with each component's TERM MAGNITUDE G: the same sums with c_ij replaced by (|a_i a_j| + |invQ_ij|) Z_ij, and
G_D+1 = 1/2 e_D+1 (sum |invQ_ii| + a.a).  A gradient is judged against G, not against |g|: at a trained theta g is a
difference of nearly equal terms and that cancellation is not the kernel's error.

The measure, with u = 2^-53 and kappa = cond_2 of the float64 Q: a result passes when

    max|invQ - V| / max|V|,  max|invQt - a| / max|a|,  |cost - c| / max(1, |c|),  max_k |g_k - g*_k| / G_k

are all <= K kappa u, K = 8 (a component with G_k = 0 must be exactly 0).  K is nearly six times the worst ratio of
the reference's own numpy route over the case list (1.37, the gradient at N = 1, where kappa = 1;
test_likelihood_truth_cpu.py asserts the bound for every case), not a figure taken from the kernels.

Which compiled instance a case runs (launch_likelihood in gp_train_tu.hip): N <= 256 likelihood_mfma_kernel<DM>, else
likelihood_kernel + likelihood_grad_kernel<DM>, DM = 4, 8, 12, 16 the smallest >= D; with GP_TRAIN_GENERIC=1 (read
once per process) the second pair at every N.  ``instance`` states that rule.

Run as a program (``python likelihood_cases.py OUT.npz``) it evaluates AB_KEYS on device 0 with the inverse and saves
the arrays: the child process of the A/B test, started with GP_TRAIN_GENERIC=1 in its environment.
"""
import functools
import os
import sys

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
K = 8.0

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MFMA_SHAPES = [(1, 1), (2, 16), (7, 3), (8, 13), (9, 5), (15, 9), (16, 4), (17, 6), (24, 9), (33, 12),
               (120, 8), (128, 16), (129, 7), (240, 4), (241, 12), (248, 8), (249, 5), (255, 13), (256, 16), (256, 1)]
WORKSPACE_SHAPES = [(257, 4), (257, 8), (257, 13), (264, 12), (300, 3), (505, 13), (511, 7)]
NOISES = [-4, -9]
# a key is (N, D, noise) for a seeded case or a name for a committed real problem
REAL_KEYS = ["prosail_pc0", "smooth0", "smooth1", "smooth2"]
CASE_KEYS = [(n, d, z) for n, d in MFMA_SHAPES + WORKSPACE_SHAPES for z in NOISES] + REAL_KEYS
AB_KEYS = [(n, d, -4) for n, d in [(1, 1), (3, 2), (7, 3), (8, 13), (9, 5), (24, 9), (129, 7), (249, 5), (256, 16)]] + ["prosail_pc0"]


def key_id(key):
    return key if isinstance(key, str) else "n%d_d%d_noise%d" % key


def instance(N, D, generic=False):
    dm = 4 * ((D + 3) // 4)
    return ("mfma<%d>" if N <= 256 and not generic else "workspace+grad<%d>") % dm


def _golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def seeded(N, D, noise):
    rs = np.random.RandomState(1000 * D + N)
    X = rs.random_sample((N, D))
    t = np.sin(X.sum(1))
    theta = np.concatenate([0.3 * rs.standard_normal(D), [0.0, float(noise)]])
    return X, t, theta


@functools.lru_cache(maxsize=None)
def case(key):
    """(X, t, theta) of a key, float64, read-only."""
    if isinstance(key, str):
        g = _golden("training_objective")
        if key == "prosail_pc0":
            p = _golden("prosail_pc0")
            out = p["inputs"], p["targets"], g["prosail_pc0_theta"]
        else:
            out = g["smooth_inputs"], g["smooth_targets"], g["smooth_thetas"][int(key[-1])]
    else:
        out = seeded(*key)
    out = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in out)
    for a in out:
        a.setflags(write=False)
    return out


def truth(X, t, theta):
    """dict(invQ, invQt, cost, grad, G, Q, cond) of the module docstring; invQ .. G in longdouble, Q the longdouble
    matrix rounded to float64 and cond its 2-norm condition number."""
    X, t, theta = (np.asarray(a, dtype=np.float64).astype(LD) for a in (X, t, theta))
    N, D = X.shape
    e = np.exp(theta)
    dl2 = [(X[:, d, None] - X[None, :, d]) ** 2 for d in range(D)]
    r2 = np.zeros((N, N), LD)
    for d in range(D):
        r2 += e[d] * dl2[d]
    Z = e[D] * np.exp(LD(-0.5) * r2)
    Q = Z + e[D + 1] * np.eye(N, dtype=LD)
    # Cholesky, a column at a time; the trailing matrix takes each column's rank-1 update
    A = Q.copy()
    L = np.zeros((N, N), LD)
    for k in range(N):
        if not A[k, k] > 0:
            raise np.linalg.LinAlgError("truth: pivot %d is not positive" % k)
        L[k, k] = np.sqrt(A[k, k])
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] -= L[k + 1:, k, None] * L[None, k + 1:, k]
    # Y = L^-1 by forward substitution on the identity (row k of Y is finished at step k; Y is lower triangular)
    Y = np.eye(N, dtype=LD)
    for k in range(N):
        Y[k, :k + 1] /= L[k, k]
        Y[k + 1:, :k + 1] -= L[k + 1:, k, None] * Y[None, k, :k + 1]
    invQ = Y.T @ Y
    a = invQ @ t
    cost = np.sum(np.log(np.diag(L))) + LD(0.5) * (t @ a) + LD(0.5) * N * np.log(8 * np.arctan(LD(1)))
    aa = a[:, None] * a[None, :]
    c = (aa - invQ) * Z
    C = (np.abs(aa) + np.abs(invQ)) * Z
    g, G = np.zeros(D + 2, LD), np.zeros(D + 2, LD)
    for d in range(D):
        g[d] = e[d] / 4 * np.sum(c * dl2[d])
        G[d] = e[d] / 4 * np.sum(C * dl2[d])
    g[D], G[D] = -np.sum(c) / 2, np.sum(C) / 2
    g[D + 1] = e[D + 1] / 2 * (np.trace(invQ) - a @ a)
    G[D + 1] = e[D + 1] / 2 * (np.sum(np.abs(np.diag(invQ))) + a @ a)
    Q64 = Q.astype(np.float64)
    return dict(invQ=invQ, invQt=a, cost=cost, grad=g, G=G, Q=Q64, cond=float(np.linalg.cond(Q64)))


@functools.lru_cache(maxsize=None)
def truth_of(key):
    """``truth`` of a key, computed once per process (about a second at N = 250, a few at N = 510); leave it unchanged."""
    return truth(*case(key))


def ratios(tr, cost, grad, invQ=None, invQt=None, other=None):
    """The four errors of the module docstring in units of kappa u: dict(invQ, invQt, cost, grad), the quantities not
    given left out.  grad is inf where a component with G_k = 0 is not exactly 0.  With ``other`` (a dict of a second
    float64 result) the differences are taken to it instead of to the truth, on the truth's scales."""
    ku = tr["cond"] * U
    ref = tr if other is None else other
    out = {}
    for name, got in (("invQ", invQ), ("invQt", invQt)):
        if got is not None:
            out[name] = float(np.max(np.abs(np.asarray(got).astype(LD) - ref[name])) / np.max(np.abs(tr[name])) / ku)
    out["cost"] = float(abs(LD(float(cost)) - LD(ref["cost"])) / max(LD(1), abs(tr["cost"])) / ku)
    err = np.abs(np.asarray(grad).astype(LD) - ref["grad"])
    zero = tr["G"] == 0
    r = np.where(zero, np.where(err == 0, LD(0), LD(np.inf)), err / np.where(zero, LD(1), tr["G"]))
    out["grad"] = float(np.max(r) / ku)
    return out


def check(tr, cost, grad, invQ=None, invQt=None, label="", other=None):
    """Assert the bound on whatever is given (between two float64 results: the sum of their bounds); prints the ratios
    first (pytest -s shows them) and returns them."""
    r = ratios(tr, cost, grad, invQ, invQt, other)
    k = K if other is None else 2 * K
    print("%s cond %.3g: %s" % (label, tr["cond"], "  ".join("%s %.3g" % kv for kv in r.items())))
    for name, v in r.items():
        assert v <= k, "%s %s: %.4g kappa u > %g kappa u (cond %.3g)" % (label, name, v, k, tr["cond"])
    return r


def main(out_path):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    from gp_emulator_amd import _lib
    _lib.load()
    ctx = _lib.default_context(0)
    out = {}
    for key in AB_KEYS:
        X, t, theta = case(key)
        cost, grad, invQ, invQt = ctx.likelihood_batch(theta[None, :], X, t, want_inverse=True)
        for name, a in (("cost", cost), ("grad", grad), ("invQ", invQ), ("invQt", invQt)):
            out[key_id(key) + "/" + name] = a[0]
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
