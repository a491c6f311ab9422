"""What the CPU and GPU tests of the multivariate retrieval share (test_mv_retrieve_cpu.py, test_mv_retrieve_gpu.py):
the synthetic emulators, the retrieval problem on them and the extended-precision statements of the two new
contractions.  Error metric, as in the misfit tests: max|ref - got| / max|ref|."""
import numpy as np

from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, MultivariateEmulator, _lib

LD = np.longdouble
TOL = {np.float64: 1e-10, np.float32: 1e-4}
# (P, N, D, B) of the retrieval tests: both full rank (P >= D); M = 65 rows is one work item + 1 row
RETRIEVAL_SHAPES = [(7, 100, 5, 301), (12, 40, 9, 33)]


def err(ref, got):
    ref = np.asarray(ref, dtype=LD)
    scale = np.max(np.abs(ref))
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref)) / (scale if scale > 0 else 1))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def synthetic_emulator(P, N, D, B, M, seed):
    """P benchmark_inputs GPs on shared inputs with a random normal basis (no PCA, no training), as
    test_misfit_gpu.synthetic_emulator builds them; returns the emulator and M rows in the unit cube."""
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(seed, N, D, M)
    mv.emulators = []
    for p in range(P):
        if p:
            _, _, theta, invQ, invQt = gp_oracle.benchmark_inputs(seed + p, N, D, 1)
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQ, gp.invQt = theta, invQ, invQt
        mv.emulators.append(gp)
    mv.n_pcs = P
    mv.basis_functions = np.random.RandomState(seed).standard_normal((P, B))
    return mv, testing


def gram_ref(basis, w, dt):
    """G[m] = basis diag(w[m]) basis^T in arithmetic ``dt``, row by row as a two-operand product (NOT a three-operand
    einsum, which runs one chain over the bands)."""
    b = np.asarray(basis, dtype=dt)
    w = np.asarray(w, dtype=dt)
    return np.stack([(b * w[m]) @ b.T for m in range(w.shape[0])])


def contract_ref(deriv, G, dt):
    d, G = np.asarray(deriv, dtype=dt), np.asarray(G, dtype=dt)
    return np.einsum("pmd,mpq,qme->mde", d, G, d)


_cases = {}


def retrieval_case(P, N, D, B, M=65):
    """The emulator, obs = its numpy reconstruction at x_true, Y0 around x_true, bounds [0, 1], per-row weights
    U(0.5, 2) / B with 30 % zeros, and the numpy branch's run with them: computed once, never changed."""
    key = (P, N, D, B, M)
    if key not in _cases:
        mv, x_true = synthetic_emulator(P, N, D, B, M, 4242)
        obs = mv.predict_many(x_true, is_gpu=False)
        rs = np.random.RandomState(3)
        Y0 = np.clip(x_true + 0.05 * rs.uniform(-1.0, 1.0, (M, D)), 0.0, 1.0)
        w = rs.uniform(0.5, 2.0, (M, B)) / B
        w[rs.random_sample((M, B)) < 0.3] = 0.0
        bounds = (np.zeros(D), np.ones(D))
        cost0, grad0 = mv.misfit_many(Y0, obs, weights=w, is_gpu=False)
        gn0 = mv.gauss_newton_many(Y0, weights=w, is_gpu=False)
        ref = mv.retrieve_many(Y0, obs, weights=w, bounds=bounds, is_gpu=False)
        trial0 = _lib.newton_step_numpy(Y0, grad0, gn0, 1e-2, "diagonal", None, bounds)[1]
        for a in (obs, Y0, w, cost0, gn0, trial0) + ref:
            a.setflags(write=False)
        _cases[key] = dict(mv=mv, obs=obs, Y0=Y0, w=w, bounds=bounds, cost0=cost0, gn0=gn0, ref=ref, trial0=trial0)
    return _cases[key]
