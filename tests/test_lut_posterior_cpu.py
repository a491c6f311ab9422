"""The look-up-table posterior without a GPU: the numpy branch against the longdouble truth within the derived gate, the
exact cases, the linear-Gaussian case against its analytic posterior, what the feature is for (two basins), the bad-row
rules, the wrappers with is_gpu=False, the launch plan and the binding."""
import ctypes

import numpy as np
import pytest

import lut_cases as lc
import lut_posterior_cases as pc
from mv_retrieve_cases import synthetic_emulator

from gp_emulator_amd import _lib, _retrieve, perband

F64, F32 = np.float64, np.float32


def numpy_branch(c, **kw):
    return _lib.lut_posterior_numpy(c["S"], c["X"], c["o"], c["w"], c["a"], **kw)


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    for name, nargs in (("gp_lut_posterior_device", 26), ("gp_lut_posterior_geometry", 7)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    for D in (1, 8, 9, 12, 13, 16):
        for dt in (F64, F32):
            geo = _lib.lut_posterior_geometry(D, dt)
            assert geo["padded_dims"] == (8 if D <= 8 else 12 if D <= 12 else 16) and geo["workgroups_per_cu"] >= 1
            assert geo["rows_per_item"] > 0 and geo["candidate_tile"] % 8 == 0 and geo["term_chunk"] > 0
    for bad in (0, 17):
        with pytest.raises(_lib.GpuPredictError):
            _lib.lut_posterior_geometry(bad)


# ---- the numpy branch against the truth ------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("D", [1, 2, 11, 16])
def test_numpy_branch_against_the_truth(K, D):
    # (a row whose weights are all 0 has every J equal: with one term and no offset the per-row zeros give way to shared weights)
    last = ("rows", False, 24) if K > 1 else ("shared", False, 24)
    for weights, offset, seed in ((None, False, 21), ("shared", True, 22), ("rows", True, 23), last):
        c = pc.make_case(F64, 23, 150, K, D, seed=seed, weights=weights, offset=offset)
        val, gate = pc.truth(c)
        out = numpy_branch(c)
        worst = pc.check(val, gate, out, (K, D, weights, offset))
        print("K %d D %d %s %s: worst error / (2 gate) %s" % (K, D, weights, offset, worst))
        # chunked over rows: the index and cost are the same whatever the chunk, the moments within the gate
        chunked = numpy_branch(c, max_elements=150 * max(K, D) * 4)
        lc.same(out[0], chunked[0]), lc.same(out[1], chunked[1])
        pc.check(val, gate, chunked, "chunked")


def test_numpy_branch_float32_inputs_and_the_gpu_grid_is_separated():
    """Inputs rounded to float32 (the gate of float32) and the separation of every case the GPU tests use, asserted
    here where no GPU is needed (make_case asserts it)."""
    c = pc.make_case(F32, 9, 40, 7, 3, seed=31)
    val, gate = pc.truth(c)
    pc.check(val, gate, numpy_branch(c), "float32 inputs")
    for dt in pc.DTYPES:
        for M, L, K, D, weights, offset, seed in pc.grid_cases(dt, lambda D: _lib.lut_posterior_geometry(D, dt)):
            pc.make_case(dt, M, L, K, D, seed=seed, weights=weights, offset=offset)
        pc.round_case(dt, 3000)
    with pytest.raises(AssertionError):      # two equal candidates are not separated
        S = np.zeros((2, 3))
        T, g = lc.truth(lc.as_case(F64, S, np.ones(3)))
        assert pc.separated(T, g)


def test_gate_rejects_wrong_results():
    c = pc.make_case(F64, 5, 60, 7, 3, seed=41)
    val, gate = pc.truth(c)
    index, cost, mean, cov, lse, ess = numpy_branch(c)
    pc.check(val, gate, (index, cost, mean, cov, lse, ess))
    skew = cov.copy()
    skew[:, 0, 1] *= 1 + 1e-15
    for bad in ((index, cost, mean * (1 + 1e-9), cov, lse, ess), (index, cost, mean, cov * (1 + 1e-9), lse, ess),
                (index, cost, mean, cov, lse + 1e-9, ess), (index, cost, mean, cov, lse, ess * (1 + 1e-9)),
                (index, cost, mean, skew, lse, ess), (np.roll(index, 1), cost, mean, cov, lse, ess)):
        with pytest.raises(AssertionError):
            pc.check(val, gate, bad)


# ---- exact cases -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", pc.DTYPES)
def test_one_candidate_is_exact(dt):
    c = pc.one_candidate_case(dt)
    pc.check_one_candidate(c, numpy_branch(c))


@pytest.mark.parametrize("dt", pc.DTYPES)
def test_two_candidates_are_exact(dt):
    c = pc.two_candidate_case(dt)
    pc.check_two_candidates(c, numpy_branch(c))


# ---- the linear-Gaussian case ------------------------------------------------------------------------------

def test_linear_gaussian_posterior():
    """S = A x on a regular D = 2 grid of spacing sigma_min / 2 that covers +-8 sigma of the analytic posterior
    N((A^T W A)^-1 A^T W o, (A^T W A)^-1).  The trapezoid sum of a Gaussian at that spacing is wrong by O(exp(-2 pi^2 4))
    and the truncation by O(exp(-32)): mean and cov match to 1e-9 relative, and lse + log(cell area) the analytic
    integral log(2 pi sqrt(det C)) - J(x^) to the same tolerance."""
    A = np.array([[1.0, 0.3], [-0.2, 0.9], [0.5, 0.5]])
    W = np.array([400.0, 250.0, 300.0])
    x_true = np.array([0.4, 0.6])
    o = A @ x_true + np.array([0.01, -0.02, 0.015])
    P = A.T @ (W[:, None] * A)
    C = np.linalg.inv(P)
    xh = C @ (A.T @ (W * o))
    Jh = 0.5 * np.sum(W * (A @ xh - o) ** 2)
    h = np.sqrt(np.linalg.eigvalsh(C)[0]) / 2
    axes = [xh[d] + 0.37 * h + h * np.arange(-np.ceil(8 * np.sqrt(C[d, d]) / h), np.ceil(8 * np.sqrt(C[d, d]) / h) + 1)
            for d in range(2)]
    X = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 2)
    index, cost, mean, cov, lse, ess = _lib.lut_posterior_numpy(X @ A.T, X, o, W)
    assert np.max(np.abs(mean[0] - xh)) <= 1e-9 * np.max(np.abs(xh))
    assert np.max(np.abs(cov[0] - C)) <= 1e-9 * np.max(np.abs(C))
    want = np.log(2 * np.pi * np.sqrt(np.linalg.det(C))) - Jh
    assert abs(lse[0] + np.log(h * h) - want) <= 1e-9 * abs(want)
    # the effective sample size of a Gaussian sampled on a grid: (int p)^2 / int p^2 / cell = 4 pi sqrt(det C) / h^2
    assert abs(ess[0] - 4 * np.pi * np.sqrt(np.linalg.det(C)) / (h * h)) <= 1e-9 * ess[0]


# ---- what the feature is for -------------------------------------------------------------------------------

def test_two_basins():
    """A forward model that cannot tell x_0 from 1 - x_0: per-band emulators trained on f(x) = ((x_0 - 1/2)^2, x_1).  An
    observation of x = (0.2, 0.6) is explained equally well near (0.8, 0.6).  The posterior over a grid of candidates
    reports both: ess > 1, a mean between the clusters and a covariance whose leading eigenvector joins them;
    retrieve_bands(return_cov=True) from either side reports one basin and a spread that does not reach the other."""
    from gp_emulator_amd import GaussianProcess
    rs = np.random.RandomState(3)
    inputs = rs.uniform(0.0, 1.0, (60, 2))
    gps = []
    for f in ((inputs[:, 0] - 0.5) ** 2, inputs[:, 1]):
        gp = GaussianProcess(inputs, f)
        gp._set_params(np.log([4.0, 4.0, 1.0, 1e-8]))      # (fixed hyper-parameters: smooth functions, no training run)
        gps.append(gp)
    g = (np.arange(41) + 0.5) / 41
    cand = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    obs = np.array([(0.2 - 0.5) ** 2, 0.6])
    w = np.array([4.0e4, 1.0e3])
    mean, cov, info = perband.posterior_bands(gps, cand, obs, w, is_gpu=False)
    assert info["ess"][0] > 2
    assert abs(mean[0, 0] - 0.5) < 0.05 and abs(mean[0, 1] - 0.6) < 0.05
    lam, vec = np.linalg.eigh(cov[0])
    assert abs(vec[0, -1]) > 0.99 and 0.25 < np.sqrt(lam[-1]) < 0.35         # (two clusters 0.6 apart: sigma 0.3)
    for start, side in (((0.25, 0.5), 0.2), ((0.75, 0.5), 0.8)):
        res = perband.retrieve_bands(gps, np.array([start]), obs[:, None], w[:, None], bounds=(np.zeros(2), np.ones(2)),
                                     is_gpu=False, return_cov=True)
        x = res[0][0]
        assert abs(x[0] - side) < 0.05                                           # one basin ...
        assert abs(x[0] - mean[0, 0]) > 0.2                                       # ... not the posterior mean
        cov_lm = [a for a in res if np.shape(a) == (1, 2, 2)][0][0]
        assert np.sqrt(cov_lm[0, 0]) < 0.1                                        # ... and a spread that does not reach the other


# ---- bad rows, masking, the table --------------------------------------------------------------------------

def test_bad_rows_masking_and_table_candidates():
    c = pc.make_case(F64, 8, 30, 5, 3, seed=51, weights="rows", offset=True)
    base = numpy_branch(c)
    o, w = c["o"].copy(), c["w"].copy()
    live = [np.argwhere(w[m] != 0)[0, 0] for m in (1, 3, 5)]
    o[1, live[0]] = np.nan
    o[3, live[1]] = np.inf
    w[5, live[2]] = np.inf
    out = _lib.lut_posterior_numpy(c["S"], c["X"], o, w, c["a"])
    for m in (1, 3, 5):
        assert out[0][m] == -1 and all(np.all(np.isnan(a[m])) for a in out[1:])
    keep = [0, 2, 4, 6, 7]
    pc.same_outputs([a[keep] for a in out], [a[keep] for a in base])
    # a NaN observation under a weight of exactly 0 is masked: the case holds such terms already
    assert np.isnan(c["o"]).any() and np.all(base[0] >= 0) and np.all(np.isfinite(base[2]))
    # a NaN or an infinity in the table takes its candidate out for every row: the call without that candidate
    S = c["S"].copy()
    S[4, 0], S[9, 1] = np.nan, np.inf
    rest = np.delete(np.arange(30), [4, 9])
    got = _lib.lut_posterior_numpy(S, c["X"], c["o"], c["w"], c["a"])
    ref = _lib.lut_posterior_numpy(c["S"][rest], c["X"][rest], c["o"], c["w"], c["a"][rest])
    lc.same(got[0], rest[ref[0]].astype(np.int32))
    val, gate = pc.truth(dict(c, S=c["S"][rest], X=c["X"][rest], a=c["a"][rest], L=28))
    pc.check(dict(val, index=got[0]), gate, got, "NaN candidates")
    with pytest.raises(ValueError):
        _lib.lut_posterior_numpy(c["S"], c["X"][:5], c["o"])
    with pytest.raises(ValueError):
        _lib.lut_posterior_numpy(c["S"], np.zeros((30, 17)), c["o"])
    with pytest.raises(ValueError):
        _lib.lut_posterior_numpy(c["S"], c["X"], c["o"][:, :4])
    same = _lib.Context.lut_posterior(None, c["S"], c["X"], c["o"], c["w"], c["a"], is_gpu=False)
    pc.same_outputs(same, base)


# ---- the wrappers, numpy branch -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    mv, x_true = synthetic_emulator(5, 40, 3, 21, 6, 77)
    rs = np.random.RandomState(9)
    cand = rs.uniform(0.0, 1.0, (200, 3))
    prior = (np.full(3, 0.5), np.diag([0.3, 0.2, 0.1]) + 0.02)
    return dict(mv=mv, gps=mv.emulators, x_true=x_true, cand=cand, prior=prior,
                obs_mv=mv.predict_many(x_true, is_gpu=False),
                obs_pb=np.stack([gp.cpu_predict(x_true, do_unc=False)[0] for gp in mv.emulators]))


def check_wrapper(res, direct, L):
    mean, cov, info = res
    assert sorted(info) == ["cost", "ess", "index", "log_evidence"]
    lc.same(info["index"], direct[0]), lc.same(info["cost"], direct[1]), lc.same(mean, direct[2]), lc.same(cov, direct[3])
    lc.same(info["log_evidence"], direct[4] - np.log(L)), lc.same(info["ess"], direct[5])


def test_posterior_bands_numpy(small):
    gps, cand, prior, obs = small["gps"], small["cand"], small["prior"], small["obs_pb"]
    w = 200.0 * np.random.RandomState(1).uniform(0.5, 2.0, obs.shape)
    S = np.stack([gp.cpu_predict(cand, do_unc=False)[0] for gp in gps], axis=1)
    check_wrapper(perband.posterior_bands(gps, cand, obs, w, is_gpu=False), _lib.lut_posterior_numpy(S, cand, obs.T, w.T), 200)
    a = _retrieve._prior_term(cand, prior)
    res = perband.posterior_bands(gps, cand, obs, w, prior=prior, is_gpu=False)
    check_wrapper(res, _lib.lut_posterior_numpy(S, cand, obs.T, w.T, a), 200)
    assert res[0].shape == (6, 3) and res[1].shape == (6, 3, 3) and np.all(res[2]["ess"] >= 1)
    # one spectrum for all rows: M = 1; candidates None: the training inputs
    inputs = np.asarray(gps[0].inputs)
    S0 = np.stack([gp.cpu_predict(inputs, do_unc=False)[0] for gp in gps], axis=1)
    check_wrapper(perband.posterior_bands(gps, None, obs[:, 2], is_gpu=False), _lib.lut_posterior_numpy(S0, inputs, obs[:, 2]), 40)
    with pytest.raises(ValueError):      # a per-row prior is not an offset per candidate
        perband.posterior_bands(gps, cand, obs, w, prior=(np.tile(prior[0], (6, 1)), prior[1]), is_gpu=False)


def test_posterior_many_numpy(small):
    mv, cand, prior, obs = small["mv"], small["cand"], small["prior"], small["obs_mv"]
    rs = np.random.RandomState(2)
    w = 50.0 * rs.uniform(0.5, 2.0, obs.shape)
    w[rs.random_sample(obs.shape) < 0.2] = 0.0
    S = mv.predict_many(cand, is_gpu=False)
    a = _retrieve._prior_term(cand, prior)
    for weights, pr, off in ((None, None, None), (w[0], None, None), (w, prior, a)):
        check_wrapper(mv.posterior_many(cand, obs, weights, prior=pr, is_gpu=False),
                      _lib.lut_posterior_numpy(S, cand, obs, weights, off), 200)
    inputs = np.asarray(mv.emulators[0].inputs)
    check_wrapper(mv.posterior_many(None, obs[3], is_gpu=False),
                  _lib.lut_posterior_numpy(mv.predict_many(inputs, is_gpu=False), inputs, obs[3]), 40)
    with pytest.raises(ValueError):
        mv.posterior_many(cand, obs, space="pc", is_gpu=False)
    with pytest.raises(ValueError):
        mv.posterior_many(cand, obs[:, :5], is_gpu=False)


# ---- the launch plan and the binding -------------------------------------------------------------------------

def test_launch_plan():
    budget = 256 << 20
    for dt in (F64, F32):
        for D in (3, 11, 16):
            geo = _lib.lut_posterior_geometry(D, dt)
            R, LT = geo["rows_per_item"], geo["candidate_tile"]
            terms = 2 + D + D * (D + 1) // 2
            for cu in (256, 8):
                cap = cu * geo["workgroups_per_cu"]
                for L in (4096, 32768, LT, 9):
                    tiles = -(-L // LT)
                    for M in (1, 255, 1000, 100000, 3000000):
                        p = _lib.launch_plan("lut_posterior", dt, M, n_inputs=D, n_candidates=L, compute_units=cu)
                        row_tiles = -(-M // R)
                        assert p["kernel"] == "lut_posterior" and p["rows_per_item"] == R and p["candidate_tile"] == LT
                        assert p["padded_dims"] == geo["padded_dims"]
                        assert p["items"] == row_tiles * p["slices"] and 1 <= p["slices"] <= tiles
                        assert p["workgroups"] == min(p["items"], cap)
                        assert p["slices"] == 1 or p["slices"] * M * terms * 8 <= budget      # the scratch budget
                        search = _lib.launch_plan("lut_search", dt, M, n_terms=12, n_candidates=L, compute_units=cu)
                        assert p["slices"] <= max(1, search["slices"] * (64 // LT) * 2)
    # by hand: 1e5 rows are 391 row tiles on 256 workgroups: ceil(1024 / 391) = 3 slices of the 128 tiles of 32
    p = _lib.launch_plan("lut_posterior", F64, 100000, n_inputs=11, n_candidates=4096)
    assert p["slices"] == 3 and p["items"] == 1173 and p["workgroups"] == 256
    # 3e6 rows x 154 terms x 8 bytes is 3.7 GB a slice: one slice, which needs no scratch
    p = _lib.launch_plan("lut_posterior", F64, 3000000, n_inputs=16, n_candidates=32768, compute_units=32768)
    assert p["slices"] == 1
    # 1e4 rows, 16 dims: the chip would take 26 slices, the budget 21
    p = _lib.launch_plan("lut_posterior", F64, 10000, n_inputs=16, n_candidates=32768)
    assert 1 < p["slices"] <= (256 << 20) // (10000 * 154 * 8) == 21
    for bad in (dict(n_inputs=0, n_candidates=5), dict(n_inputs=17, n_candidates=5), dict(n_inputs=3, n_candidates=0)):
        with pytest.raises(_lib.GpuPredictError):
            _lib.launch_plan("lut_posterior", F64, 10, **bad)


def test_argument_errors_without_a_context():
    lib = _lib.load()
    args = [_lib.GP_F64, None, 1, 1, None, None, 1, 1, None, 0, 0, None, 1, 1, 3] + [None] * 6 + [1, 1, 1, 0]
    assert lib.gp_lut_posterior_device(None, *args) == -1 and lib.gp_last_error_string().decode() == "null context"
    r = ctypes.c_int()
    assert lib.gp_lut_posterior_geometry(_lib.GP_F64, 11, None, None, None, ctypes.byref(r), None) == 0 and r.value == 12
    assert lib.gp_lut_posterior_geometry(7, 11, None, None, None, None, None) == -1                # bad dtype: GP_ERR_INVALID
    assert lib.gp_lut_posterior_geometry(_lib.GP_F64, 17, None, None, None, None, None) not in (0, -1)   # GP_ERR_UNSUPPORTED
