"""The per-band misfit with the emulators' variance in the data term, without a GPU: the numpy branch of
perband.misfit_bands(emulator_unc=True) and retrieve_bands(emulator_unc=True) against the 80-bit truth of
band_unc_cases.py, the four rules of the data term, the sharding logic, and a check of the GPU tests' own cases."""
import os
import re

import numpy as np
import pytest

import band_unc_cases as bc
from band_unc_cases import LD
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, _lib, perband

CPU_CASES = [(40, 3, 5, 1e-1, 33), (250, 10, 7, 1e-1, 21)]          # (n, d, E, nugget, M)


def unc(gps, X, obs, w, second_order="gauss_newton", return_residual=True, **kw):
    return perband.misfit_bands(gps, X, obs, w, second_order=second_order, return_residual=return_residual, is_gpu=False,
                                emulator_unc=True, **kw)


@pytest.fixture(scope="module", params=CPU_CASES, ids=lambda c: "%d-%d-%d" % c[:3])
def case(request):
    n, d, E, nugget, M = request.param
    gps, t, obs, w = bc.inputs(n, d, E, nugget)
    return gps, t[-M:], obs[:, -M:], w[:, -M:]           # (the last rows: the four outside the box among them)


def test_numpy_branch_against_the_longdouble_truth(case):
    gps, X, obs, w = case
    got = unc(gps, X, obs, w)
    ref = bc.truth(*bc.terms_ld(gps, X), obs, w)
    for name, g in zip(("cost", "grad", "gn", "wr", "weff"), got):
        err = gp_oracle.maxnorm_err(ref[name][0].astype(np.float64), g)
        print("numpy branch against longdouble, %s: %.3g" % (name, err))
        assert err <= 1e-11, (name, err)
    assert np.all(got[0] >= 0)
    # shared vectors are those vectors repeated; no weights are ones
    M, E = X.shape[0], len(gps)
    for a, b in zip(unc(gps, X, obs[:, 0], w[:, 0]), unc(gps, X, np.repeat(obs[:, :1], M, 1), np.repeat(w[:, :1], M, 1))):
        assert np.array_equal(a, b)
    for a, b in zip(unc(gps, X, obs, None), unc(gps, X, obs, np.ones(E))):
        assert np.array_equal(a, b)
    assert len(unc(gps, X, obs, w, None, False)) == 2 and len(unc(gps, X, obs, w, None, True)) == 4


def test_gradient_against_central_differences_of_the_longdouble_cost(case):
    gps, X, obs, w = case
    grad = unc(gps, X, obs, w)[1]
    h = LD(2) ** -24
    num = np.empty(X.shape, LD)
    for q in range(X.shape[1]):
        step = np.zeros(X.shape[1], LD)
        step[q] = h
        cp = bc.truth(*bc.terms_ld(gps, X.astype(LD) + step), obs, w)["cost"][0]
        cm = bc.truth(*bc.terms_ld(gps, X.astype(LD) - step), obs, w)["cost"][0]
        num[:, q] = (cp - cm) / (2 * h)
    err = gp_oracle.maxnorm_err(num.astype(np.float64), grad)
    print("gradient against central differences: %.3g" % err)
    assert err <= 1e-6      # (truncation h^2 f''' / 6 ~ 6e-16 x the third derivative's scale; 7e-9 measured on (40, 3, 5))


def test_gn_is_symmetric_and_psd(case):
    gps, X, obs, w = case
    gn = unc(gps, X, obs, w)[2]
    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))
    ev = np.linalg.eigvalsh(gn)
    assert np.all(ev[:, 0] >= -1e-12 * ev[:, -1])


def test_zero_weight_bands_contribute_exactly_nothing(case):
    gps, X, obs, w = case
    assert len(gps) >= 3
    keep = [e for e in range(len(gps)) if e not in (1, len(gps) - 1)]
    w0 = w.copy()
    w0[1] = 0.0
    w0[-1] = 0.0
    got = unc(gps, X, obs, w0)
    ref = unc([gps[e] for e in keep], X, obs[keep], w[keep])
    for a, b in zip(got[:3], ref[:3]):
        assert np.array_equal(a, b)
    assert np.all(got[3][[1, -1]] == 0) and np.all(got[4][[1, -1]] == 0)


def bench_gps(n, d, E, M):
    """Emulators of ``gp_oracle.benchmark_inputs``: their random invQ drives every variance far below 0."""
    gps = []
    for e in range(E):
        inputs, testing, th, invQ, iqt = gp_oracle.benchmark_inputs(n * 31 + d + (e if e else 0), n, d, M)
        if e == 0:
            shared, rows = inputs, testing
        gp = GaussianProcess(shared, [])
        gp.theta, gp.invQ, gp.invQt = th, invQ, iqt
        gps.append(gp)
    return gps, rows


def test_all_negative_variances_give_the_plain_misfit():
    gps, X = bench_gps(40, 9, 5, 33)
    assert all(np.all(gp.cpu_predict(X)[1] < 0) for gp in gps)
    rs = np.random.RandomState(3)
    obs, w = rs.random_sample((5, 33)), 0.5 + rs.random_sample((5, 33))
    got = unc(gps, X, obs, w)
    ref = perband.misfit_bands(gps, X, obs, w, second_order="gauss_newton", return_residual=True, is_gpu=False)
    for a, b in zip(got[:4], ref):
        assert gp_oracle.maxnorm_err(b, a) <= 1e-12
    assert np.array_equal(got[4], w)


def test_far_rows_have_the_closed_form(case):
    gps, X, obs, w = case
    far = X + 1e4
    cost, grad, gn, wr, weff = unc(gps, far, obs, w)
    b = np.array([np.exp(gp.theta[gp.D]) for gp in gps])[:, None]
    assert np.all(grad == 0) and np.all(gn == 0)
    ref = 0.5 * (w * obs ** 2 / (1 + w * b) + np.log1p(w * b)).sum(0)
    assert gp_oracle.maxnorm_err(ref, cost) <= 1e-14
    # a NaN row is NaN throughout, the others unchanged
    bad = X.copy()
    bad[2, -1] = np.nan
    got, ref = unc(gps, bad, obs, w), unc(gps, X, obs, w)
    ok = np.arange(X.shape[0]) != 2
    for g, r in zip(got[:3], ref[:3]):
        assert np.all(np.isnan(g[2])) and np.array_equal(g[ok], r[ok])
    for g, r in zip(got[3:], ref[3:]):
        assert np.all(np.isnan(g[:, 2])) and np.array_equal(g[:, ok], r[:, ok])


@pytest.mark.parametrize("n_dev", [1, 2, 3])
def test_emulator_sharding_through_misfit_fn(case, n_dev):
    gps, X, obs, w = case
    calls = []

    def fn(device, gps_block, X, obs_block, weights_block, second_order, return_residual, **kw):
        calls.append((device, len(gps_block), kw))
        return perband.misfit_bands(gps_block, X, obs_block, weights_block, second_order, return_residual, is_gpu=False, **kw)
    ref = unc(gps, X, obs, w)
    got = unc(gps, X, obs, w, devices=list(range(n_dev)), misfit_fn=fn)
    assert sum(c[1] for c in calls) == len(gps) and all(c[2] == {"emulator_unc": True} for c in calls)
    assert len(got) == 5
    for r, g in zip(ref[:3], got[:3]):
        assert gp_oracle.maxnorm_err(r, g) <= 1e-12
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[4], ref[4])
    # an existing hook without the keyword keeps working when the flag is off
    old = lambda device, g, X, o, ww, so, rr: perband.misfit_bands(g, X, o, ww, so, rr, is_gpu=False)      # noqa: E731
    got = perband.misfit_bands(gps, X, obs, w, devices=[0, 1], misfit_fn=old)
    ref = perband.misfit_bands(gps, X, obs, w, is_gpu=False)
    assert gp_oracle.maxnorm_err(ref[0], got[0]) <= 1e-12


def test_full_second_order_raises(case):
    gps, X, obs, w = case
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, X, obs, w, second_order="full", is_gpu=False, emulator_unc=True)
    with pytest.raises(ValueError):
        perband.retrieve_bands(gps, X, obs, w, second_order="full", is_gpu=False, emulator_unc=True)
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, X, obs, w, second_order="full", emulator_unc=True, misfit_fn=lambda *a, **k: None)


def test_retrieve_bands_numpy_branch():
    gps, X0, obs, w, bounds = bc.retrieval_inputs(40, 3, 5)
    cost0 = unc(gps, X0, obs, w, None, False)[0]
    run = lambda k, **kw: perband.retrieve_bands(gps, X0, obs, w, bounds=bounds, is_gpu=False, emulator_unc=True,   # noqa: E731
                                                 max_iter=k, **kw)
    runs = [run(k) for k in (0, 1, 2, 3, 4, 6, 9)]
    assert np.array_equal(runs[0][1], cost0) and np.array_equal(runs[0][0], X0)
    for a, b in zip(runs, runs[1:]):
        assert np.all(b[1] <= a[1]) and np.all(b[3] >= a[3])
    assert runs[-1][3].max() >= 2
    plain = perband.retrieve_bands(gps, X0, obs, w, bounds=bounds, is_gpu=False, max_iter=9)
    assert not np.array_equal(plain[1], runs[-1][1])                    # (the flag does change the data term)
    out = run(9, return_cov=True, return_A=True)
    cov, sigma, status, A = out[5], out[6], out[7], out[8]
    good = status == 0
    assert good.sum() >= good.size // 2
    eye = np.einsum("mij,mjk->mik", cov[good], A[good])
    assert np.max(np.abs(eye - np.eye(X0.shape[1]))) <= 1e-8
    assert np.allclose(sigma[good] ** 2, np.einsum("mii->mi", cov[good]))
    # A is the Fisher matrix at the returned X
    gn = unc(gps, out[0], obs, w, "gauss_newton", False)[2]
    moved = out[3] > 0
    assert gp_oracle.maxnorm_err(gn[moved], A[moved]) <= 1e-12


@pytest.mark.parametrize("n,d,E,nugget", bc.GPU_CASES + [bc.CLAMPED_CASE], ids=lambda v: str(v))
def test_the_gpu_tests_cases(n, d, E, nugget):
    """A float64 restatement of the fold's chain on a stand-in slab (the numpy branches' per-emulator arrays, rounded to
    the precision under test) stays within HALF the fold bound, and outside the deliberately clamped case at most 5 %
    of the (emulator, row) pairs have v <= 0."""
    gps, t, obs, w = bc.inputs(n, d, E, nugget)
    M = 83
    t, obs, w = t[-M:], obs[:, -M:], w[:, -M:]
    slab64 = bc.terms_f64(gps, t)
    for prec in ((np.float32,) if (n, d, E, nugget) == bc.CLAMPED_CASE else (np.float64, np.float32)):
        slab = tuple(a.astype(prec) for a in slab64)
        o, ww = obs.astype(prec), w.astype(prec)
        frac = float(np.mean(slab[2] <= 0))
        if (n, d, E, nugget) == bc.CLAMPED_CASE:
            print("clamped case: %.1f %% of the pairs have v <= 0" % (100 * frac))
        else:
            assert frac <= 0.05, frac
        ref = bc.truth(*slab, o, ww)
        got = bc.chain(*slab, o, ww, prec)
        for name in ("cost", "grad", "gn", "wr", "weff"):
            x = bc.excess(got[name], *ref[name], E, prec, scale=0.5)
            print("%s %s: %.3f of half the bound" % (np.dtype(prec).name, name, x))
            assert x <= 1.0, (prec, name, x)


def test_new_symbol_is_declared_exported_and_bound():
    name = "gp_band_misfit_unc_device"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(bc.ROOT, "include", "gp_predict_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in gp_predict_hip.h" % name
    assert hasattr(_lib.load(), name)
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_int and len(args) == len(m.group(1).split(","))
    assert hasattr(_lib.BatchModel, "misfit_unc") and hasattr(_lib.BatchModel, "misfit_unc_device")
