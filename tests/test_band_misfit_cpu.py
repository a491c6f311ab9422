"""perband.misfit_bands without a GPU: the numpy branch (the plain statement of the formulas), the sharding logic
with ``misfit_fn`` in place of the HIP path, and the boundary (ctypes signatures, C99 header) of the two new symbols.

Gates: 1e-5 for central differences of the cost at a step of 1e-4 of the training range (the step and gate of
tests/test_misfit_cpu.py; measured 2.6e-8 here); the same gate and step for ``hess`` against central differences of
``grad`` (measured 2.4e-8); 1e-12 between the sharded and the unsharded float64 sums (another order of the same
additions)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from gp_emulator_amd import GaussianProcess, _lib, perband


def maxnorm(ref, got):
    return np.max(np.abs(np.asarray(got) - ref)) / np.max(np.abs(ref))


def make_gps(E, N=30, D=4, seed=8):
    rs = np.random.RandomState(seed)
    inputs = rs.random_sample((N, D))
    gps = []
    for e in range(E):
        r = np.random.RandomState(100 + e)
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQt = r.random_sample(D + 2), r.random_sample(N)
        gps.append(gp)
    return gps


@pytest.fixture(scope="module")
def case():
    """E = 5 emulators, M = 9 rows; observations = the emulators' own means at other rows; per-row weights."""
    gps = make_gps(5)
    rs = np.random.RandomState(3)
    X, X2 = rs.random_sample((9, 4)), rs.random_sample((9, 4))
    obs = np.stack([gp.cpu_predict(X2, do_unc=False)[0] for gp in gps])
    w = 0.5 + rs.random_sample((5, 9))
    return gps, X, obs, w


def test_gradient_against_central_differences(case):
    gps, X, obs, w = case
    rng = np.ptp(np.asarray(gps[0].inputs), axis=0)
    cost, grad = perband.misfit_bands(gps, X, obs, w, is_gpu=False)
    fd = np.empty_like(grad)
    for d in range(X.shape[1]):
        h = 1e-4 * rng[d]
        Xp, Xm = X.copy(), X.copy()
        Xp[:, d] += h
        Xm[:, d] -= h
        fd[:, d] = (perband.misfit_bands(gps, Xp, obs, w, is_gpu=False)[0]
                    - perband.misfit_bands(gps, Xm, obs, w, is_gpu=False)[0]) / (2 * h)
    err = maxnorm(fd, grad)
    print("band misfit gradient against central differences: %.3g" % err)
    assert err <= 1e-5


def test_full_second_order_against_central_differences_of_the_gradient(case):
    """hess = gn + sum_e w r H_e is the derivative of grad: central differences of grad at the same step, gate 1e-5
    (measured 2.4e-8: the truncation error h^2/6 |grad'''| / |hess| of a smooth squared-exponential mean).  gn alone
    must NOT pass that gate here (the residuals are of the order of the means), or the test would not see the
    curvature term."""
    gps, X, obs, w = case
    cost, grad, hess = perband.misfit_bands(gps, X, obs, w, second_order="full", is_gpu=False)
    gn = perband.misfit_bands(gps, X, obs, w, second_order="gauss_newton", is_gpu=False)[2]
    rng = np.ptp(np.asarray(gps[0].inputs), axis=0)
    fd = np.empty_like(hess)
    for d in range(X.shape[1]):
        h = 1e-4 * rng[d]
        Xp, Xm = X.copy(), X.copy()
        Xp[:, d] += h
        Xm[:, d] -= h
        fd[:, :, d] = (perband.misfit_bands(gps, Xp, obs, w, is_gpu=False)[1]
                       - perband.misfit_bands(gps, Xm, obs, w, is_gpu=False)[1]) / (2 * h)
    err, err_gn = maxnorm(fd, hess), maxnorm(fd, gn)
    print("band misfit hess against central differences of grad: %.3g (gn alone: %.3g)" % (err, err_gn))
    assert err <= 1e-5
    assert err_gn > 1e-3
    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))


def test_shapes_and_broadcasting(case):
    gps, X, obs, w = case
    E, (M, D) = len(gps), X.shape
    out = perband.misfit_bands(gps, X, obs, w, second_order="full", return_residual=True, is_gpu=False)
    assert [a.shape for a in out] == [(M,), (M, D), (M, D, D), (E, M)]
    assert len(perband.misfit_bands(gps, X, obs, is_gpu=False)) == 2
    assert len(perband.misfit_bands(gps, X, obs, return_residual=True, is_gpu=False)) == 3
    # the formulas, once more, from the parts
    mu = np.stack([gp.cpu_predict(X, do_unc=False)[0] for gp in gps])
    dmu = np.stack([gp.cpu_predict(X, do_unc=False)[1] for gp in gps])
    r = mu - obs
    assert np.allclose(out[0], 0.5 * np.sum(w * r * r, axis=0), rtol=1e-13, atol=0)
    assert np.allclose(out[1], np.einsum("em,emd->md", w * r, dmu), rtol=1e-12, atol=1e-15)
    assert np.array_equal(out[3], w * r)
    # (E,) observations and weights are those vectors repeated for every row; no weights are ones
    o1, w1 = obs[:, 0], w[:, 0]
    a = perband.misfit_bands(gps, X, o1, w1, second_order="full", return_residual=True, is_gpu=False)
    b = perband.misfit_bands(gps, X, np.repeat(o1[:, None], M, 1), np.repeat(w1[:, None], M, 1), second_order="full",
                             return_residual=True, is_gpu=False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    a = perband.misfit_bands(gps, X, o1, None, second_order="gauss_newton", is_gpu=False)
    b = perband.misfit_bands(gps, X, o1, np.ones(E), second_order="gauss_newton", is_gpu=False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # mixed: shared observations, per-row weights
    a = perband.misfit_bands(gps, X, o1, w, is_gpu=False)
    b = perband.misfit_bands(gps, X, np.repeat(o1[:, None], M, 1), w, is_gpu=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def numpy_fn(calls):
    def fn(device, gps_block, X, obs_block, weights_block, second_order, return_residual):
        calls.append((device, len(gps_block), np.shape(obs_block), None if weights_block is None else np.shape(weights_block)))
        return perband.misfit_bands(gps_block, X, obs_block, weights_block, second_order, return_residual, is_gpu=False)
    return fn


@pytest.mark.parametrize("n_dev", [1, 2, 3])
@pytest.mark.parametrize("shared", [False, True], ids=["per-row", "shared"])
def test_emulator_sharding_reproduces_the_unsharded_sum(case, n_dev, shared):
    gps, X, obs, w = case
    E, M = len(gps), X.shape[0]
    if shared:
        obs, w = obs[:, 0], w[:, 0]
    ref = perband.misfit_bands(gps, X, obs, w, second_order="full", return_residual=True, is_gpu=False)
    calls = []
    got = perband.misfit_bands(gps, X, obs, w, second_order="full", return_residual=True,
                               devices=list(range(10, 10 + n_dev)), misfit_fn=numpy_fn(calls))
    assert [c[0] for c in sorted(calls)] == list(range(10, 10 + n_dev)) and sum(c[1] for c in calls) == E
    for c in calls:           # every block gets its own rows of obs and weights, in the caller's shape
        assert c[2] == c[3] == ((c[1],) if shared else (c[1], M))
    assert len(got) == 4
    for r, g in zip(ref[:3], got[:3]):
        assert g.shape == r.shape and maxnorm(r, g) <= 1e-12
    assert np.array_equal(got[3], ref[3])
    # without the optional outputs, and without weights
    got = perband.misfit_bands(gps, X, obs, devices=list(range(n_dev)), misfit_fn=numpy_fn([]))
    ref = perband.misfit_bands(gps, X, obs, is_gpu=False)
    assert len(got) == 2 and maxnorm(ref[0], got[0]) <= 1e-12 and maxnorm(ref[1], got[1]) <= 1e-12
    # more devices than emulators: the empty blocks are skipped
    got = perband.misfit_bands(gps[:2], X, obs[:2], devices=[0, 1, 2], misfit_fn=numpy_fn([]))
    ref = perband.misfit_bands(gps[:2], X, obs[:2], is_gpu=False)
    assert maxnorm(ref[0], got[0]) <= 1e-12 and maxnorm(ref[1], got[1]) <= 1e-12


def test_bad_arguments_raise(case):
    gps, X, obs, w = case
    fn = numpy_fn([])
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, X, obs[:4], is_gpu=False)
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, X, obs[:, :5], is_gpu=False)
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, X, obs, w[:, :5], misfit_fn=fn)
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, X, obs, second_order="newton", is_gpu=False)
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, X[:, :3], obs, is_gpu=False)
    with pytest.raises(ValueError):
        perband.misfit_bands([], X, obs, is_gpu=False)
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, X, obs, devices=[], misfit_fn=fn)

    def broken(device, gps_block, *rest):
        raise RuntimeError("shard %d failed" % device)
    with pytest.raises(RuntimeError, match="shard"):
        perband.misfit_bands(gps, X, obs, devices=[0, 1], misfit_fn=broken)


NEW_SYMBOLS = ("gp_band_misfit_device", "gp_band_misfit_host")


def test_new_symbols_are_declared_exported_and_bound():
    """The two entry points are in the header (outside comments), in the library and in the ctypes table, with one
    ctypes argument per declared parameter."""
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in gp_predict_hip.h" % name
        assert hasattr(lib, name), "libgp_predict_hip.so does not export %s" % name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(args) == len(m.group(1).split(","))
    assert hasattr(_lib.BatchModel, "misfit") and hasattr(_lib.BatchModel, "misfit_device")


def test_new_symbols_link_from_c99(tmp_path):
    """A strict C99 program that names both functions compiles against the header and links against the library;
    called with null handles they fail with GP_ERR_INVALID and a message, touching no GPU."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "band.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "gp_predict_hip.h"\n'
        "int main(void) {\n"
        "  double x = 0;\n"
        "  int rc = gp_band_misfit_device(NULL, NULL, &x, &x, 1, 0, NULL, 0, 0, &x, &x, NULL, NULL, NULL, 1);\n"
        "  if (rc != GP_ERR_INVALID || strlen(gp_last_error_string()) == 0) return 2;\n"
        "  rc = gp_band_misfit_host(NULL, NULL, GP_F64, &x, &x, 1, 0, NULL, 0, 0, &x, &x, NULL, NULL, NULL, 1);\n"
        "  if (rc != GP_ERR_INVALID || strlen(gp_last_error_string()) == 0) return 3;\n"
        "  return 0;\n}\n")
    exe = tmp_path / "band"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH),
                    "-Wl,-rpath," + libdir], check=True, timeout=120)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
