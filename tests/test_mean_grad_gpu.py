"""Mean and gradient without the variance (gp_predict_mean_grad_*) on a real MI355X.

The no-variance instances run phase A from the same source as the full kernels, so every mu and
deriv here must equal the full call's BIT FOR BIT, on every kernel form (latency, throughput,
general shape), route (device, direct, staged, page-locked) and caller (Model, BatchModel,
GaussianProcess, perband, MultivariateEmulator).  Parity with the oracle is checked at the gates
test_gpu_parity.py uses for the full path.
"""
import ctypes

import numpy as np
import pytest

from conftest import SYNTHETIC_CASES, load_golden, synthetic_case
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, _lib, perband

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
ROW, DMAJ = _lib.GP_DERIV_ROWMAJOR, _lib.GP_DERIV_DMAJOR


@pytest.fixture(autouse=True, params=["latency-kernel", "throughput-kernel"])
def kernel_form(request, monkeypatch):
    """Both forms: GP_NO_FEW=1 sends calls of up to 512 row tiles to the throughput kernel."""
    if request.param == "throughput-kernel":
        monkeypatch.setenv("GP_NO_FEW", "1")
    else:
        monkeypatch.delenv("GP_NO_FEW", raising=False)
    return request.param


def make_gp(g, with_invq=True):
    gp = GaussianProcess(g["inputs"], [])
    gp.theta, gp.invQt = g["theta"], g["invQt"]
    if with_invq:
        gp.invQ = g["invQ"]
    return gp


def model(g, precision, with_invq=True):
    return _lib.Model(_lib.default_context(0), np.exp(g["theta"]), g["inputs"], g["invQt"],
                      g["invQ"] if with_invq else None, precision)


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def errs(ref, got):
    return [gp_oracle.maxnorm_err(r, x) for r, x in zip(ref, got)]


# (model precision, host row dtype): fp64, fp32, float32 arithmetic on float64 rows
PRECS = [(np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64)]


@pytest.mark.parametrize("prec,host", PRECS)
@pytest.mark.parametrize("name", SYNTHETIC_CASES + ["prosail_pc0"])
def test_fixture_bitwise_and_parity(gpu_lib, name, prec, host):
    g = load_golden(name) if name == "prosail_pc0" else synthetic_case(name)
    m = model(g, prec)
    testing = np.ascontiguousarray(g["testing"], dtype=host)
    mu, var, der = m.predict(testing)
    mu2, der2 = m.predict_mean_grad(testing)
    same(mu2, mu)
    same(der2, der)
    if name == "prosail_pc0" and prec == np.float32:
        return       # (float32 on the real emulator: test_gpu_parity.py's own looser gates apply)
    e = errs((g["mu"], g["deriv"]), (mu2, der2))
    assert max(e) <= TOL[prec], (name, e)


@pytest.mark.parametrize("M", [1, 15, 16, 17, 63, 64, 65, 127, 129, 1000])
def test_ragged_rows_both_layouts(gpu_lib, M):
    g = synthetic_case("c2_n250_d11")
    for prec in (np.float64, np.float32):
        m = model(g, prec)
        t = np.ascontiguousarray(g["testing"][:M], dtype=prec)
        for layout in (ROW, DMAJ):
            mu, var, der = m.predict(t, deriv_layout=layout)
            mu2, der2 = m.predict_mean_grad(t, deriv_layout=layout)
            same(mu2, mu)
            same(der2, der)


def test_empty_call(gpu_lib):
    g = synthetic_case("c1_n100_d5")
    m = model(g, np.float64)
    mu, der = m.predict_mean_grad(g["testing"][:0])
    assert mu.shape == (0,) and der.shape == (0, 5)
    m.predict_mean_grad_device(0, 0, 0, 0)          # M = 0: nothing to do, no pointer is read


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("M", [5, 130, 1999])
def test_device_call_writes_only_its_rows(gpu_lib, prec, M):
    """Sentinels around mu and deriv on the device: nothing outside [0, M) is written."""
    g = synthetic_case("c2_n250_d11")
    ctx = _lib.default_context(0)
    m = model(g, prec)
    t = np.ascontiguousarray(g["testing"][:M], dtype=prec)
    D, pad = t.shape[1], 256
    sentinel = np.full(pad + M * D + pad, 7.25, dtype=prec)
    d_t = ctx.to_device(t)
    d_mu = ctx.to_device(sentinel[:pad + M + pad].copy())
    d_der = ctx.to_device(sentinel.copy())
    isz = np.dtype(prec).itemsize
    try:
        for layout in (ROW, DMAJ):
            m.predict_mean_grad_device(d_t, ctypes.c_void_p(d_mu.value + pad * isz),
                                       ctypes.c_void_p(d_der.value + pad * isz), M, layout)
            ctx.synchronize()
            mu = ctx.to_host(d_mu, (pad + M + pad,), prec)
            der = ctx.to_host(d_der, (pad + M * D + pad,), prec)
            assert np.all(mu[:pad] == 7.25) and np.all(mu[pad + M:] == 7.25)
            assert np.all(der[:pad] == 7.25) and np.all(der[pad + M * D:] == 7.25)
            ref_mu, _, ref_der = m.predict(t, deriv_layout=layout)
            same(mu[pad:pad + M], ref_mu)
            same(der[pad:pad + M * D].reshape(ref_der.shape), ref_der)
    finally:
        for p in (d_t, d_mu, d_der):
            ctx.free(p)


@pytest.mark.parametrize("prec,host", PRECS)
def test_host_routes(gpu_lib, prec, host):
    """direct (small M), staged slabs (several, ragged last one), page-locked arrays."""
    N, D, M = 250, 11, 70001
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(77, N, D, M)
    g = dict(inputs=inputs, testing=testing, theta=theta, invQ=invQ, invQt=invQt)
    m = model(g, prec)
    t = np.ascontiguousarray(testing, dtype=host)
    for rows, mbr in ((300, 0), (M, 9000), (M, 0)):
        for layout in (ROW, DMAJ):
            mu, var, der = m.predict(t[:rows], deriv_layout=layout, max_block_rows=mbr)
            mu2, der2 = m.predict_mean_grad(t[:rows], deriv_layout=layout, max_block_rows=mbr)
            same(mu2, mu)
            same(der2, der)
    if host == prec:      # page-locked caller arrays (one emulator, row-major gradient)
        ctx = m.ctx
        tp = ctx.pinned_empty((M, D), prec)
        tp[:] = t
        mu_p, der_p = ctx.pinned_empty((M,), prec), ctx.pinned_empty((M, D), prec)
        m.predict_mean_grad(tp, out=(mu_p, der_p))
        mu, var, der = m.predict(t)
        same(mu_p, mu)
        same(der_p, der)


@pytest.mark.parametrize("prec", [np.float64, np.float32])
def test_model_without_invq(gpu_lib, prec):
    g = synthetic_case("c2_n250_d11")
    t = np.ascontiguousarray(g["testing"], dtype=prec)
    full = model(g, prec).predict_mean_grad(t)
    bare = model(g, prec, with_invq=False)
    got = bare.predict_mean_grad(t)
    same(got[0], full[0])
    same(got[1], full[1])
    with pytest.raises(_lib.GpuPredictError):
        bare.predict(t)                                   # the full predict still needs invQ
    # batched, E = 3
    ctx = _lib.default_context(0)
    e = np.exp(g["theta"])
    args = (ctx, np.stack([e] * 3), g["inputs"], np.stack([g["invQt"]] * 3))
    bw = _lib.BatchModel(*args, np.stack([g["invQ"]] * 3), prec).predict_mean_grad(t)
    bb = _lib.BatchModel(*args, None, prec).predict_mean_grad(t)
    same(bb[0], bw[0])
    same(bb[1], bw[1])
    for k in range(3):
        same(bb[0][k], full[0])
        same(bb[1][k], full[1])
    # GaussianProcess without invQ
    gp = make_gp(g, with_invq=False)
    mu, der = gp.gpu_predict(g["testing"], prec, 2e5, do_unc=False)
    full_gp = make_gp(g).gpu_predict(g["testing"], prec, 2e5, do_unc=False)
    same(mu, full_gp[0])
    same(der, full_gp[1])


@pytest.mark.parametrize("prec", [np.float64, np.float32])
def test_batched_emulators(gpu_lib, prec):
    N, D, M, E = 250, 11, 777, 7
    rs = np.random.RandomState(42)
    inputs, testing = rs.random_sample((N, D)), rs.random_sample((M, D))
    th, iq, iqt = [], [], []
    for e in range(E):
        r = np.random.RandomState(100 + e)
        th.append(r.random_sample(D + 2))
        iq.append(r.random_sample((N, N)))
        iqt.append(r.random_sample(N))
    b = _lib.BatchModel(_lib.default_context(0), np.exp(np.stack(th)), inputs, np.stack(iqt), np.stack(iq), prec)
    t = np.ascontiguousarray(testing, dtype=prec)
    for layout in (ROW, DMAJ):
        mu, var, der = b.predict(t, deriv_layout=layout)
        mu2, der2 = b.predict_mean_grad(t, deriv_layout=layout)
        same(mu2, mu)
        same(der2, der)
    mu2, der2 = b.predict_mean_grad(t)
    for e in range(E):
        ref = gp_oracle.cpu_predict(inputs, th[e], iq[e], iqt[e], testing)
        assert max(errs((ref[0], ref[2]), (mu2[e], der2[e]))) <= TOL[prec], e


@pytest.mark.parametrize("N,D", [(321, 16), (400, 4), (20, 17), (640, 30), (1024, 64)])
def test_general_shape_kernel(gpu_lib, N, D):
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(500 + N + D, N, D, 333)
    g = dict(inputs=inputs, testing=testing, theta=theta, invQ=invQ, invQt=invQt)
    for prec in (np.float64, np.float32):
        m = model(g, prec)
        t = np.ascontiguousarray(testing, dtype=prec)
        for layout in (ROW, DMAJ):
            mu, var, der = m.predict(t, deriv_layout=layout)
            mu2, der2 = m.predict_mean_grad(t, deriv_layout=layout)
            same(mu2, mu)
            same(der2, der)
        bare = model(g, prec, with_invq=False).predict_mean_grad(t)
        same(bare[0], m.predict(t)[0])


@pytest.mark.parametrize("N,D", [(16, 2), (17, 4), (33, 7), (112, 8), (113, 9), (129, 12),
                                 (192, 13), (257, 16), (304, 3), (320, 16)])
def test_every_kernel_size_class(gpu_lib, N, D):
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(900 + N + D, N, D, 321)
    g = dict(inputs=inputs, testing=testing, theta=theta, invQ=invQ, invQt=invQt)
    ref = gp_oracle.cpu_predict(inputs, theta, invQ, invQt, testing)
    for prec in (np.float64, np.float32):
        m = model(g, prec)
        t = np.ascontiguousarray(testing, dtype=prec)
        mu, var, der = m.predict(t)
        mu2, der2 = m.predict_mean_grad(t)
        same(mu2, mu)
        same(der2, der)
        assert max(errs((ref[0], ref[2]), (mu2, der2))) <= TOL[prec]


@pytest.mark.parametrize("prec", [np.float64, np.float32])
def test_full_size_c2_device_resident(gpu_lib, prec):
    N, D, M = 250, 11, 1_000_000
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(3, N, D, M)
    g = dict(inputs=inputs, testing=testing, theta=theta, invQ=invQ, invQt=invQt)
    ctx = _lib.default_context(0)
    m = model(g, prec)
    t = np.ascontiguousarray(testing, dtype=prec)
    isz = np.dtype(prec).itemsize
    d_t = ctx.to_device(t)
    bufs = [ctx.malloc(M * isz), ctx.malloc(M * isz), ctx.malloc(M * D * isz), ctx.malloc(M * isz), ctx.malloc(M * D * isz)]
    try:
        m.predict_device(d_t, bufs[0], bufs[1], bufs[2], M)
        m.predict_mean_grad_device(d_t, bufs[3], bufs[4], M)
        ctx.synchronize()
        mu, der = ctx.to_host(bufs[0], (M,), prec), ctx.to_host(bufs[2], (M, D), prec)
        mu2, der2 = ctx.to_host(bufs[3], (M,), prec), ctx.to_host(bufs[4], (M, D), prec)
    finally:
        for p in [d_t] + bufs:
            ctx.free(p)
    same(mu2, mu)
    same(der2, der)
    idx = np.random.RandomState(5).choice(M, 2000, replace=False)
    ref = gp_oracle.cpu_predict(inputs, theta, invQ, invQt, testing[idx])
    assert max(errs((ref[0], ref[2]), (mu2[idx], der2[idx]))) <= TOL[prec]


@pytest.mark.parametrize("prec", [np.float64, np.float32])
def test_gaussianprocess_gpu_predict_do_unc(gpu_lib, prec):
    g = synthetic_case("c2_n250_d11")
    gp = make_gp(g)
    testing = g["testing"]
    M = testing.shape[0]
    mu, der = gp.gpu_predict(testing, prec, 2e5, do_unc=False)
    assert mu.dtype == np.float64 and der.dtype == np.float64
    assert mu.shape == (M,) and der.shape == (M, 11)
    fmu, fvar, fder = gp.gpu_predict(testing, prec, 2e5)
    same(mu, fmu)
    same(der, fder)
    if prec == np.float64:
        cmu, cder = gp.cpu_predict(testing, do_unc=False)
        assert gp_oracle.maxnorm_err(cmu, mu) <= 1e-10
        assert gp_oracle.maxnorm_err(cder, der) <= 1e-10
    # the reference API is unchanged: predict(do_unc=False, is_gpu=True) still gives three arrays
    out = gp.predict(testing, do_unc=False, is_gpu=True, precision=prec)
    assert len(out) == 3


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("M", [1, 2000])
def test_multivariate_emulator_equals_full_path_rebuilt(gpu_lib, prec, M):
    """predict_many / predict(is_gpu=True) now run the mean+gradient kernels; they must equal the
    full batched predict's mu / deriv passed through the same reconstruction kernel."""
    from gp_emulator_amd import MultivariateEmulator
    g = load_golden("prosail_mv")
    X = g["train_data"].T @ g["basis_functions"]
    mv = MultivariateEmulator(X=X, y=g["y_train"], hyperparams=g["hyperparams"],
                              basis_functions=g["basis_functions"], n_pcs=int(g["n_pcs"]))
    rs = np.random.RandomState(9)
    lo, hi = g["y_train"].min(0), g["y_train"].max(0)
    Y = lo + (hi - lo) * rs.random_sample((M, lo.size))
    fwd, jac = mv.predict_many(Y, precision=prec, do_deriv=True)
    fwd_only = mv.predict_many(Y, precision=prec)
    same(fwd_only, fwd)
    if M == 1 and prec == np.float64:
        f1, j1 = mv.predict(Y[0], is_gpu=True)
        same(f1, fwd[0])
        same(j1, jac[0])
        same(mv.predict(Y[0], do_deriv=False, is_gpu=True), fwd[0])
    # the full path from its pieces
    st = mv._gpu_state(np.dtype(prec))
    ctx, batch = st["ctx"], st["batch"]
    P, B, D = batch.n_emulators, g["basis_functions"].shape[1], lo.size
    mu, var, der = batch.predict(np.ascontiguousarray(Y, dtype=prec))
    isz = np.dtype(prec).itemsize
    d_mu, d_der = ctx.to_device(np.ascontiguousarray(mu)), ctx.to_device(np.ascontiguousarray(der))
    d_f, d_j = ctx.malloc(M * B * isz), ctx.malloc(M * D * B * isz)
    try:
        ctx.reconstruct_device(np.dtype(prec), st["d_basis"], d_mu, d_f, M, P, B)
        ctx.reconstruct_device(np.dtype(prec), st["d_basis"], d_der, d_j, M * D, P, B)
        ctx.synchronize()
        ref_f = ctx.to_host(d_f, (M, B), prec)
        ref_j = ctx.to_host(d_j, (M, D, B), prec)
    finally:
        for p in (d_mu, d_der, d_f, d_j):
            ctx.free(p)
    same(fwd, ref_f)
    same(jac, ref_j)


def test_predict_bands_do_unc_false(gpu_lib):
    N, D, M, E = 100, 5, 999, 6
    rs = np.random.RandomState(4)
    inputs, testing = rs.random_sample((N, D)), rs.random_sample((M, D))
    gps = []
    for e in range(E):
        r = np.random.RandomState(200 + e)
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQ, gp.invQt = r.random_sample(D + 2), r.random_sample((N, N)), r.random_sample(N)
        gps.append(gp)
    for prec in (np.float64, np.float32):
        mu, var, der = perband.predict_bands(gps, testing, prec)
        out = perband.predict_bands(gps, testing, prec, do_unc=False)
        assert len(out) == 2
        same(out[0], mu)
        same(out[1], der)
