"""The mean+gradient entry points without a GPU: declarations, ctypes signatures, the emulator
sharding of predict_bands(do_unc=False) and the Python argument checks."""
import numpy as np
import pytest

from conftest import synthetic_case

from gp_emulator_amd import GaussianProcess, _lib, perband
from test_abi_cpu import header_functions


def test_new_symbols_are_declared_and_have_signatures():
    names = header_functions()
    for n in ("gp_predict_mean_grad_device", "gp_predict_mean_grad_host"):
        assert n in names
        assert n in _lib.SIGNATURES
        assert hasattr(_lib.load(), n)
    assert len(_lib.SIGNATURES["gp_predict_mean_grad_device"][1]) == 7
    assert len(_lib.SIGNATURES["gp_predict_mean_grad_host"][1]) == 9


def test_predict_bands_without_unc_shards_emulators():
    N, D, M, E = 20, 3, 11, 7
    rs = np.random.RandomState(0)
    inputs, testing = rs.random_sample((N, D)), rs.random_sample((M, D))
    gps = []
    for e in range(E):
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQt = np.full(D + 2, float(e)), np.zeros(N)    # no invQ at all
        gps.append(gp)
    calls = []

    def fake(dev, block, t):
        calls.append((dev, len(block)))
        ids = np.array([gp.theta[0] for gp in block])
        return (np.repeat(ids[:, None], len(t), 1),
                np.repeat(ids[:, None, None], len(t), 1).repeat(t.shape[1], 2) + dev / 10.0)

    out = perband.predict_bands(gps, testing, devices=[0, 1, 2], predict_fn=fake, do_unc=False)
    assert len(out) == 2
    mu, der = out
    assert mu.shape == (E, M) and der.shape == (E, M, D)
    assert np.array_equal(mu[:, 0], np.arange(E))
    from gp_emulator_amd import multi_gpu
    blocks = multi_gpu.row_shards(E, 3)
    assert sorted(calls) == sorted((d, e1 - e0) for d, (e0, e1) in enumerate(blocks) if e1 > e0)
    dev_of = np.rint((der[:, 0, 0] - np.arange(E)) * 10).astype(int)
    assert list(dev_of) == sorted(dev_of)              # contiguous blocks, in device order
    assert set(dev_of) == {0, 1, 2}


class _NoDevice(_lib.Model):
    """A Model whose checks can run without a device (no library handle)."""

    def __init__(self, D, dtype=np.float64):
        self.dtype, self.n_inputs, self.n_train = np.dtype(dtype), D, 10
        self.h = None


def test_argument_checks_need_no_device():
    m = _NoDevice(4)
    with pytest.raises(ValueError):
        m.predict_mean_grad(np.zeros((5, 3)))                    # wrong number of columns
    with pytest.raises(ValueError):
        m.predict_mean_grad(np.zeros(12))                        # not 2-D
    ok = np.zeros((5, 4))
    with pytest.raises(ValueError):
        m.predict_mean_grad(ok, out=(np.zeros(5), np.zeros((5, 4)), np.zeros(5)))      # three arrays
    with pytest.raises(ValueError):
        m.predict_mean_grad(ok, out=(np.zeros(5, np.float32), np.zeros((5, 4))))       # wrong dtype
    with pytest.raises(ValueError):
        m.predict_mean_grad(ok, out=(np.zeros(5), np.zeros((4, 5))))                    # wrong shape
    with pytest.raises(ValueError):
        m.predict_mean_grad(ok, deriv_layout=_lib.GP_DERIV_DMAJOR, out=(np.zeros(5), np.zeros((5, 4))))
    with pytest.raises(ValueError):
        m.predict_mean_grad(ok, out=(np.zeros(5), np.zeros((4, 5)).T))                  # not C-contiguous


def test_batch_model_checks_invq_shape_only_when_given():
    with pytest.raises(ValueError):
        _lib.BatchModel(None, np.ones((2, 5)), np.zeros((6, 3)), np.zeros((2, 6)), np.zeros((2, 5, 5)))
    with pytest.raises(ValueError):
        _lib.BatchModel(None, np.ones((2, 5)), np.zeros((6, 3)), np.zeros((3, 6)), None)


def test_gpu_predict_do_unc_checks_precision():
    g = synthetic_case("odd_n37_d3")
    gp = GaussianProcess(g["inputs"], [])
    gp.theta, gp.invQt = g["theta"], g["invQt"]
    with pytest.raises(TypeError):
        gp.gpu_predict(g["testing"], np.int32, 2e5, do_unc=False)
