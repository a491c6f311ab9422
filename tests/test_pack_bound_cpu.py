"""The host-side bound that replaces the exp clamp of the fp64 fused predict kernel.

Real<double>::exp_ needs |argument| log2e < 2^31.  The kernel guards every test row; the host guarantees
|x''_i|^2 / 2 <= 2^26 for every packed training point (x'' = sqrt(e)(x - centre); the derivation is beside
Real<double>::kFarG in gp_predict_kernel.hpp) by refusing an emulator that holds a point farther out.  The general-
shape kernel and float32 keep a clamp (or __expf) and take any point."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401
from gp_emulator_amd import _lib

LIMIT = 2.0 ** 13.5          # length scales from the training mean


def packed(far, prec=np.float64, n=250, d=11):
    """n points of which the last lies `far` length scales (e = 1) along dimension 0 from the others."""
    rs = np.random.RandomState(5)
    x = rs.random_sample((n, d))
    x[-1, 0] += far
    return _lib.pack_model(np.ones(d + 2), x, np.zeros(n), np.zeros((n, n)), prec)


def test_bound_is_enforced_for_the_fp64_fused_kernel():
    pk = packed(0.99 * LIMIT)                  # (the mean moves by far / n: the point is far * (n - 1) / n out)
    assert pk["kernel_nb"] > 0
    h = pk["xa"].reshape(-1, 16)[:, 12]
    assert h.min() >= -(2.0 ** 26) and np.all(np.isfinite(pk["xa"]))
    with pytest.raises(_lib.GpuPredictError, match="length scales"):
        packed(1.02 * LIMIT * 250 / 249)


def test_other_kernels_take_any_point():
    assert packed(1e6, np.float32)["kernel_nb"] > 0        # fp32: difference form and __expf
    assert packed(1e6, np.float64, n=400, d=4)["kernel_nb"] == 0     # general-shape kernel: clamped exp
