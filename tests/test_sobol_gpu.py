"""gp_sobol_batch_f64 on the GPU -- sobol_pair_kernel<8 | 12 | 16> and sobol_fold_kernel -- and the Python layer above it.

The kernels are held to the quadrature truth of sobol_cases.py inside its gates (16 x the worse of two float64 numpy
evaluations, floor 16, cap 1024, in units of u S), their reproducibility is checked bit for bit, and -7.25e300
sentinels lie behind every output of every call made through ``call``.  Every test here needs the entry, the binding or
the methods, none of which exist before this feature."""
import numpy as np
import pytest

import sobol_cases as sc

from gp_emulator_amd import _lib, _sobol_numpy as sn, perband
from gp_emulator_amd.GaussianProcess import GaussianProcess
from gp_emulator_amd.multivariate_gp import MultivariateEmulator

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4


def call(expX, x, alpha, lo, hi, pairs=None, n_pairs=None, want_rc=False):
    """The C entry itself on arrays with eight sentinels behind each output: (mean (B, E), cov (B, P, 1 + 2D)), or with
    ``want_rc`` (status, mean, cov) without a check of the status."""
    ctx = _lib.default_context(0)
    expX = np.ascontiguousarray(np.atleast_2d(expX), dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    alpha = np.ascontiguousarray(np.atleast_2d(alpha), dtype=np.float64)
    E, (N, D) = expX.shape[0], x.shape
    lo, hi = (np.ascontiguousarray(np.atleast_2d(np.asarray(v, dtype=np.float64))) for v in (lo, hi))
    B = lo.shape[0]
    if pairs is not None:
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    P = n_pairs if n_pairs is not None else (E if pairs is None else pairs.shape[0])
    mean, cov = np.full(B * E + 8, SENTINEL), np.full(B * P * (1 + 2 * D) + 8, SENTINEL)
    rc = ctx.lib.gp_sobol_batch_f64(ctx.h, E, _lib._ptr(expX), _lib._ptr(x), _lib._ptr(alpha), N, D, B, _lib._ptr(lo),
                                    _lib._ptr(hi), P, None if pairs is None else _lib._ptr(pairs), _lib._ptr(mean),
                                    _lib._ptr(cov))
    assert np.all(mean[-8:] == SENTINEL) and np.all(cov[-8:] == SENTINEL), "a sentinel behind an output was overwritten"
    if want_rc:
        return rc, mean, cov
    _lib.check(rc, "gp_sobol_batch_f64")
    return mean[:-8].reshape(B, E), cov[:-8].reshape(B, P, 1 + 2 * D)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


PQ, UNIT, THREE, CASES, case = sc.PQ, sc.UNIT, sc.THREE, sc.CASES, sc.case


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_truth(gpu_lib, name):
    """mean and [V, Vm, Vt] of the pairs (0, 0), (0, 1), (1, 1) -- p = q and p != q with different theta -- inside the gate
    of every family, in every box of the case."""
    args = case(name)
    tr, g = sc.truth(name, *args, PQ), sc.gates(name, *args, PQ)
    mean, cov = call(*args, pairs=PQ)
    print(name, "yardsticks", g["a"], g["b"], "device", sc.units(mean, cov, tr))
    assert not sc.within(mean, cov, tr, g["gate"])
    # the indices of the two emulators inside the propagated gates
    S, ST, gS, gST = sc.index_gates(tr, g["gate"])
    first, total, _ = sn.indices(cov[:, [0, 2]])
    assert np.all(np.abs(first - S[:, [0, 2]].astype(np.float64)) <= gS[:, [0, 2]] + 2 * sc.U * np.abs(first))
    assert np.all(np.abs(total - ST[:, [0, 2]].astype(np.float64)) <= gST[:, [0, 2]] + 2 * sc.U * np.abs(total))


def test_default_pairs_are_the_emulators_themselves(gpu_lib):
    args = case("n33_d2_boxes")
    mean, cov = call(*args)
    mean2, cov2 = call(*args, pairs=[[0, 0], [1, 1]])
    assert same_bits(mean, mean2) and same_bits(cov, cov2)


def test_bit_for_bit_alone_in_a_batch_permuted_and_twice(gpu_lib):
    """A (box, pair) result does not depend on what else the call holds, on the order of the pairs, or on the call."""
    expX, x, alpha, lo, hi = case("n33_d11")
    m1, c1 = call(expX, x, alpha, lo, hi, pairs=[[0, 0], [0, 1], [1, 0], [1, 1]])
    m2, c2 = call(expX, x, alpha, lo, hi, pairs=[[0, 0], [0, 1], [1, 0], [1, 1]])
    assert same_bits(m1, m2) and same_bits(c1, c2)
    perm = [2, 0, 3, 1]
    _, cp = call(expX, x, alpha, lo, hi, pairs=np.array([[0, 0], [0, 1], [1, 0], [1, 1]])[perm])
    assert same_bits(cp, c1[:, perm])
    for k, (p, q) in enumerate([[0, 0], [0, 1], [1, 0], [1, 1]]):
        ms, cs = call(expX[[p, q]], x, alpha[[p, q]], lo, hi, pairs=[[0, 1]])
        assert same_bits(cs[:, 0], c1[:, k]) and same_bits(ms[:, 0], m1[:, p]) and same_bits(ms[:, 1], m1[:, q])
    # one emulator alone, default pairs
    ms, cs = call(expX[1], x, alpha[1], lo, hi)
    assert same_bits(cs[:, 0], c1[:, 3]) and same_bits(ms[:, 0], m1[:, 1])


def test_three_boxes_in_one_call_are_three_calls(gpu_lib):
    expX, x, alpha, lo, hi = case("n16_d7_boxes")
    m3, c3 = call(expX, x, alpha, lo, hi, pairs=PQ)
    for k in range(3):
        m1, c1 = call(expX, x, alpha, lo[k], hi[k], pairs=PQ)
        assert same_bits(m1[0], m3[k]) and same_bits(c1[0], c3[k])


def test_past_two_rounds_of_the_persistent_grid(gpu_lib):
    """More items than two rounds of the grid, with a ragged tail: four emulators at N = 33, D = 2 (three j-blocks, the
    last of one row) in a list of all their 16 ordered pairs repeated.  Every entry is held to the truth and to the
    numpy branch, entries of one pair are the same bits wherever they stand, and a sample is single-pair calls."""
    n, d = 33, 2
    expX, x, alpha = sc.stack([sc.emulator(n, d, k) for k in range(4)])
    lo, hi = UNIT(d)
    cu = _lib.default_context(0).device_info()["compute_units"]
    cap = _lib.launch_plan("sobol", np.float64, 1, n_train=n, n_inputs=d, n_emulators=1 << 20, compute_units=cu)["workgroups"]
    unique = np.array([(p, q) for p in range(4) for q in range(4)], dtype=np.int32)
    n_pairs = (2 * cap) // 3 + 7
    pairs = unique[(np.arange(n_pairs) * 5 + 3) % 16]
    plan = _lib.launch_plan("sobol", np.float64, 1, n_train=n, n_inputs=d, n_emulators=n_pairs, compute_units=cu)
    assert plan["kernel"] == "sobol" and plan["items"] == 3 * n_pairs and plan["workgroups"] == cap
    assert plan["items"] > 2 * cap and plan["items"] % cap != 0
    mean, cov = call(expX, x, alpha, lo, hi, pairs=pairs)
    key = "grid_n33_d2"
    tr, g = sc.truth(key, expX, x, alpha, lo, hi, unique), sc.gates(key, expX, x, alpha, lo, hi, unique)
    first = np.array([np.flatnonzero((pairs == u).all(axis=1))[0] for u in unique])
    assert not sc.within(mean, cov[:, first], tr, g["gate"])
    mn, cn = sn.sobol_pairs_numpy(expX, x, alpha, lo, hi, unique)
    slack = {f: g["gate"][f] * (1 + 1.0 / sc.MARGIN) for f in sc.FAMILIES}      # the numpy branch's own error on top
    tn = dict(tr, mean=mn[None].astype(sc.LD), cov=cn[None].astype(sc.LD))
    assert not sc.within(mean, cov[:, first], tn, slack)
    which = (pairs[:, 0] * 4 + pairs[:, 1])
    assert same_bits(cov[0], cov[0, first][which])
    for k in (0, 1, cap // 3, n_pairs // 2, n_pairs - 1):
        p, q = pairs[k]
        _, cs = call(expX[[p, q]], x, alpha[[p, q]], lo, hi, pairs=[[0, 1]])
        assert same_bits(cs[0, 0], cov[0, k])


def test_non_finite_emulators_poison_their_pairs_only(gpu_lib):
    """A NaN in one emulator's theta and an infinity in another's alpha: their means and every pair they are part of are
    NaN, every other output is bit for bit the call without them."""
    n, d = 33, 11
    expX, x, alpha = sc.stack([sc.emulator(n, d, k) for k in range(4)])
    lo, hi = THREE(d)
    pairs = np.array([(p, q) for p in range(4) for q in range(4)], dtype=np.int32)
    m0, c0 = call(expX, x, alpha, lo, hi, pairs=pairs)
    assert np.all(np.isfinite(m0)) and np.all(np.isfinite(c0))
    bad_e, bad_a = expX.copy(), alpha.copy()
    bad_e[1, 4] = np.nan
    bad_a[3, 20] = np.inf
    m1, c1 = call(bad_e, x, bad_a, lo, hi, pairs=pairs)
    hit = np.isin(pairs, (1, 3)).any(axis=1)
    assert np.all(np.isnan(c1[:, hit])) and np.all(np.isnan(m1[:, [1, 3]]))
    assert same_bits(c1[:, ~hit], c0[:, ~hit]) and same_bits(m1[:, [0, 2]], m0[:, [0, 2]])
    # an infinite length scale parameter and a NaN alpha in the first row of a block
    bad_e, bad_a = expX.copy(), alpha.copy()
    bad_e[0, 0] = np.inf
    bad_a[2, 16] = np.nan
    m2, c2 = call(bad_e, x, bad_a, lo, hi, pairs=pairs)
    hit = np.isin(pairs, (0, 2)).any(axis=1)
    assert np.all(np.isnan(c2[:, hit])) and np.all(np.isnan(m2[:, [0, 2]]))
    assert same_bits(c2[:, ~hit], c0[:, ~hit]) and same_bits(m2[:, [1, 3]], m0[:, [1, 3]])


def test_error_returns_leave_the_outputs_untouched(gpu_lib):
    expX, x, alpha, lo, hi = case("n33_d2_boxes")

    def refused(code, *a, **k):
        rc, mean, cov = call(*a, want_rc=True, **k)
        assert rc == code, _lib.load().gp_last_error_string()
        assert np.all(mean == SENTINEL) and np.all(cov == SENTINEL)

    h = hi.copy()
    h[1, 0] = lo[1, 0]
    refused(GP_ERR_INVALID, expX, x, alpha, lo, h, pairs=PQ)                      # hi <= lo
    h[1, 0] = lo[1, 0] - 1.0
    refused(GP_ERR_INVALID, expX, x, alpha, lo, h, pairs=PQ)
    for v in (np.nan, np.inf):
        h = hi.copy()
        h[2, 1] = v
        refused(GP_ERR_INVALID, expX, x, alpha, lo, h, pairs=PQ)                  # a non-finite bound
        l_ = lo.copy()
        l_[0, 0] = -v
        refused(GP_ERR_INVALID, expX, x, alpha, l_, hi, pairs=PQ)
    refused(GP_ERR_INVALID, expX, x, alpha, lo, hi, pairs=[[0, 0], [0, 2]])       # a pair index out of range
    refused(GP_ERR_INVALID, expX, x, alpha, lo, hi, pairs=[[-1, 0]])
    refused(GP_ERR_INVALID, expX, x, alpha, lo, hi, pairs=None, n_pairs=3)        # no list: n_pairs is n_emulators
    e17 = np.ones((2, 19))
    refused(GP_ERR_UNSUPPORTED, e17, np.zeros((4, 17)), np.ones((2, 4)), np.zeros(17), np.ones(17))       # D = 17
    refused(GP_ERR_UNSUPPORTED, np.ones((1, 3)), np.zeros((513, 1)), np.ones((1, 513)), [0.0], [1.0])     # N above the limit


# ---- the Python layer --------------------------------------------------------------------------------------

def gps_of(ems):
    out = []
    for m in ems:
        gp = GaussianProcess(m["inputs"], np.zeros(m["n"]))
        gp.theta, gp.invQt = np.log(m["expX"]), m["invQt"]
        out.append(gp)
    return out


def test_sobol_bands_and_sobol_indices_are_the_batch(gpu_lib):
    """perband.sobol_bands(is_gpu=True) is Context.sobol_batch on the stacked constants, bit for bit, and
    gp.sobol_indices(is_gpu=True) is the batch's row; 1-D bounds carry no box axis."""
    n, d = 33, 11
    ems = [sc.emulator(n, d, k) for k in range(3)]
    gps = gps_of(ems)
    expX = np.stack([np.exp(gp.theta) for gp in gps])            # (what the layer itself forms from theta)
    lo, hi = THREE(d)
    ctx = _lib.default_context(0)
    for bounds in ((lo, hi), (lo[1], hi[1])):
        mean, cov = ctx.sobol_batch(expX, ems[0]["inputs"], np.stack([m["invQt"] for m in ems]), *bounds)
        assert mean.shape == np.shape(bounds[0])[:-1] + (3,) and cov.shape == np.shape(bounds[0])[:-1] + (3, 1 + 2 * d)
        mc, cc = call(expX, ems[0]["inputs"], np.stack([m["invQt"] for m in ems]), *bounds)
        assert same_bits(mean, mc.reshape(mean.shape)) and same_bits(cov, cc.reshape(cov.shape))
        first, total, variance = sn.indices(cov)
        r = perband.sobol_bands(gps, bounds, is_gpu=True)
        assert same_bits(r.first, first) and same_bits(r.total, total) and same_bits(r.variance, variance)
        assert same_bits(r.mean, mean) and r.first.shape == mean.shape + (d,)
        one = gps[1].sobol_indices(bounds, is_gpu=True)
        assert same_bits(one.first, first[..., 1, :]) and same_bits(one.total, total[..., 1, :])
        assert same_bits(one.variance, variance[..., 1]) and same_bits(one.mean, mean[..., 1])


def small_mv(n=24, d=3, P=3, K=40):
    """A MultivariateEmulator built from arrays: P trained-like per-PC emulators and a seeded basis."""
    ems = [sc.emulator(n, d, k) for k in range(P)]
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    mv.n_pcs = P
    mv.basis_functions = np.random.RandomState(77).standard_normal((P, K))
    mv.emulators = gps_of(ems)
    return mv, ems


def test_multivariate_sobol_against_the_numpy_branch_and_the_truth(gpu_lib):
    mv, ems = small_mv()
    d, P = 3, 3
    lo, hi = np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3])
    args = sc.stack(ems) + (lo, hi)
    pairs = sn.upper_pairs(P)
    tr, g = sc.truth("mv_small", *args, pairs), sc.gates("mv_small", *args, pairs)
    st = sc.spectral_truth(mv.basis_functions, tr, P, g["gate"])
    dev, host = mv.sobol((lo, hi), is_gpu=True), mv.sobol((lo, hi), is_gpu=False)
    assert dev.first.shape == (d, 40) and dev.total.shape == (d, 40) and dev.variance.shape == (40,) and dev.mean.shape == (40,)
    own = 1 + 1.0 / sc.MARGIN                                   # (the numpy branch's own error on top of the gate)
    for name in ("first", "total", "variance", "mean"):
        got, ref, gate = getattr(dev, name), getattr(host, name), st["g_" + name]
        t = st[name].astype(np.float64)
        assert np.all(np.abs(got - t) <= gate + 4 * sc.U * np.abs(t)), name
        assert np.all(np.abs(got - ref) <= own * gate + 4 * sc.U * np.abs(t)), name
    # two boxes: a leading axis, the first box the call above bit for bit
    two = mv.sobol((np.stack([lo, lo - 0.5]), np.stack([hi, hi + 0.5])), is_gpu=True)
    assert two.first.shape == (2, d, 40) and two.mean.shape == (2, 40)
    assert np.all(np.abs(two.first[0] - dev.first) <= st["g_first"]) and np.all(np.abs(two.variance[0] - dev.variance) <= st["g_variance"])
