"""gp_moments_batch_f64 on the GPU -- moments_prepare_kernel, moments_mean_kernel<8 | 12 | 16>,
moments_pair_kernel<8 | 12 | 16> -- and the Python layer above it.

The kernels are held to the longdouble truth of moments_cases.py inside its gates (16 x the worse of two float64 numpy
evaluations, floor 16, cap 1024, in units of u S) and to the numpy branch inside twice the gate, their reproducibility
is checked bit for bit, and -7.25e300 sentinels lie behind every output of every call made through ``call``.  Every
test here needs the entry, the binding or the methods, none of which exist before this feature.

Measured (profiles/r20_moments.txt): the device's errors are 0.09 to 1.1 u S over every family of every case here, the
yardsticks' 0.06 to 2.3 u S, so every gate is the floor of 16."""
import numpy as np
import pytest

import moments_cases as mc

from gp_emulator_amd import _lib, _moments_numpy as mn, perband
from gp_emulator_amd.GaussianProcess import GaussianProcess
from gp_emulator_amd.multivariate_gp import MultivariateEmulator

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4


def call(expX, x, alpha, invQ, m, S, pairs=None, n_pairs=None, want_rc=False, grad=True):
    """The C entry itself on arrays with eight sentinels behind each output: (mean (M, E), egrad (M, E, D), cov (M, P),
    evar (M, E) or None, info (M,)), or with ``want_rc`` (status, raw outputs) without a check of the status."""
    ctx = _lib.default_context(0)
    expX = np.ascontiguousarray(np.atleast_2d(expX), dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    alpha = np.ascontiguousarray(np.atleast_2d(alpha), dtype=np.float64)
    E, (N, D) = expX.shape[0], x.shape
    if invQ is not None:
        invQ = np.ascontiguousarray(np.asarray(invQ, dtype=np.float64).reshape(E, N, N))
    m, S = mn.rows_arrays(m, S, D)
    M = m.shape[0]
    if pairs is not None:
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    P = n_pairs if n_pairs is not None else (E if pairs is None else pairs.shape[0])
    mean, egrad, cov, evar = (np.full(n + 8, SENTINEL) for n in (M * E, M * E * D, M * P, M * E))
    info = np.full(M + 8, -77, np.int32)
    ptr = _lib._ptr
    rc = ctx.lib.gp_moments_batch_f64(ctx.h, E, ptr(expX), ptr(x), ptr(alpha), None if invQ is None else ptr(invQ), N, D, M,
                                      ptr(m), ptr(S), P, None if pairs is None else ptr(pairs), ptr(mean),
                                      ptr(egrad) if grad else None, ptr(cov), None if invQ is None else ptr(evar), ptr(info))
    for o in (mean, egrad, cov, evar):
        assert np.all(o[-8:] == SENTINEL), "a sentinel behind an output was overwritten"
    assert np.all(info[-8:] == -77)
    if want_rc:
        return rc, (mean, egrad, cov, evar, info)
    _lib.check(rc, "gp_moments_batch_f64")
    return (mean[:-8].reshape(M, E), egrad[:-8].reshape(M, E, D) if grad else None, cov[:-8].reshape(M, P),
            None if invQ is None else evar[:-8].reshape(M, E), info[:-8])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else a.dtype),
                                                 b.view(np.uint64 if b.dtype == np.float64 else b.dtype))


def all_same(a, b):
    return all((u is None and v is None) or same_bits(u, v) for u, v in zip(a, b))


def check_case(key, args, m, S, pairs, with_invQ=True):
    """The device inside the gate against the truth and inside twice the gate against the numpy branch."""
    expX, x, alpha, invQ = args
    invQ = invQ if with_invQ else None
    tr = mc.truth(key, expX, x, alpha, invQ, m, S, pairs)
    g = mc.gates(key, expX, x, alpha, invQ, m, S, pairs)
    got = call(expX, x, alpha, invQ, m, S, pairs)
    print(key, "yardsticks", g["a"], g["b"], "device", mc.units(got, tr))
    assert np.array_equal(got[4], tr["info"])
    assert not mc.within(got, tr, g["gate"])
    host = mn.moments_pairs_numpy(expX, x, alpha, invQ, m, S, pairs)
    assert not mc.within(got, mc.as_truth(host, tr), g["gate"], factor=2.0)
    return got


SHAPES = [(37, 3), (250, 11), (300, 13)]      # DM = 8, 12, 16; a ragged N; two column steps at N > 256


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("rows", [1, 5])
def test_kernel_against_the_truth_and_the_numpy_branch(gpu_lib, n, d, rows):
    """The upper pairs of three emulators with invQ (V for p = q and p != q, Ev, mean, gradient), and the default pairs
    without invQ, in every instance."""
    args = mc.stack([mc.emulator(n, d, k) for k in range(3)])
    m, S = mc.rows(rows, d)
    got = check_case(("gpu", n, d, rows, "upper"), args, m, S, mn.upper_pairs(3))
    assert np.all(np.isfinite(got[3]))
    dflt = check_case(("gpu", n, d, rows, "default"), args, m, S, None, with_invQ=False)
    assert dflt[3] is None
    # the per-emulator results do not depend on the pair list, the pairs not on invQ
    assert same_bits(dflt[0], got[0]) and same_bits(dflt[1], got[1]) and same_bits(dflt[2], got[2][:, [0, 3, 5]])


def test_small_sigma_keeps_its_digits(gpu_lib):
    """Sigma scaled by 1e-8 (s = 1e-4), where alpha' Q alpha - M^2 is at 1e-6 relative error in any precision: V inside
    the gate, i.e. to about 16 u S."""
    n, d = 37, 3
    args = mc.stack([mc.emulator(n, d, k) for k in range(2)])
    m, S = mc.rows(3, d, s=1e-4)
    got = check_case(("gpu", "small"), args, m, S, [[0, 0], [0, 1], [1, 1]])
    tr = mc.truth(("gpu", "small"), args[0], args[1], args[2], args[3], m, S, [[0, 0], [0, 1], [1, 1]])
    assert np.all(np.abs(got[2] - tr["cov"].astype(np.float64)) <= 1e-9 * np.abs(tr["cov"].astype(np.float64)))
    naive = float(mc.naive_ld(args[0], args[1], args[2], m[0], S[0], 0, 1))
    print("naive form in longdouble: relative error %.3g" % abs(naive / float(tr["cov"][0, 1]) - 1))


def test_past_two_rounds_of_the_persistent_grid(gpu_lib):
    """N = 37, the 15 pairs of five emulators, and enough rows that the (row, pair) items pass two rounds of the grid
    with a ragged tail: every entry against the truth and the numpy branch, a sample against single-item calls."""
    n, d = 37, 3
    args = mc.stack([mc.emulator(n, d, k) for k in range(5)])
    pairs = mn.upper_pairs(5)
    cu = _lib.default_context(0).device_info()["compute_units"]
    cap = _lib.launch_plan("moments", np.float64, 1, n_train=n, n_inputs=d, n_emulators=1 << 20, compute_units=cu)["workgroups"]
    rows = (2 * cap) // 15 + 2
    plan = _lib.launch_plan("moments", np.float64, rows, n_train=n, n_inputs=d, n_emulators=15, compute_units=cu)
    assert plan["kernel"] == "moments" and plan["items"] == 15 * rows and plan["workgroups"] == cap
    assert plan["items"] > 2 * cap and plan["items"] % cap != 0
    m, S = mc.rows(rows, d, seed=3)
    got = check_case(("gpu", "grid", rows), args, m, S, pairs)
    for r, k in ((0, 0), (1, 14), (rows // 2, 7), (rows - 1, 14), (rows - 1, 0)):
        p, q = pairs[k]
        one = call(args[0][[p, q]], args[1], args[2][[p, q]], args[3][[p, q]], m[r], S[r], [[0, 1]])
        assert same_bits(one[2][0, 0], got[2][r, k])
        assert same_bits(one[0][0], got[0][r, [p, q]]) and same_bits(one[1][0], got[1][r, [p, q]])


def test_bit_for_bit_alone_in_a_batch_permuted_and_twice(gpu_lib):
    """A (row, pair) result does not depend on what else the call holds, on the order of the pairs, or on the call."""
    n, d = 250, 11
    args = mc.stack([mc.emulator(n, d, k) for k in range(2)])
    m, S = mc.rows(3, d, seed=1)
    pairs = np.array([[0, 0], [0, 1], [1, 0], [1, 1]])
    a, b = call(*args, m, S, pairs), call(*args, m, S, pairs)
    assert all_same(a, b)
    perm = [2, 0, 3, 1]
    c = call(*args, m, S, pairs[perm])
    assert same_bits(c[2], a[2][:, perm]) and same_bits(c[0], a[0]) and same_bits(c[1], a[1]) and same_bits(c[3], a[3])
    for r in range(3):
        one = call(*args, m[r], S[r], pairs)
        assert all(same_bits(u[0], v[r]) for u, v in zip(one[:4], a[:4]))
    solo = call(args[0][1], args[1], args[2][1], args[3][1], m, S)           # one emulator alone, default pairs
    assert same_bits(solo[2][:, 0], a[2][:, 3]) and same_bits(solo[0][:, 0], a[0][:, 1]) and same_bits(solo[3][:, 0], a[3][:, 1])
    nograd = call(*args, m, S, pairs, grad=False)
    assert same_bits(nograd[0], a[0]) and same_bits(nograd[2], a[2])


def test_invalid_rows_leave_the_others_bit_identical(gpu_lib):
    """NaN, indefinite and Sigma = 0 rows mixed into a batch: NaN and info where they are due, V == 0 exactly at
    Sigma = 0 with predict's values, every other row bit for bit the call without them."""
    n, d = 37, 3
    args = mc.stack([mc.emulator(n, d, k) for k in range(2)])
    expX, x, alpha, invQ = args
    pairs = [[0, 0], [0, 1], [1, 1]]
    m, S = mc.rows(7, d, seed=2)
    clean = call(*args, m, S, pairs)
    m2, S2 = m.copy(), S.copy()
    m2[1, 2] = np.nan
    S2[2, 1, 0] = np.inf
    S2[3] = np.diag([0.04, -1e-3, 0.02])                     # pivot 1 negative
    S2[4] = 0.0
    S2[5, 0, 2] = np.nan                                      # the upper triangle is not read
    got = call(*args, m2, S2, pairs)
    assert list(got[4]) == [0, -1, -1, 2, 0, 0, 0]
    for o in got[:4]:
        assert np.all(np.isnan(o[[1, 2, 3]]))
    for o, c in zip(got[:4], clean[:4]):
        assert same_bits(o[[0, 5, 6]], c[[0, 5, 6]])
    assert np.all(got[2][4] == 0.0)
    from oracle import gp_oracle
    for e in range(2):
        mu, var, deriv = gp_oracle.cpu_predict(x, np.log(expX[e]), invQ[e], alpha[e], m[4:5])
        k = gp_oracle.kernel_rows(x, np.log(expX[e]), m[4:5])[:, 0]
        assert abs(got[0][4, e] - mu[0]) <= 1e-12 * np.abs(alpha[e] * k).sum()
        assert abs(got[3][4, e] - var[0]) <= 1e-12 * (expX[e, d] + np.abs(invQ[e] * np.outer(k, k)).sum())
        mag = expX[e, :d] * (np.abs(alpha[e] * k)[:, None] * np.abs(x - m[4])).sum(axis=0)
        assert np.all(np.abs(got[1][4, e] - deriv[0]) <= 1e-12 * mag)


def test_non_finite_emulators_poison_their_pairs_only(gpu_lib):
    n, d = 37, 3
    args = mc.stack([mc.emulator(n, d, k) for k in range(4)])
    expX, x, alpha, invQ = args
    pairs = np.array([(p, q) for p in range(4) for q in range(4)], dtype=np.int32)
    m, S = mc.rows(2, d)
    clean = call(*args, m, S, pairs)
    assert all(np.all(np.isfinite(o)) for o in clean[:4])
    e2, a2, q2 = expX.copy(), alpha.copy(), invQ.copy()
    e2[1, 1] = np.nan
    q2[3, 5, 7] = np.inf
    got = call(e2, x, a2, q2, m, S, pairs)
    hit = np.isin(pairs, (1, 3)).any(axis=1)
    assert np.all(np.isnan(got[2][:, hit])) and all(np.all(np.isnan(o[:, [1, 3]])) for o in (got[0], got[1], got[3]))
    assert same_bits(got[2][:, ~hit], clean[2][:, ~hit])
    assert all(same_bits(o[:, [0, 2]], c[:, [0, 2]]) for o, c in zip((got[0], got[1], got[3]), (clean[0], clean[1], clean[3])))
    e2, a2 = expX.copy(), alpha.copy()
    e2[0, d] = np.inf
    a2[2, 36] = np.nan
    got = call(e2, x, a2, invQ, m, S, pairs)
    hit = np.isin(pairs, (0, 2)).any(axis=1)
    assert np.all(np.isnan(got[2][:, hit])) and same_bits(got[2][:, ~hit], clean[2][:, ~hit])
    assert same_bits(got[0][:, [1, 3]], clean[0][:, [1, 3]]) and np.all(np.isnan(got[0][:, [0, 2]]))


def test_error_returns_leave_the_outputs_untouched(gpu_lib):
    n, d = 37, 3
    args = mc.stack([mc.emulator(n, d, k) for k in range(2)])
    m, S = mc.rows(2, d)

    def refused(code, *a, **k):
        rc, outs = call(*a, want_rc=True, **k)
        assert rc == code, _lib.load().gp_last_error_string()
        assert all(np.all(o == SENTINEL) for o in outs[:4]) and np.all(outs[4] == -77)

    refused(GP_ERR_INVALID, *args, m, S, [[0, 0], [0, 2]])
    refused(GP_ERR_INVALID, *args, m, S, [[-1, 0]])
    refused(GP_ERR_INVALID, *args, m, S, None, n_pairs=3)
    refused(GP_ERR_UNSUPPORTED, np.ones((1, 19)), np.zeros((4, 17)), np.ones((1, 4)), None, np.zeros((1, 17)), np.eye(17))
    refused(GP_ERR_UNSUPPORTED, np.ones((1, 3)), np.zeros((513, 1)), np.ones((1, 513)), None, np.zeros((1, 1)), np.eye(1))


# ---- the Python layer --------------------------------------------------------------------------------------

def gps_of(ems):
    out = []
    for m in ems:
        gp = GaussianProcess(m["inputs"], np.zeros(m["n"]))
        gp.theta, gp.invQt, gp.invQ = np.log(m["expX"]), m["invQt"], m["invQ"]
        out.append(gp)
    return out


def small_mv(n=37, d=3, P=3, K=40):
    ems = [mc.emulator(n, d, k) for k in range(P)]
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    mv.n_pcs = P
    mv.basis_functions = np.random.RandomState(77).standard_normal((P, K))
    mv.emulators = gps_of(ems)
    return mv, ems


def test_the_three_wrappers_against_their_numpy_branches(gpu_lib):
    n, d = 37, 3
    mv, ems = small_mv(n, d)
    gps = mv.emulators
    m, S = mc.rows(4, d, seed=5)
    args = (np.stack([np.exp(gp.theta) for gp in gps]),) + mc.stack(ems)[1:]
    key = ("gpu", "wrappers")
    tr = mc.truth(key, *args, m, S, mn.upper_pairs(3))
    gate = mc.gates(key, *args, m, S, mn.upper_pairs(3))["gate"]
    diag = [0, 3, 5]
    tol = {"mean": 2 * gate["mean"] * mc.U * tr["S_mean"].astype(np.float64).T,
           "var_state": 2 * gate["V"] * mc.U * tr["S_cov"].astype(np.float64)[:, diag].T,
           "var_emulator": 2 * gate["Ev"] * mc.U * tr["S_evar"].astype(np.float64).T,
           "expected_grad": 2 * gate["grad"] * mc.U * tr["S_grad"].astype(np.float64).transpose(1, 0, 2)}
    dev, host = perband.predict_uncertain_bands(gps, m, S, is_gpu=True), perband.predict_uncertain_bands(gps, m, S, is_gpu=False)
    assert dev.mean.shape == (3, 4) and dev.expected_grad.shape == (3, 4, d) and np.array_equal(dev.info, host.info)
    for name, t in tol.items():
        assert np.all(np.abs(getattr(dev, name) - getattr(host, name)) <= t), name
    one = gps[1].predict_uncertain(m, S, is_gpu=True)
    for name in tol:
        assert same_bits(getattr(one, name), getattr(dev, name)[1]), name
    shared = gps[1].predict_uncertain(m, S[0], is_gpu=True)                  # one (D, D) covariance for all rows
    assert same_bits(shared.mean[0], one.mean[0]) and same_bits(shared.var_state[0], one.var_state[0])
    sd, sh = mv.predict_uncertain(m, S, is_gpu=True, return_pc=True), mv.predict_uncertain(m, S, is_gpu=False, return_pc=True)
    B = np.abs(mv.basis_functions)
    Sc = mn.mirror(tr["S_cov"].astype(np.float64)[..., None], 3)[..., 0]
    assert sd.mean.shape == (4, 40) and sd.pc_cov.shape == (4, 3, 3)
    assert np.all(np.abs(sd.mean - sh.mean) <= 2 * gate["mean"] * mc.U * (tr["S_mean"].astype(np.float64) @ B))
    assert np.all(np.abs(sd.var_state - sh.var_state) <= 2 * gate["V"] * mc.U * np.einsum("pk,mpq,qk->mk", B, Sc, B))
    assert np.all(np.abs(sd.var_emulator - sh.var_emulator) <= 2 * gate["Ev"] * mc.U * (tr["S_evar"].astype(np.float64) @ (B * B)))
