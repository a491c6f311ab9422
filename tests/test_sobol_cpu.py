"""Sobol indices without a GPU: the quadrature truth of sobol_cases.py against mpmath, the numpy branch against the
definition of the indices and inside its gates, the properties of the indices, the MultivariateEmulator route, the
launch-plan arithmetic and the error returns that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import sobol_cases as sc

from gp_emulator_amd import _lib, _sobol_numpy as sn, perband
from gp_emulator_amd.GaussianProcess import GaussianProcess
from gp_emulator_amd.multivariate_gp import MultivariateEmulator

LD = sc.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quadrature_against_mpmath():
    """int_a^b exp(-u^2) du of ``gauss_integral`` against mpmath at 40 digits over the intervals the cases produce: boxes
    around the point, boxes far to one side (|u| up to 12), e w^2 from 1e-6 (an interval 1e-3 wide) to 1e4 (70 wide).
    Worst relative difference measured: 1.6e-18 = 2^-59.1; the bound is 2^-56."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    rs = np.random.RandomState(5)
    batches = []
    for sq, lo, hi in ((0.7, 0.0, 1.0), (2.8, 0.0, 1.0), (2.8, 1.5, 2.5), (4.0, 1.5, 2.5), (4.0, -0.5, 1.5), (7.1e-4, 0.0, 1.0),
                       (70.7, 0.0, 1.0), (50.0, 0.0, 1.0), (1.2, 0.2, 0.7), (1.2, -1.0, 3.0)):
        m = np.concatenate([rs.uniform(size=12), [0.0, 1.0]])
        batches.append((sq * (lo - m), sq * (hi - m)))
    worst = 0.0
    for a, b in batches:
        got = sc.gauss_integral(a, b)
        for ai, bi, gi in zip(a, b, got):
            ai, bi = mp.mpf(float(ai)), mp.mpf(float(bi))
            if ai > 0:
                ref = (mp.erfc(ai) - mp.erfc(bi)) * mp.sqrt(mp.pi) / 2
            elif bi < 0:
                ref = (mp.erfc(-bi) - mp.erfc(-ai)) * mp.sqrt(mp.pi) / 2
            else:
                ref = (mp.erf(bi) - mp.erf(ai)) * mp.sqrt(mp.pi) / 2
            hi_, lo_ = float(gi), float(gi - LD(float(gi)))                # the longdouble as two doubles, exactly
            worst = max(worst, float(abs((mp.mpf(hi_) + mp.mpf(lo_)) - ref) / ref))
    print("worst relative difference %.3g = 2^%.1f" % (worst, np.log2(worst)))
    assert worst <= 2.0 ** -56


def test_gauss_legendre_rule_is_exact_where_it_must_be():
    x, w = sc.gauss_legendre(20)
    assert abs(float(w.sum() - 2)) < 1e-18 and abs(float((w * x ** 38).sum() - LD(2) / 39)) < 1e-18


# ---- the definition of the indices -----------------------------------------------------------------------

def tensor_definition(expX, x, alpha, lo, hi, coef=None, n=60):
    """Means and [V, Vm^i, Vt^i] of the functions f_k = sum_p coef[p, k] mu_p (default: the emulators themselves) and of
    all their pairs, from their values on the n^3 tensor Gauss-Legendre grid of the box (D = 3): conditional
    expectations by summing axes out.  Returns (mean (K,), cov (K, K, 7)) in longdouble."""
    E, (N, D) = expX.shape[0], x.shape
    assert D == 3
    z, wz = sc.gauss_legendre(n)
    nodes = [LD(lo[d]) + (LD(hi[d]) - LD(lo[d])) * (z + 1) / 2 for d in range(D)]
    w = wz / 2
    f = []
    for e in range(E):
        g = [np.exp(-LD(expX[e, d]) / 2 * (x[:, d].astype(LD)[:, None] - nodes[d][None, :]) ** 2) for d in range(D)]
        f.append(np.einsum("j,ja,jb,jc->abc", LD(expX[e, D]) * alpha[e].astype(LD), g[0], g[1], g[2]))
    f = np.stack(f)
    if coef is not None:
        f = np.einsum("pk,pabc->kabc", np.asarray(coef, dtype=LD), f)
    K = f.shape[0]
    mean = np.einsum("kabc,a,b,c->k", f, w, w, w)
    cov = np.empty((K, K, 7), LD)
    letters = "abc"
    for p in range(K):
        for q in range(K):
            mm = mean[p] * mean[q]
            cov[p, q, 0] = np.einsum("abc,abc,a,b,c->", f[p], f[q], w, w, w) - mm
            for i in range(3):
                rest = letters.replace(letters[i], "")
                mp_, mq_ = (np.einsum("abc,%s,%s->%s" % (rest[0], rest[1], letters[i]), g_, w, w) for g_ in (f[p], f[q]))
                cov[p, q, 1 + i] = (mp_ * mq_ * w).sum() - mm                                # Cov(E[.|t_i], E[.|t_i])
                cp_, cq_ = (np.einsum("abc,%s->%s" % (letters[i], rest), g_, w) for g_ in (f[p], f[q]))
                cov[p, q, 4 + i] = cov[p, q, 0] - ((cp_ * cq_ * w[:, None] * w[None, :]).sum() - mm)   # V - Cov(E[.|t_~i], ..)
    return mean, cov


def test_numpy_branch_against_the_definition():
    """D = 3, N = 14, two emulators with different theta and their cross pair: every output within 1e-10 |V| of the
    conditional expectations by 60-node tensor Gauss-Legendre (the margin is for the quadrature at the shortest length
    scale and for other seeds; measured: 2.6e-13, printed by the test)."""
    ems = [sc.emulator(14, 3, 0), sc.emulator(14, 3, 1)]
    expX, x, alpha = sc.stack(ems)
    assert not np.allclose(expX[0], expX[1])
    lo, hi = np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3])
    mean_d, cov_d = tensor_definition(expX, x, alpha, lo, hi)
    pairs = [[0, 0], [0, 1], [1, 0], [1, 1]]
    mean, cov = sn.sobol_pairs_numpy(expX, x, alpha, lo, hi, pairs)
    worst = 0.0
    for k, (p, q) in enumerate(pairs):
        worst = max(worst, float(np.max(np.abs(cov[k] - cov_d[p, q]) / np.abs(cov_d[p, q, 0]))))
    print("worst difference relative to |V|: %.3g" % worst)
    assert worst <= 1e-10
    assert np.all(np.abs(mean - mean_d.astype(np.float64)) <= 1e-10 * np.abs(mean_d.astype(np.float64)))
    # and the quadrature truth of the GPU tests says the same
    tr = sc.truth("definition", expX, x, alpha, lo, hi, pairs)
    assert float(np.max(np.abs(tr["cov"][0] - cov_d.reshape(4, 7)) / np.abs(cov_d.reshape(4, 7)[:, :1]))) <= 1e-10


# ---- the numpy branch inside its gates -----------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.CASES))
def test_numpy_branch_and_kernel_form_inside_the_gate(name):
    """Both yardsticks of every case of the kernel tests stay far below the cap (so the gates are theirs, not the cap),
    and the indices they give obey S_i <= ST_i and sum S_i <= 1 inside the propagated gates."""
    args = sc.case(name)
    tr, g = sc.truth(name, *args, sc.PQ), sc.gates(name, *args, sc.PQ)
    print(name, "a", g["a"], "b", g["b"])
    mean, cov = sn.sobol_pairs_numpy(*args, sc.PQ)
    mean, cov = np.atleast_2d(mean), cov.reshape(tr["cov"].shape)
    assert not sc.within(mean, cov, tr, g["gate"])
    assert max(max(g["a"].values()), max(g["b"].values())) <= sc.CAP / sc.MARGIN
    S, ST, gS, gST = sc.index_gates(tr, g["gate"])
    first, total, V = sn.indices(cov[:, [0, 2]])
    assert np.all(V > 0)
    assert np.all(first <= total + gS[:, [0, 2]] + gST[:, [0, 2]])
    assert np.all(first.sum(axis=-1) <= 1 + gS[:, [0, 2]].sum(axis=-1))
    assert np.all(first >= -gS[:, [0, 2]])


def test_the_far_box_discriminates():
    """The box [2.5, 3.5]^2 holds no training point and lies 1.5 to 10 scaled lengths from all of them: the plain
    difference of two erf near 1 misses the gate (by 1e7 u S) that the erfc form meets, so the case does tell the two apart.  (At
    [1.5, 2.5]^7 the terms that dominate S have arguments near 1/2, where both forms are good: that case tests the
    branch, this one its purpose.)"""
    from scipy.special import erf
    name = "n33_d2_boxes"
    args = sc.case(name)
    tr, g = sc.truth(name, *args, sc.PQ), sc.gates(name, *args, sc.PQ)
    far = {k: (v[1:2] if isinstance(v, np.ndarray) else v) for k, v in tr.items()}
    good = sn.sobol_pairs_numpy(*args[:3], args[3][1], args[4][1], sc.PQ)
    assert not sc.within(good[0], good[1], far, g["gate"])
    keep = sn.derf
    sn.derf = lambda a, b: erf(a) - erf(b)
    try:
        naive = sn.sobol_pairs_numpy(*args[:3], args[3][1], args[4][1], sc.PQ)
    finally:
        sn.derf = keep
    missed = sc.within(naive[0], naive[1], far, g["gate"])
    print("naive erf difference, errors in u S:", sc.units(naive[0], naive[1], far))
    assert missed


def test_one_active_input_has_indices_of_one():
    n, d = 20, 4
    e = np.full(d, 1e-12)
    e[2] = 3.0
    em = sc.emulator(n, d, 0, e=e)
    args = sc.stack([em]) + sc.UNIT(d)
    tr, g = sc.truth("one_active", *args), sc.gates("one_active", *args)
    S, ST, gS, gST = sc.index_gates(tr, g["gate"])
    mean, cov = sn.sobol_pairs_numpy(*args)
    first, total, V = sn.indices(cov)
    assert abs(first[0, 2] - 1.0) <= gS[0, 0, 2] + 4 * sc.U and abs(total[0, 2] - 1.0) <= gST[0, 0, 2] + 4 * sc.U
    others = [0, 1, 3]
    assert np.all(np.abs(first[0, others]) <= gS[0, 0, others]) and np.all(np.abs(total[0, others]) <= gST[0, 0, others])


def test_indices_are_nan_without_variance():
    S, ST, V = sn.indices(np.array([[0.0, 0.0, 0.0], [-1e-30, 1.0, 1.0], [2.0, 1.0, 1.5]]))
    assert np.all(np.isnan(S[:2])) and np.all(np.isnan(ST[:2])) and S[2, 0] == 0.5 and ST[2, 0] == 0.75


# ---- the Python layer ------------------------------------------------------------------------------------

def gps_of(ems):
    out = []
    for m in ems:
        gp = GaussianProcess(m["inputs"], np.zeros(m["n"]))
        gp.theta, gp.invQt = np.log(m["expX"]), m["invQt"]
        out.append(gp)
    return out


def small_mv(n=24, d=3, P=3, K=40):
    ems = [sc.emulator(n, d, k) for k in range(P)]
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    mv.n_pcs = P
    mv.basis_functions = np.random.RandomState(77).standard_normal((P, K))
    mv.emulators = gps_of(ems)
    return mv, ems


def test_multivariate_sobol_against_the_band_functions():
    """mv.sobol(is_gpu=False) for three bands against the indices of the band functions f_k themselves on the tensor grid."""
    mv, ems = small_mv()
    lo, hi = np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3])
    r = mv.sobol((lo, hi), is_gpu=False)
    assert r.first.shape == (3, 40) and r.total.shape == (3, 40) and r.variance.shape == (40,) and r.mean.shape == (40,)
    bands = [0, 17, 39]
    expX, x, alpha = (np.stack([np.exp(gp.theta) for gp in mv.emulators]), ems[0]["inputs"],
                      np.stack([gp.invQt for gp in mv.emulators]))
    mean_d, cov_d = tensor_definition(expX, x, alpha, lo, hi, coef=mv.basis_functions[:, bands])
    # the quadratic form cancels too: the tolerance is 1e-10 of sum |beta_p beta_q V_pq| over the band's variance
    mean_p, cov_p = tensor_definition(expX, x, alpha, lo, hi)
    for i, k in enumerate(bands):
        beta = np.abs(mv.basis_functions[:, k])
        V = float(cov_d[i, i, 0])
        tol = 1e-10 * float(beta @ np.abs(cov_p[:, :, 0]).astype(np.float64) @ beta) / V
        assert np.all(np.abs(r.first[:, k] - (cov_d[i, i, 1:4] / cov_d[i, i, 0]).astype(np.float64)) <= tol)
        assert np.all(np.abs(r.total[:, k] - (cov_d[i, i, 4:7] / cov_d[i, i, 0]).astype(np.float64)) <= tol)
        assert abs(r.variance[k] - V) <= tol * V
        assert abs(r.mean[k] - float(mean_d[i])) <= 1e-10 * float(beta @ np.abs(mean_p).astype(np.float64))
    # 2-D bounds: a leading axis
    two = mv.sobol((np.stack([lo, lo - 0.5]), np.stack([hi, hi + 0.5])), is_gpu=False)
    assert two.first.shape == (2, 3, 40) and two.variance.shape == (2, 40)
    assert np.allclose(two.first[0], r.first, rtol=1e-9, atol=1e-12)


def test_mirrored_pairs_against_all_pairs():
    """The P (P + 1) / 2 pairs mirrored give the P^2 pairs inside the gate (a pair and its transpose are different sums),
    and the bands' indices from either agree inside the propagated gates."""
    mv, ems = small_mv()
    P = 3
    args = sc.stack(ems) + (np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3]))
    up = sn.upper_pairs(P)
    assert up.tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]]
    every = np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)
    tr, g = sc.truth("mirror_all", *args, every), sc.gates("mirror_all", *args, every)
    mean, cov_up = sn.sobol_pairs_numpy(*args, up)
    mirrored = sn.mirror(cov_up, P).reshape(1, P * P, -1)
    assert not sc.within(mean, mirrored, tr, g["gate"])
    _, cov_all = sn.sobol_pairs_numpy(*args, every)
    tr_up = sc.truth("mirror_up", *args, up)
    st = sc.spectral_truth(mv.basis_functions, tr_up, P, sc.gates("mirror_up", *args, up)["gate"])
    a = sn.spectral(mv.basis_functions, mean, sn.mirror(cov_up, P))
    b = sn.spectral(mv.basis_functions, mean, cov_all.reshape(P, P, -1))
    for name in ("first", "total", "variance"):
        assert np.all(np.abs(getattr(a, name) - getattr(b, name)) <= 2 * st["g_" + name])
        assert np.all(np.abs(getattr(a, name) - st[name].astype(np.float64)) <= st["g_" + name] + 4 * sc.U * np.abs(getattr(a, name)))


def test_sobol_bands_and_sobol_indices_numpy():
    ems = [sc.emulator(20, 3, k) for k in range(3)]
    gps = gps_of(ems)
    lo, hi = sc.THREE(3)
    r = perband.sobol_bands(gps, (lo, hi), is_gpu=False)
    assert r.first.shape == (3, 3, 3) and r.total.shape == (3, 3, 3) and r.variance.shape == (3, 3) and r.mean.shape == (3, 3)
    r1 = perband.sobol_bands(gps, (lo[2], hi[2]), is_gpu=False)
    assert r1.first.shape == (3, 3) and r1.mean.shape == (3,) and np.array_equal(r1.first, r.first[2])
    one = gps[1].sobol_indices((lo[2], hi[2]))
    assert one.first.shape == (3,) and np.ndim(one.variance) == 0
    assert np.array_equal(one.first, r1.first[1]) and one.mean == r1.mean[1] and one.variance == r1.variance[1]
    boxed = gps[1].sobol_indices((lo, hi))
    assert boxed.first.shape == (3, 3) and np.array_equal(boxed.total, r.total[:, 1])
    with pytest.raises(ValueError):
        perband.sobol_bands(gps, (lo[:, :2], hi[:, :2]), is_gpu=False)
    with pytest.raises(ValueError):
        perband.sobol_bands(gps, (hi[0], lo[0]), is_gpu=False)
    with pytest.raises(ValueError):
        sn.sobol_pairs_numpy(*sc.stack(ems), lo[0], hi[0], pairs=[[0, 3]])


# ---- launch plan and error returns -----------------------------------------------------------------------

def test_launch_plan_arithmetic():
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    assert re.search(r"#define GP_OP_SOBOL %d\b" % _lib.GP_OP_SOBOL, text)
    plan_code = int(re.search(r"#define GP_PLAN_SOBOL (\d+)", text).group(1))
    assert _lib.PLAN_KERNELS[plan_code] == "sobol" and _lib._PLAN_OPS["sobol"] == _lib.GP_OP_SOBOL
    wgs = {8: 1, 12: 1, 16: 1}                                    # workgroups per compute unit by instance (> 256 VGPRs each)
    for cu in (1, 8, 256):
        for n in (1, 15, 16, 17, 250, 512):
            for d in (1, 8, 9, 12, 13, 16):
                for boxes, pairs in ((1, 1), (3, 78), (1000, 78), (1, 2101)):
                    p = _lib.launch_plan("sobol", np.float64, boxes, n_train=n, n_inputs=d, n_emulators=pairs, compute_units=cu)
                    items = boxes * pairs * ((n + 15) // 16)
                    cap = cu * wgs[8 if d <= 8 else 12 if d <= 12 else 16]
                    assert p == dict(kernel="sobol", rows_per_item=16, items=items, workgroups=min(items, cap), rest_items=0,
                                     rest_workgroups=0)
    for bad in (dict(n_train=513, n_inputs=2), dict(n_train=10, n_inputs=17)):
        with pytest.raises(_lib.GpuPredictError, match="status -4"):
            _lib.launch_plan("sobol", np.float64, 1, n_emulators=1, **bad)
    with pytest.raises(_lib.GpuPredictError, match="status -1"):
        _lib.launch_plan("sobol", np.float64, 1, n_emulators=1, n_train=0, n_inputs=2)


def test_error_returns_without_a_device():
    lib = _lib.load()
    d = (ctypes.c_double * 8)()
    assert lib.gp_sobol_batch_f64(None, 1, d, d, d, 1, 1, 1, d, d, 1, None, d, d) == -1
    assert lib.gp_last_error_string().decode() == "null context"
    ctx = _lib.Context.__new__(_lib.Context)                      # the binding's own checks come before the library
    with pytest.raises(ValueError):
        _lib.Context.sobol_batch(ctx, np.ones((2, 4)), np.zeros((5, 3)), np.ones((2, 5)), np.zeros(3), np.ones(3))
    with pytest.raises(ValueError):
        _lib.Context.sobol_batch(ctx, np.ones((2, 5)), np.zeros((5, 3)), np.ones((2, 4)), np.zeros(3), np.ones(3))
    with pytest.raises(ValueError):
        _lib.Context.sobol_batch(ctx, np.ones((2, 5)), np.zeros((5, 3)), np.ones((2, 5)), np.zeros(2), np.ones(2))
    with pytest.raises(ValueError):
        _lib.Context.sobol_batch(ctx, np.ones((2, 5)), np.zeros((5, 3)), np.ones((2, 5)), np.zeros(3), np.ones(3), pairs=[0, 1, 1])
