"""Sobol interactions and main-effect curves without a GPU: the numpy branch against the definition, the exact
decompositions, the moments of the curves, the matrix form, the band form, the launch-plan arithmetic and the error
returns that need no device.  Every test here needs functions or entries that do not exist before this feature."""
import ctypes
import os
import re

import numpy as np
import pytest

import sobol_cases as sc
import sobol2_cases as s2

from gp_emulator_amd import _lib, _sobol_numpy as sn, perband
from gp_emulator_amd.GaussianProcess import GaussianProcess
from gp_emulator_amd.multivariate_gp import MultivariateEmulator

LD = sc.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition ----------------------------------------------------------------------------------------

def tensor_functions(expX, x, alpha, lo, hi, n=60, coef=None):
    """The emulators (or, with ``coef`` (E, K), the functions sum_p coef[p, k] mu_p) on the n^3 tensor Gauss-Legendre grid
    of the box (D = 3), the nodes per input and the weights: (f (K, n, n, n), nodes, w) in longdouble."""
    E, (N, D) = expX.shape[0], x.shape
    assert D == 3
    z, wz = sc.gauss_legendre(n)
    nodes = [LD(lo[d]) + (LD(hi[d]) - LD(lo[d])) * (z + 1) / 2 for d in range(D)]
    f = []
    for e in range(E):
        g = [np.exp(-LD(expX[e, d]) / 2 * (x[:, d].astype(LD)[:, None] - nodes[d][None, :]) ** 2) for d in range(D)]
        f.append(np.einsum("j,ja,jb,jc->abc", LD(expX[e, D]) * alpha[e].astype(LD), g[0], g[1], g[2]))
    f = np.stack(f)
    if coef is not None:
        f = np.einsum("pk,pabc->kabc", np.asarray(coef, dtype=LD), f)
    return f, nodes, wz / 2


def definition_v2(f, w):
    """(K, K, 3): Cov(E[f_p | t_i, t_k], E[f_q | t_i, t_k]) - Vm^i - Vm^k for (i, k) = (0,1), (0,2), (1,2)."""
    K = f.shape[0]
    mean = np.einsum("kabc,a,b,c->k", f, w, w, w)
    one = [np.einsum("kabc,%s,%s->k%s" % (r[0], r[1], i), f, w, w) for i, r in (("a", "bc"), ("b", "ac"), ("c", "ab"))]
    two = [np.einsum("kabc,%s->k%s" % (o, ik), f, w) for ik, o in (("ab", "c"), ("ac", "b"), ("bc", "a"))]
    out = np.empty((K, K, 3), LD)
    for p in range(K):
        for q in range(K):
            mm = mean[p] * mean[q]
            vm = [(one[i][p] * one[i][q] * w).sum() - mm for i in range(3)]
            for n, (i, k) in enumerate(((0, 1), (0, 2), (1, 2))):
                out[p, q, n] = (two[n][p] * two[n][q] * w[:, None] * w[None, :]).sum() - mm - vm[i] - vm[k]
    return out, mean, one


def test_numpy_branch_against_the_definition():
    """D = 3, N = 14, two emulators with different theta and their cross pair: V2 within 1e-10 |V| of
    Cov(E[.|t_i,t_k]) - Vm^i - Vm^k by 60-node tensor Gauss-Legendre, and the main effect within 1e-10 of the curve's
    scale of E[mu | t_i = t] - mean at the nodes 3, 30 and 57 of every input (the margin is test_sobol_cpu.py's)."""
    ems = [sc.emulator(14, 3, 0), sc.emulator(14, 3, 1)]
    expX, x, alpha = sc.stack(ems)
    lo, hi = np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3])
    f, nodes, w = tensor_functions(expX, x, alpha, lo, hi)
    v2, mean, one = definition_v2(f, w)
    pairs = [[0, 0], [0, 1], [1, 0], [1, 1]]
    _, cov = sn.sobol_pairs_numpy(expX, x, alpha, lo, hi, pairs)
    inter = sn.interactions_numpy(expX, x, alpha, lo, hi, pairs)
    assert inter.shape == (4, 3)
    worst = max(float(np.max(np.abs(inter[k] - v2[p, q]) / abs(cov[k, 0]))) for k, (p, q) in enumerate(pairs))
    print("V2: worst difference relative to |V|: %.3g" % worst)
    assert worst <= 1e-10
    at = [3, 30, 57]
    grid = np.stack([nodes[d][at].astype(np.float64) for d in range(3)])
    eff = sn.main_effects_numpy(expX, x, alpha, lo, hi, grid)
    assert eff.shape == (2, 3, 3)
    worst = 0.0
    for e in range(2):
        for d in range(3):
            ref = (one[d][e] - mean[e])
            scale = float(np.max(np.abs(ref)))
            # (the float64 grid point is the longdouble node rounded: the curve's slope times 1e-16 is far below the margin)
            worst = max(worst, float(np.max(np.abs(eff[e, d] - ref[at].astype(np.float64)))) / scale)
    print("main effect: worst difference relative to the curve's largest value: %.3g" % worst)
    assert worst <= 1e-10


# ---- the yardsticks inside the gate, the exact decompositions ----------------------------------------------------

@pytest.mark.parametrize("name", list(s2.CASES))
def test_numpy_branch_and_kernel_form_inside_the_gate(name):
    """Both yardsticks of every case of the kernel tests stay far below the cap (so the gates are theirs, not the cap),
    and the restated summation of the kernels lies within the gate of the truth."""
    args = s2.case(name)
    tr, g = s2.truth(name, *args, s2.PQ), s2.gates(name, *args, s2.PQ)
    print(name, "a", g["a"], "b", g["b"])
    assert max(max(g["a"].values()), max(g["b"].values())) <= s2.CAP / s2.MARGIN
    assert not s2.within(*s2.kernel_form(*args, s2.PQ, tr["grid"]), tr, g["gate"])
    grid = tr["grid"] if np.ndim(args[3]) == 2 else tr["grid"][0]
    assert not s2.within(sn.interactions_numpy(*args, s2.PQ), sn.main_effects_numpy(*args, grid), tr, g["gate"])


def _sums(expX, x, alpha, lo, hi, pairs):
    """Truths and numpy values of one box: (cov, S_cov, inter, S_inter) truth rows and (cov, inter) of the numpy branch."""
    key = ("decomp", x.shape, tuple(map(tuple, pairs)))
    t1, g1 = sc.truth(key, expX, x, alpha, lo, hi, pairs), sc.gates(key, expX, x, alpha, lo, hi, pairs)
    t2, g2 = s2.truth(key, expX, x, alpha, lo, hi, pairs), s2.gates(key, expX, x, alpha, lo, hi, pairs)
    _, cov = sn.sobol_pairs_numpy(expX, x, alpha, lo, hi, pairs)
    return t1, g1["gate"], t2, g2["gate"], cov, sn.interactions_numpy(expX, x, alpha, lo, hi, pairs)


def test_exact_decomposition_two_inputs():
    """D = 2: Vt^i = Vm^i + V2^{01} for both i and V = Vm^0 + Vm^1 + V2^{01}, every term inside its gate in u S."""
    expX, x, alpha = sc.stack([sc.emulator(20, 2, 0), sc.emulator(20, 2, 1)])
    lo, hi = np.array([0.0, -0.3]), np.array([1.0, 1.2])
    t1, g1, t2, g2, cov, inter = _sums(expX, x, alpha, lo, hi, s2.PQ)
    S, u = t1["S_cov"][0].astype(np.float64), sc.U
    S2 = t2["S_inter"][0].astype(np.float64)
    for n in range(3):
        V, Vm, Vt, V2 = cov[n, 0], cov[n, 1:3], cov[n, 3:5], inter[n, 0]
        for i in range(2):
            assert abs(Vt[i] - Vm[i] - V2) <= u * (g1["Vt"] * S[n, 3 + i] + g1["Vm"] * S[n, 1 + i] + g2["V2"] * S2[n, 0])
        assert abs(V - Vm.sum() - V2) <= u * (g1["V"] * S[n, 0] + g1["Vm"] * S[n, 1:3].sum() + g2["V2"] * S2[n, 0])


def test_exact_decomposition_three_inputs():
    """D = 3: Vt^i - Vm^i - sum_k V2^{ik} is the third-order term for every i, and it is V - sum Vm - sum V2."""
    expX, x, alpha = sc.stack([sc.emulator(14, 3, 0), sc.emulator(14, 3, 1)])
    lo, hi = np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3])
    t1, g1, t2, g2, cov, inter = _sums(expX, x, alpha, lo, hi, s2.PQ)
    S, S2, u = t1["S_cov"][0].astype(np.float64), t2["S_inter"][0].astype(np.float64), sc.U
    with_i = {0: [0, 1], 1: [0, 2], 2: [1, 2]}      # (0,1), (0,2), (1,2)
    for n in range(3):
        V, Vm, Vt = cov[n, 0], cov[n, 1:4], cov[n, 4:7]
        third = V - Vm.sum() - inter[n].sum()
        tol3 = u * (g1["V"] * S[n, 0] + g1["Vm"] * S[n, 1:4].sum() + g2["V2"] * S2[n].sum())
        assert third != 0.0
        for i in range(3):
            v = Vt[i] - Vm[i] - inter[n, with_i[i]].sum()
            tol = u * (g1["Vt"] * S[n, 4 + i] + g1["Vm"] * S[n, 1 + i] + g2["V2"] * S2[n, with_i[i]].sum())
            assert abs(v - third) <= tol + tol3


def test_main_effect_moments():
    """On panelled Gauss-Legendre nodes the weighted mean of the curve is 0 and its weighted mean square Vm^i, relative
    to the terms' magnitudes: |mean| <= gate u max S and |mean square - Vm^i| <= u (gate_Vm S_Vm + 2 gate max|m| max S)."""
    em = sc.emulator(20, 3, 0)
    expX, x, alpha = sc.stack([em])
    lo, hi = np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3])
    z, wz = sc.gauss_legendre(20)
    panels = 8
    f = np.concatenate([(k + (z.astype(np.float64) + 1) / 2) / panels for k in range(panels)])
    w = np.concatenate([wz.astype(np.float64) / 2 / panels] * panels)
    grid = lo[:, None] + (hi - lo)[:, None] * f[None, :]
    key = "moments"
    t1, g1 = sc.truth(key, expX, x, alpha, lo, hi), sc.gates(key, expX, x, alpha, lo, hi)
    t2, g2 = s2.truth(key, expX, x, alpha, lo, hi, grid=grid), s2.gates(key, expX, x, alpha, lo, hi, grid=grid)
    eff = sn.main_effects_numpy(expX, x, alpha, lo, hi, grid)[0]
    assert not s2.within(None, eff, t2, g2["gate"])
    S = t2["S_main"][0, 0].astype(np.float64)
    _, cov = sn.sobol_pairs_numpy(expX, x, alpha, lo, hi)
    for i in range(3):
        assert abs((w * eff[i]).sum()) <= (g2["gate"]["main"] + 4) * sc.U * S[i].max()
        tol = sc.U * (g1["gate"]["Vm"] * float(t1["S_cov"][0, 0, 1 + i]) + 2 * (g2["gate"]["main"] + 4) * np.abs(eff[i]).max() * S[i].max())
        assert abs((w * eff[i] ** 2).sum() - cov[0, 1 + i]) <= tol


def test_pair_symmetry_and_matrix_shape():
    expX, x, alpha = sc.stack([sc.emulator(14, 3, 0), sc.emulator(14, 3, 1)])
    lo, hi = sc.THREE(3)
    key = "symmetry"
    pairs = [[0, 1], [1, 0], [0, 0], [1, 1]]
    t2, g2 = s2.truth(key, expX, x, alpha, lo, hi, pairs), s2.gates(key, expX, x, alpha, lo, hi, pairs)
    inter = sn.interactions_numpy(expX, x, alpha, lo, hi, pairs)
    assert inter.shape == (3, 4, 3)
    tol = 2 * g2["gate"]["V2"] * sc.U * t2["S_inter"][:, 0].astype(np.float64)
    assert np.all(np.abs(inter[:, 0] - inter[:, 1]) <= tol)                 # (a pair and its transpose are different sums)
    _, cov = sn.sobol_pairs_numpy(expX, x, alpha, lo, hi)
    second, higher = sn.second_order(cov, inter[:, 2:])
    first, total, V = sn.indices(cov)
    assert second.shape == (3, 2, 3, 3) and higher.shape == (3, 2)
    assert np.array_equal(second, np.swapaxes(second, -1, -2))
    assert np.array_equal(np.diagonal(second, axis1=-2, axis2=-1), first)
    assert np.array_equal(second[..., 0, 2], inter[:, 2:, 1] / V)
    assert np.allclose(higher, 1 - first.sum(-1) - (inter[:, 2:] / V[..., None]).sum(-1), rtol=0, atol=1e-15)
    assert sn.input_pairs(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert sn.input_pairs(1).shape == (0, 2)
    with pytest.raises(ValueError):
        sn.second_order(cov, inter[:, 2:, :2])


def test_no_variance_is_nan_and_one_input_is_empty():
    second, higher = sn.second_order(np.array([[0.0, 0.0, 0.0, 0.0, 0.0], [-1e-30, 1.0, 1.0, 1.0, 1.0], [2.0, 1.0, 0.5, 1.5, 1.0]]),
                                     np.array([[0.0], [1.0], [0.5]]))
    assert np.all(np.isnan(second[:2])) and np.all(np.isnan(higher[:2]))
    assert second[2].tolist() == [[0.5, 0.25], [0.25, 0.25]] and higher[2] == 0.0
    em = sc.emulator(15, 1, 0)
    expX, x, alpha = sc.stack([em, sc.emulator(15, 1, 1)])
    inter = sn.interactions_numpy(expX, x, alpha, [0.0], [1.0], s2.PQ)
    assert inter.shape == (3, 0)
    assert sn.interactions_numpy(expX, x, alpha, [[0.0], [0.5]], [[1.0], [2.0]]).shape == (2, 2, 0)
    _, cov = sn.sobol_pairs_numpy(expX, x, alpha, [0.0], [1.0])
    second, higher = sn.second_order(cov, inter[[0, 2]])
    assert second.shape == (2, 1, 1) and np.allclose(higher, 0.0, atol=1e-9)


# ---- the Python layer ------------------------------------------------------------------------------------------

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


def test_band_form_against_the_band_functions():
    """mv.sobol_interactions and mv.main_effects (numpy branch) for three bands of a 3-PC toy against the band functions
    f_k themselves on the tensor grid; tolerances as test_sobol_cpu.py's band test (the quadratic form cancels too)."""
    mv, ems = small_mv()
    lo, hi = np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3])
    r = mv.sobol_interactions((lo, hi), is_gpu=False)
    ref = mv.sobol((lo, hi), is_gpu=False)
    assert r.second.shape == (3, 3, 40) and r.higher.shape == (40,)
    for name in ("first", "total", "variance", "mean"):
        assert np.array_equal(getattr(r, name), getattr(ref, name))
    assert np.array_equal(r.second, np.swapaxes(r.second, 0, 1))
    assert np.array_equal(r.second[[0, 1, 2], [0, 1, 2]], r.first)
    bands = [0, 17, 39]
    expX, x, alpha = sc.stack(ems)
    f, nodes, w = tensor_functions(expX, x, alpha, lo, hi, coef=mv.basis_functions[:, bands])
    v2, mean, one = definition_v2(f, w)
    _, mean_p, one_p = definition_v2(tensor_functions(expX, x, alpha, lo, hi)[0], w)
    _, cov_p = sn.sobol_pairs_numpy(expX, x, alpha, lo, hi, [(p, q) for p in range(3) for q in range(3)])
    at = [3, 30, 57]
    grid = np.stack([nodes[d][at].astype(np.float64) for d in range(3)])
    m = mv.main_effects((lo, hi), grid=grid, is_gpu=False)
    assert m.effect.shape == (3, 3, 40) and m.mean.shape == (40,) and np.array_equal(m.grid, grid)
    assert np.allclose(m.mean, ref.mean, rtol=1e-12, atol=0)
    for i, k in enumerate(bands):
        beta = np.abs(mv.basis_functions[:, k])
        V = float(r.variance[k])
        tol = 1e-10 * float(beta @ np.abs(cov_p[:, 0]).reshape(3, 3) @ beta) / V
        for n, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
            assert abs(r.second[a, b, k] - float(v2[i, i, n]) / V) <= tol
        for d in range(3):
            refc = (one[d][i] - mean[i])[at].astype(np.float64)
            scale = float(beta @ np.max(np.abs(one_p[d] - mean_p[:, None]), axis=1).astype(np.float64))      # (the sum over PCs cancels)
            assert np.all(np.abs(m.effect[d, :, k] - refc) <= 1e-10 * scale)
    two = mv.sobol_interactions((np.stack([lo, lo - 0.5]), np.stack([hi, hi + 0.5])), is_gpu=False)
    assert two.second.shape == (2, 3, 3, 40) and two.higher.shape == (2, 40)
    assert np.allclose(two.second[0], r.second, rtol=1e-9, atol=1e-12)


def test_bands_and_single_emulator_numpy():
    ems = [sc.emulator(20, 3, k) for k in range(3)]
    gps = gps_of(ems)
    lo, hi = sc.THREE(3)
    r = perband.sobol_interactions_bands(gps, (lo, hi), is_gpu=False)
    ref = perband.sobol_bands(gps, (lo, hi), is_gpu=False)
    assert r.second.shape == (3, 3, 3, 3) and r.higher.shape == (3, 3)
    assert all(np.array_equal(getattr(r, k), getattr(ref, k)) for k in ("first", "total", "variance", "mean"))
    one = gps[1].sobol_interactions((lo[2], hi[2]))
    assert one.second.shape == (3, 3) and np.ndim(one.higher) == 0 and np.array_equal(one.second, r.second[2, 1])
    boxed = gps[1].sobol_interactions((lo, hi))
    assert boxed.second.shape == (3, 3, 3) and np.array_equal(boxed.higher, r.higher[:, 1])
    m = perband.main_effects_bands(gps, (lo, hi), is_gpu=False)
    assert m.grid.shape == (3, 3, 33) and m.effect.shape == (3, 3, 3, 33) and m.mean.shape == (3, 3)
    assert np.array_equal(m.grid[..., 0], lo) and np.array_equal(m.grid[..., -1], hi)
    assert np.allclose(m.mean, ref.mean, rtol=1e-13, atol=0)
    m1 = gps[1].main_effects((lo[2], hi[2]), n_grid=5)
    assert m1.grid.shape == (3, 5) and m1.effect.shape == (3, 5) and np.ndim(m1.mean) == 0
    assert np.array_equal(m1.effect[:, [0, 4]], m.effect[2, 1][:, [0, 32]])
    mb = gps[1].main_effects((lo, hi), grid=np.array([[0.1, 0.2], [0.3, 0.4], [3.0, -2.0]]))
    assert mb.effect.shape == (3, 3, 2) and mb.grid.shape == (3, 3, 2) and np.all(np.isfinite(mb.effect))
    with pytest.raises(ValueError):
        perband.main_effects_bands(gps, (lo, hi), grid=np.zeros((2, 4)), is_gpu=False)
    with pytest.raises(ValueError):
        perband.main_effects_bands(gps, (lo, hi), n_grid=0, is_gpu=False)
    with pytest.raises(ValueError):
        perband.sobol_interactions_bands(gps, (hi[0], lo[0]), is_gpu=False)
    with pytest.raises(ValueError):
        sn.interactions_numpy(*sc.stack(ems), lo[0], hi[0], pairs=[[0, 3]])


# ---- launch plan and error returns -----------------------------------------------------------------------------

def test_launch_plan_arithmetic():
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    assert re.search(r"#define GP_OP_SOBOL_INTER %d\b" % _lib.GP_OP_SOBOL_INTER, text)
    plan_code = int(re.search(r"#define GP_PLAN_SOBOL_INTER (\d+)", text).group(1))
    assert _lib.PLAN_KERNELS[plan_code] == "sobol_inter" and _lib._PLAN_OPS["sobol_inter"] == _lib.GP_OP_SOBOL_INTER
    ops = [int(v) for v in re.findall(r"#define GP_OP_\w+ (\d+)", text)]
    plans = [int(v) for v in re.findall(r"#define GP_PLAN_\w+ (\d+)", text)]
    assert len(set(ops)) == len(ops) and len(set(plans)) == len(plans)
    for cu in (1, 8, 256):
        for n in (1, 15, 16, 17, 250, 512):
            for d in (1, 2, 8, 9, 12, 13, 16):
                for boxes, pairs in ((1, 1), (3, 78), (1000, 78), (1, 2101)):
                    p = _lib.launch_plan("sobol_inter", np.float64, boxes, n_train=n, n_inputs=d, n_emulators=pairs, compute_units=cu)
                    items = boxes * pairs * ((n + 15) // 16) if d > 1 else 0
                    assert p == dict(kernel="sobol_inter", rows_per_item=16, items=items, workgroups=min(items, cu), rest_items=0,
                                     rest_workgroups=0)
    for bad in (dict(n_train=513, n_inputs=2), dict(n_train=10, n_inputs=17)):
        with pytest.raises(_lib.GpuPredictError, match="status -4"):
            _lib.launch_plan("sobol_inter", np.float64, 1, n_emulators=1, **bad)
    with pytest.raises(_lib.GpuPredictError, match="status -1"):
        _lib.launch_plan("sobol_inter", np.float64, 1, n_emulators=1, n_train=0, n_inputs=2)


def test_error_returns_without_a_device():
    lib = _lib.load()
    d = (ctypes.c_double * 8)()
    assert lib.gp_sobol_interactions_f64(None, 1, d, d, d, 1, 2, 1, d, d, 1, None, d) == -1
    assert lib.gp_last_error_string().decode() == "null context"
    assert lib.gp_sobol_main_effects_f64(None, 1, d, d, d, 1, 2, 1, d, d, 1, d, d) == -1
    assert lib.gp_last_error_string().decode() == "null context"
    # behind the context check nothing touches the device before the arguments are judged: a context that is never used
    fake = ctypes.create_string_buffer(4096)
    lo, hi = (ctypes.c_double * 2)(0.0, 0.0), (ctypes.c_double * 2)(1.0, 1.0)
    inter, main = lib.gp_sobol_interactions_f64, lib.gp_sobol_main_effects_f64
    assert inter(fake, 1, None, d, d, 1, 2, 1, lo, hi, 1, None, d) == -1                 # NULL
    assert inter(fake, 1, d, d, d, 1, 2, 1, lo, hi, 1, None, None) == -1
    assert inter(fake, 1, d, d, d, 0, 2, 1, lo, hi, 1, None, d) == -1                    # sizes
    assert inter(fake, 1, d, d, d, 1, 2, 0, lo, hi, 1, None, d) == -1
    assert inter(fake, 1, d, d, d, 1, 2, 1, lo, hi, 0, None, d) == -1
    assert inter(fake, 1, d, d, d, 1, 2, 1, lo, hi, 2, None, d) == -1                    # no list: n_pairs is n_emulators
    assert inter(fake, 1, d, d, d, 1, 2, 1, lo, hi, 1, (ctypes.c_int32 * 2)(0, 1), d) == -1
    assert inter(fake, 1, d, d, d, 1, 2, 1, hi, lo, 1, None, d) == -1                    # hi <= lo
    assert inter(fake, 1, d, d, d, 513, 2, 1, lo, hi, 1, None, d) == -4                  # over the limits
    assert inter(fake, 1, d, d, d, 1, 17, 1, lo, hi, 1, None, d) == -4
    assert main(fake, 1, d, d, d, 1, 2, 1, lo, hi, 1, None, d) == -1
    assert main(fake, 1, d, d, d, 1, 2, 1, lo, hi, 1, d, None) == -1
    assert main(fake, 1, d, d, d, 1, 2, 1, lo, hi, 0, d, d) == -1
    assert main(fake, 0, d, d, d, 1, 2, 1, lo, hi, 1, d, d) == -1
    assert main(fake, 1, d, d, d, 1, 2, 1, hi, lo, 1, d, d) == -1
    assert main(fake, 1, d, d, d, 513, 2, 1, lo, hi, 1, d, d) == -4
    assert main(fake, 1, d, d, d, 1, 17, 1, lo, hi, 1, d, d) == -4
    ctx = _lib.Context.__new__(_lib.Context)                      # the binding's own checks come before the library
    for fn, last in ((_lib.Context.sobol_interactions, ()), (_lib.Context.sobol_main_effects, (np.zeros((3, 4)),))):
        with pytest.raises(ValueError):
            fn(ctx, np.ones((2, 4)), np.zeros((5, 3)), np.ones((2, 5)), np.zeros(3), np.ones(3), *last)
        with pytest.raises(ValueError):
            fn(ctx, np.ones((2, 5)), np.zeros((5, 3)), np.ones((2, 4)), np.zeros(3), np.ones(3), *last)
        with pytest.raises(ValueError):
            fn(ctx, np.ones((2, 5)), np.zeros((5, 3)), np.ones((2, 5)), np.zeros(2), np.ones(2), *last)
    with pytest.raises(ValueError):
        _lib.Context.sobol_interactions(ctx, np.ones((2, 5)), np.zeros((5, 3)), np.ones((2, 5)), np.zeros(3), np.ones(3), pairs=[0, 1, 1])
    with pytest.raises(ValueError):
        _lib.Context.sobol_main_effects(ctx, np.ones((2, 5)), np.zeros((5, 3)), np.ones((2, 5)), np.zeros(3), np.ones(3), np.zeros((2, 4)))
