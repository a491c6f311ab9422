"""gp_sobol_interactions_f64 and gp_sobol_main_effects_f64 on the GPU -- sobol_inter_kernel<8 | 12 | 16>,
sobol_inter_fold_kernel, sobol_main_kernel -- and the Python layer above them.

The kernels are held to the quadrature truth inside the gates of sobol2_cases.py (16 x the worse of two float64 numpy
evaluations, floor 16, cap 1024, in units of u S), their reproducibility is checked bit for bit, and -7.25e300 sentinels
lie behind every output of every call made through ``inter_call`` and ``main_call``.  Every test here needs the entries,
the bindings or the methods, none of which exist before this feature."""
import numpy as np
import pytest

import sobol_cases as sc
import sobol2_cases as s2

from gp_emulator_amd import _lib, _sobol_numpy as sn, perband
from gp_emulator_amd.GaussianProcess import GaussianProcess
from gp_emulator_amd.multivariate_gp import MultivariateEmulator

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
PQ, UNIT, THREE = s2.PQ, s2.UNIT, s2.THREE


def _arrays(expX, x, alpha, lo, hi):
    expX = np.ascontiguousarray(np.atleast_2d(expX), dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    alpha = np.ascontiguousarray(np.atleast_2d(alpha), dtype=np.float64)
    lo, hi = (np.ascontiguousarray(np.atleast_2d(np.asarray(v, dtype=np.float64))) for v in (lo, hi))
    return expX, x, alpha, lo, hi


def inter_call(expX, x, alpha, lo, hi, pairs=None, want_rc=False):
    """The C entry itself with eight sentinels behind the output: inter (B, P, D (D - 1) / 2)."""
    ctx = _lib.default_context(0)
    expX, x, alpha, lo, hi = _arrays(expX, x, alpha, lo, hi)
    E, (N, D), B = expX.shape[0], x.shape, lo.shape[0]
    if pairs is not None:
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    P, K = E if pairs is None else pairs.shape[0], D * (D - 1) // 2
    out = np.full(B * P * K + 8, SENTINEL)
    rc = ctx.lib.gp_sobol_interactions_f64(ctx.h, E, _lib._ptr(expX), _lib._ptr(x), _lib._ptr(alpha), N, D, B, _lib._ptr(lo),
                                           _lib._ptr(hi), P, None if pairs is None else _lib._ptr(pairs), _lib._ptr(out))
    assert np.all(out[B * P * K:] == SENTINEL), "a sentinel behind the output was overwritten"
    if want_rc:
        return rc, out
    _lib.check(rc, "gp_sobol_interactions_f64")
    return out[:B * P * K].reshape(B, P, K)


def main_call(expX, x, alpha, lo, hi, grid, want_rc=False):
    """The C entry itself with eight sentinels behind the output: effects (B, E, D, G); grid (B, D, G) or (D, G)."""
    ctx = _lib.default_context(0)
    expX, x, alpha, lo, hi = _arrays(expX, x, alpha, lo, hi)
    E, (N, D), B = expX.shape[0], x.shape, lo.shape[0]
    grid = sn.grid_array(grid, lo, hi)
    G = grid.shape[2]
    out = np.full(B * E * D * G + 8, SENTINEL)
    rc = ctx.lib.gp_sobol_main_effects_f64(ctx.h, E, _lib._ptr(expX), _lib._ptr(x), _lib._ptr(alpha), N, D, B, _lib._ptr(lo),
                                           _lib._ptr(hi), G, _lib._ptr(grid), _lib._ptr(out))
    assert np.all(out[B * E * D * G:] == SENTINEL), "a sentinel behind the output was overwritten"
    if want_rc:
        return rc, out
    _lib.check(rc, "gp_sobol_main_effects_f64")
    return out[:B * E * D * G].reshape(B, E, D, G)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("name", list(s2.CASES))
def test_kernels_against_the_truth(gpu_lib, name):
    """V2 of the pairs (0, 0), (0, 1), (1, 1) and the main-effect curves of both emulators at the box's ends, inside and
    outside it, inside the gate of either family in every box of the case; the second-order indices of the two
    emulators inside the propagated gates."""
    args = s2.case(name)
    tr, g = s2.truth(name, *args, PQ), s2.gates(name, *args, PQ)
    inter = inter_call(*args, pairs=PQ)
    main = main_call(*args, tr["grid"])
    print(name, "yardsticks", g["a"], g["b"], "device", s2.units(inter, main, tr))
    assert not s2.within(inter, main, tr, g["gate"])
    key1 = ("s2", name)
    t1, g1 = sc.truth(key1, *args, PQ), sc.gates(key1, *args, PQ)
    S2, gS2 = s2.index_gates(tr, g["gate"], t1, g1["gate"])
    mean, cov = _lib.default_context(0).sobol_batch(*args, pairs=PQ)      # (V of the existing entry, inside its own gate)
    cov = cov.reshape(t1["cov"].shape)
    assert not sc.within(mean, cov, t1, g1["gate"])
    second, _ = sn.second_order(cov[:, [0, 2]], inter[:, [0, 2]])
    ik = sn.input_pairs(tr["D"])
    got = second[..., ik[:, 0], ik[:, 1]]
    assert np.all(np.abs(got - S2[:, [0, 2]].astype(np.float64)) <= gS2[:, [0, 2]] + 4 * sc.U * np.abs(got))


def test_interactions_bit_for_bit_alone_in_a_batch_permuted_and_twice(gpu_lib):
    """A (box, pair) row does not depend on what else the call holds, on the order of the pairs, or on the call."""
    expX, x, alpha, lo, hi = s2.case("n17_d7")
    every = np.array([[0, 0], [0, 1], [1, 0], [1, 1]])
    c1 = inter_call(expX, x, alpha, lo, hi, pairs=every)
    assert same_bits(c1, inter_call(expX, x, alpha, lo, hi, pairs=every))
    assert same_bits(inter_call(expX, x, alpha, lo, hi, pairs=every[::-1]), c1[:, ::-1])
    for k, (p, q) in enumerate(every):
        assert same_bits(inter_call(expX[[p, q]], x, alpha[[p, q]], lo, hi, pairs=[[0, 1]])[:, 0], c1[:, k])
    for b in range(3):
        assert same_bits(inter_call(expX, x, alpha, lo[b], hi[b], pairs=every)[0], c1[b])
    assert same_bits(inter_call(expX[1], x, alpha[1], lo, hi)[:, 0], c1[:, 3])        # one emulator, default pairs


def test_main_effects_bit_for_bit_for_any_grid_size_and_batch(gpu_lib):
    """An (emulator, input, point) is the same bits for G = 1, 33 and 300, alone or in a batch of emulators or boxes."""
    n, d = 33, 9
    expX, x, alpha = sc.stack([sc.emulator(n, d, k) for k in range(3)])
    lo, hi = THREE(d)
    g300 = sn.grid_array(None, lo, hi, 300)
    m300 = main_call(expX, x, alpha, lo, hi, g300)
    assert np.all(np.isfinite(m300))
    at = np.arange(33) * 9 + 2
    assert same_bits(main_call(expX, x, alpha, lo, hi, np.ascontiguousarray(g300[:, :, at])), m300[..., at])
    for k in (0, 257, 299):
        assert same_bits(main_call(expX, x, alpha, lo, hi, np.ascontiguousarray(g300[:, :, k:k + 1])), m300[..., k:k + 1])
    assert same_bits(main_call(expX[1], x, alpha[1], lo[2], hi[2], g300[2])[0, 0], m300[2, 1])
    assert same_bits(main_call(expX[[2, 0]], x, alpha[[2, 0]], lo, hi, g300), m300[:, [2, 0]])


def test_past_two_rounds_of_the_persistent_grid(gpu_lib):
    """More items than two rounds of the grid with a ragged tail: four emulators at N = 33, D = 3 (three j-blocks, the
    last of one row) in a list of their 16 ordered pairs repeated.  Entries of one pair are the same bits wherever they
    stand, the 16 are inside the gate, and a sample equals single-pair calls."""
    n, d = 33, 3
    expX, x, alpha = sc.stack([sc.emulator(n, d, k) for k in range(4)])
    lo, hi = UNIT(d)
    cu = _lib.default_context(0).device_info()["compute_units"]
    cap = _lib.launch_plan("sobol_inter", np.float64, 1, n_train=n, n_inputs=d, n_emulators=1 << 20, compute_units=cu)["workgroups"]
    unique = np.array([(p, q) for p in range(4) for q in range(4)], dtype=np.int32)
    n_pairs = (2 * cap) // 3 + 7
    pairs = unique[(np.arange(n_pairs) * 5 + 3) % 16]
    plan = _lib.launch_plan("sobol_inter", np.float64, 1, n_train=n, n_inputs=d, n_emulators=n_pairs, compute_units=cu)
    assert plan["kernel"] == "sobol_inter" and plan["items"] == 3 * n_pairs and plan["workgroups"] == cap
    assert plan["items"] > 2 * cap and plan["items"] % cap != 0
    inter = inter_call(expX, x, alpha, lo, hi, pairs=pairs)
    key = "grid_n33_d3"
    tr, g = s2.truth(key, expX, x, alpha, lo, hi, unique), s2.gates(key, expX, x, alpha, lo, hi, unique)
    first = np.array([np.flatnonzero((pairs == u).all(axis=1))[0] for u in unique])
    assert not s2.within(inter[:, first], None, tr, g["gate"])
    assert same_bits(inter[0], inter[0, first][pairs[:, 0] * 4 + pairs[:, 1]])
    for k in (0, 1, cap // 3, n_pairs // 2, n_pairs - 1):
        p, q = pairs[k]
        assert same_bits(inter_call(expX[[p, q]], x, alpha[[p, q]], lo, hi, pairs=[[0, 1]])[0, 0], inter[0, k])


def test_main_effects_past_two_rounds_of_the_persistent_grid(gpu_lib):
    """sobol_main_kernel's grid is min(items, 2 x compute units) (plan_sobol_main), an item a (box, emulator): two boxes
    of 2 cu + 39 emulators are more than two rounds with a ragged tail, so every workgroup writes its tables and its
    non-finite flag again for a second and a third item.  The emulators are four distinct ones cycled, with a NaN theta
    at index 1 and an infinite alpha behind the first round; every curve is bit for bit that emulator alone in that
    box, and NaN stays on the rows of the two."""
    n, d, G = 15, 2, 3
    base = sc.stack([sc.emulator(n, d, k) for k in range(4)])
    x = base[1]
    lo, hi = np.array([[0.0, 0.0], [1.5, 1.5]]), np.array([[1.0, 1.0], [2.5, 2.5]])
    grid = np.ascontiguousarray(lo[:, :, None] + (hi - lo)[:, :, None] * np.array([0.0, 0.37, 1.2]))
    cu = _lib.default_context(0).device_info()["compute_units"]
    cap = 2 * cu
    E = cap + 39
    assert 2 * E > 2 * cap and (2 * E) % cap != 0
    which = (np.arange(E) * 3 + 1) % 4
    expX, alpha = base[0][which].copy(), base[2][which].copy()
    bad = [1, cap + 5]
    expX[bad[0], 1] = np.nan
    alpha[bad[1], 7] = np.inf
    got = main_call(expX, x, alpha, lo, hi, grid)
    assert got.shape == (2, E, d, G)
    alone = np.stack([main_call(base[0][k], x, base[2][k], lo, hi, grid)[:, 0] for k in range(4)], axis=1)     # (2, 4, d, G)
    assert np.all(np.isfinite(alone))
    clean = np.setdiff1d(np.arange(E), bad)
    assert np.all(np.isnan(got[:, bad]))
    assert same_bits(got[:, clean], alone[:, which[clean]])


def test_non_finite_emulators_poison_their_own_results_only(gpu_lib):
    """A NaN in one emulator's theta, an infinite b in another's and an infinity in a third's alpha: every pair and
    curve they are part of is NaN, every other output is bit for bit the call without them."""
    n, d = 33, 9
    expX, x, alpha = sc.stack([sc.emulator(n, d, k) for k in range(5)])
    lo, hi = THREE(d)
    pairs = np.array([(p, q) for p in range(5) for q in range(5)], dtype=np.int32)
    grid = s2.test_grid(lo, hi)
    c0, m0 = inter_call(expX, x, alpha, lo, hi, pairs=pairs), main_call(expX, x, alpha, lo, hi, grid)
    assert np.all(np.isfinite(c0)) and np.all(np.isfinite(m0))
    bad_e, bad_a = expX.copy(), alpha.copy()
    bad_e[1, 4] = np.nan
    bad_e[4, d] = np.inf
    bad_a[3, 20] = np.inf
    c1, m1 = inter_call(bad_e, x, bad_a, lo, hi, pairs=pairs), main_call(bad_e, x, bad_a, lo, hi, grid)
    hit = np.isin(pairs, (1, 3, 4)).any(axis=1)
    assert np.all(np.isnan(c1[:, hit])) and np.all(np.isnan(m1[:, [1, 3, 4]]))
    assert same_bits(c1[:, ~hit], c0[:, ~hit]) and same_bits(m1[:, [0, 2]], m0[:, [0, 2]])
    bad_e, bad_a = expX.copy(), alpha.copy()
    bad_e[0, 0] = np.inf
    bad_a[2, 16] = np.nan                                       # (the first row of a j-block)
    c2, m2 = inter_call(bad_e, x, bad_a, lo, hi, pairs=pairs), main_call(bad_e, x, bad_a, lo, hi, grid)
    hit = np.isin(pairs, (0, 2)).any(axis=1)
    assert np.all(np.isnan(c2[:, hit])) and np.all(np.isnan(m2[:, [0, 2]]))
    assert same_bits(c2[:, ~hit], c0[:, ~hit]) and same_bits(m2[:, [1, 3, 4]], m0[:, [1, 3, 4]])


def test_grid_points_outside_the_box_against_the_numpy_branch(gpu_lib):
    """Points up to two box widths outside are evaluated like any other: inside the gate of the truth on that grid, and
    against the numpy branch with its own error on top."""
    n, d = 17, 7
    args = s2.case("n17_d7")
    expX, x, alpha, lo, hi = args
    f = np.array([-2.0, -1.0, -0.01, 1.01, 2.0, 3.0])
    grid = np.ascontiguousarray(lo[:, :, None] + (hi - lo)[:, :, None] * f)
    key = "outside_n17_d7"
    tr, g = s2.truth(key, *args, grid=grid), s2.gates(key, *args, grid=grid)
    main = main_call(*args, grid)
    assert not s2.within(None, main, tr, g["gate"])
    ref = sn.main_effects_numpy(*args, grid)
    slack = {"main": g["gate"]["main"] * (1 + 1.0 / sc.MARGIN), "V2": g["gate"]["V2"]}
    assert not s2.within(None, main, dict(tr, main=ref.astype(sc.LD)), slack)


def test_one_input_writes_nothing_and_errors_leave_the_outputs_untouched(gpu_lib):
    expX, x, alpha = sc.stack([sc.emulator(15, 1, 0), sc.emulator(15, 1, 1)])
    rc, out = inter_call(expX, x, alpha, [0.0], [1.0], pairs=PQ, want_rc=True)
    assert rc == 0 and np.all(out == SENTINEL)
    assert _lib.default_context(0).sobol_interactions(expX, x, alpha, [0.0], [1.0], PQ).shape == (3, 0)
    expX, x, alpha, lo, hi = s2.case("n15_d2")

    def refused(code, fn, *a, **k):
        rc, out = fn(*a, want_rc=True, **k)
        assert rc == code, _lib.load().gp_last_error_string()
        assert np.all(out == SENTINEL)

    grid = s2.test_grid(lo, hi)
    h = hi.copy()
    h[1, 0] = lo[1, 0]
    refused(-1, inter_call, expX, x, alpha, lo, h, pairs=PQ)
    refused(-1, main_call, expX, x, alpha, lo, h, grid)
    h[2, 1] = np.nan
    refused(-1, inter_call, expX, x, alpha, lo, h, pairs=PQ)
    refused(-1, inter_call, expX, x, alpha, lo, hi, pairs=[[0, 0], [0, 2]])
    refused(-4, inter_call, np.ones((2, 19)), np.zeros((4, 17)), np.ones((2, 4)), np.zeros(17), np.ones(17))
    refused(-4, main_call, np.ones((1, 4)), np.zeros((513, 2)), np.ones((1, 513)), [0.0, 0.0], [1.0, 1.0], np.zeros((2, 3)))


# ---- the Python layer ----------------------------------------------------------------------------------------

def gps_of(ems):
    out = []
    for m in ems:
        gp = GaussianProcess(m["inputs"], np.zeros(m["n"]))
        gp.theta, gp.invQt = np.log(m["expX"]), m["invQt"]
        out.append(gp)
    return out


def test_python_layer_is_the_entries_and_agrees_with_sobol_indices(gpu_lib):
    """perband.sobol_interactions_bands / main_effects_bands (is_gpu=True) are the entries on the stacked constants bit
    for bit; first, total, variance and mean of the returned tuple are those of sobol_bands / sobol_indices
    (is_gpu=True) bit for bit; a single emulator is the batch's row; 1-D bounds carry no box axis."""
    n, d = 33, 9
    ems = [sc.emulator(n, d, k) for k in range(3)]
    gps = gps_of(ems)
    expX = np.stack([np.exp(gp.theta) for gp in gps])            # (what the layer itself forms from theta)
    x, alpha = ems[0]["inputs"], np.stack([m["invQt"] for m in ems])
    lo, hi = THREE(d)
    for bounds in ((lo, hi), (lo[1], hi[1])):
        lead = np.shape(bounds[0])[:-1]
        r = perband.sobol_interactions_bands(gps, bounds, is_gpu=True)
        ref = perband.sobol_bands(gps, bounds, is_gpu=True)
        for name in ("first", "total", "variance", "mean"):
            assert same_bits(getattr(r, name), getattr(ref, name)), name
        inter = inter_call(expX, x, alpha, *bounds).reshape(lead + (3, d * (d - 1) // 2))
        _, cov = _lib.default_context(0).sobol_batch(expX, x, alpha, *bounds)
        second, higher = sn.second_order(cov, inter)
        assert r.second.shape == lead + (3, d, d) and same_bits(r.second, second) and same_bits(r.higher, higher)
        one = gps[1].sobol_interactions(bounds, is_gpu=True)
        ind = gps[1].sobol_indices(bounds, is_gpu=True)
        assert same_bits(one.second, second[..., 1, :, :]) and same_bits(one.higher, higher[..., 1])
        for name in ("first", "total", "variance", "mean"):
            assert same_bits(getattr(one, name), getattr(ind, name)), name
        m = perband.main_effects_bands(gps, bounds, is_gpu=True)
        assert m.grid.shape == lead + (d, 33) and m.effect.shape == lead + (3, d, 33)
        assert same_bits(m.effect, main_call(expX, x, alpha, *bounds, m.grid).reshape(m.effect.shape))
        assert same_bits(m.mean, ref.mean)
        m1 = gps[1].main_effects(bounds, n_grid=5, is_gpu=True)
        assert m1.effect.shape == lead + (d, 5) and same_bits(m1.effect[..., [0, 4]], m.effect[..., 1, :, :][..., [0, 32]])
        assert same_bits(m1.mean, ref.mean[..., 1])


def test_multivariate_interactions_and_curves_against_the_numpy_branch(gpu_lib):
    n, d, P, K = 24, 3, 3, 40
    ems = [sc.emulator(n, d, k) for k in range(P)]
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    mv.n_pcs = P
    mv.basis_functions = np.random.RandomState(77).standard_normal((P, K))
    mv.emulators = gps_of(ems)
    lo, hi = np.array([0.0, 0.1, -0.2]), np.array([1.0, 0.9, 1.3])
    args = sc.stack(ems) + (lo, hi)
    pairs = sn.upper_pairs(P)
    key = "mv2_small"
    t1, g1 = sc.truth(key, *args, pairs), sc.gates(key, *args, pairs)
    t2, g2 = s2.truth(key, *args, pairs), s2.gates(key, *args, pairs)
    dev, host = mv.sobol_interactions((lo, hi), is_gpu=True), mv.sobol_interactions((lo, hi), is_gpu=False)
    ind = mv.sobol((lo, hi), is_gpu=True)
    assert dev.second.shape == (d, d, K) and dev.higher.shape == (K,)
    for name in ("first", "total", "variance", "mean"):
        assert same_bits(getattr(dev, name), getattr(ind, name)), name
    # the bands' truth and propagated gate: quadratic forms of the mirrored truth and magnitudes
    basis = mv.basis_functions.astype(sc.LD)
    q2 = np.einsum("pk,pqc,qk->ck", basis, sn.mirror(t2["inter"][0], P), basis)
    m2 = np.einsum("pk,pqc,qk->ck", np.abs(basis), sn.mirror(t2["S_inter"][0], P), np.abs(basis))
    st = sc.spectral_truth(mv.basis_functions, t1, P, g1["gate"])
    V = st["variance"]
    S2 = q2 / V
    gate = ((g2["gate"]["V2"] * m2 * sc.U + np.abs(S2) * st["g_variance"]) / np.abs(V)).astype(np.float64)
    own = 1 + 1.0 / sc.MARGIN
    for n_, (i, k) in enumerate(sn.input_pairs(d)):
        t = S2[n_].astype(np.float64)
        assert np.all(np.abs(dev.second[i, k] - t) <= gate[n_] + 4 * sc.U * np.abs(t))
        assert np.all(np.abs(dev.second[i, k] - host.second[i, k]) <= own * gate[n_] + 4 * sc.U * np.abs(t))
        assert same_bits(dev.second[i, k], dev.second[k, i])
    md, mh = mv.main_effects((lo, hi), n_grid=9, is_gpu=True), mv.main_effects((lo, hi), n_grid=9, is_gpu=False)
    assert md.effect.shape == (d, 9, K) and md.mean.shape == (K,) and same_bits(md.grid, mh.grid)
    tm, gm = s2.truth("mv2_main", *args, grid=md.grid), s2.gates("mv2_main", *args, grid=md.grid)
    ref = np.einsum("pdg,pn->dgn", tm["main"][0], basis)
    mag = np.einsum("pdg,pn->dgn", tm["S_main"][0], np.abs(basis)).astype(np.float64)
    assert np.all(np.abs(md.effect - ref.astype(np.float64)) <= (gm["gate"]["main"] + P) * sc.U * mag)
    assert np.all(np.abs(md.effect - mh.effect) <= (own * gm["gate"]["main"] + 2 * P) * sc.U * mag)
    assert same_bits(md.mean, ind.mean)
