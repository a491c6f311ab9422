"""The PC-space look-up-table search without a GPU: the numpy branch against the longdouble band-space truth and the
a-priori gate (lut_pc_cases.py), the routing of rows the PC form cannot centre, argument errors, the launch plan."""
import ctypes

import numpy as np
import pytest

import lut_cases as lc
import lut_pc_cases as pc
from mv_retrieve_cases import synthetic_emulator

from gp_emulator_amd import _first_guess, _lib

F64, F32 = np.float64, np.float32


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    for name, nargs in (("gp_lut_search_pc_device", 19), ("gp_lut_search_pc_geometry", 6), ("gp_mv_lut_prepare_device", 16)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    for P, dt, padded, wgs in ((1, F64, 8, 2), (8, F64, 8, 2), (9, F64, 12, 1), (12, F64, 12, 1), (13, F64, 16, 1),
                               (16, F64, 16, 1), (8, F32, 8, 2), (12, F32, 12, 2), (16, F32, 16, 2)):
        geo = _lib.lut_search_pc_geometry(P, dt)
        assert geo == dict(rows_per_item=256, candidate_tile=64, padded_pcs=padded, workgroups_per_cu=wgs)
    with pytest.raises(_lib.GpuPredictError):
        _lib.lut_search_pc_geometry(17, F64)


# ---- the numpy branch against the truth ----------------------------------------------------------------

@pytest.mark.parametrize("offset", [True, False])
@pytest.mark.parametrize("weights", [None, "shared", "rows"])
@pytest.mark.parametrize("P", [1, 3, 7, 12, 16])
def test_numpy_branch_against_the_truth(P, weights, offset):
    case = pc.make_problem(F64, P, 61, 90, 9, seed=40 + P, weights=weights, offset=offset)
    T = pc.band_truth(case)
    G, c0, J0, g0, status = _lib.lut_pc_prepare_numpy(case["B"], case["o"], case["w"])
    assert np.all(status == 0) and c0.shape == (9, P) and G.shape == ((9, P, P) if weights == "rows" else (P, P))
    g = pc.band_gate(case, c0)
    assert np.all(g < 1e-11 * T)                       # the gate resolves ranks far closer than any used below
    worst = 0.0
    for n_best in (1, 3, 8):
        index, cost, st = _lib.lut_search_pc_numpy(case["mu"], case["B"], case["o"], case["w"], case["a"], n_best)
        assert np.all(st == 0) and cost.dtype == F64
        worst = max(worst, lc.check_result(T, g, index, cost, n_best, (P, weights, offset, n_best)))
    print("P %d %s offset %s: worst |cost - T| / gate = %.3g" % (P, weights, offset, worst))
    assert worst <= 1.0


def test_the_two_truths_of_lut_pc_cases_agree_for_any_centre():
    """A check of the test helpers alone (no code of the package runs; it passes without the feature): the identity
    holds for ANY c0, so lut_pc_cases.kernel_truth, given the exact J0, g0 and G at a centre far from the least-squares
    one, is lut_pc_cases.band_truth to longdouble rounding.  The GPU tests lean on both truths."""
    case = pc.make_problem(F64, 7, 61, 40, 5, seed=3, weights="rows", offset=True)
    T = pc.band_truth(case)
    o, w = pc._rows(case)
    B = case["B"].astype(lc.LD)
    c0 = np.random.RandomState(1).uniform(-3.0, 3.0, (5, 7))
    r0 = c0.astype(lc.LD) @ B - o
    J0 = 0.5 * np.sum(w * r0 * r0, axis=1)
    g0 = (w * r0) @ B.T
    G = np.stack([(B * w[m]) @ B.T for m in range(5)])
    Tk, _ = pc.kernel_truth(F64, case["mu"], case["a"], c0, J0, g0, G)
    assert np.max(np.abs(Tk - T) / T) < 1e-15


# ---- the public function: indices, routing, NaN rules ---------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    """test_lut_cpu's small emulator: P = 5 PCs, 40 training points, D = 3, B = 21 bands; a pool of 150 states,
    200 candidates, a shared prior, per-row weights with 30 % zeros."""
    mv, _ = synthetic_emulator(5, 40, 3, 21, 1, 77)
    rs = np.random.RandomState(9)
    cand = rs.uniform(0.0, 1.0, (200, 3))
    x_true = rs.uniform(0.0, 1.0, (150, 3))
    w = rs.uniform(0.5, 2.0, (150, 21)) / 21
    w[rs.random_sample((150, 21)) < 0.3] = 0.0
    w[np.count_nonzero(w, axis=1) < 8, :8] = 0.05           # (every pool row keeps enough informative bands)
    mu = np.stack([gp.predict(cand)[0] for gp in mv.emulators])
    return dict(mv=mv, cand=cand, obs=mv.predict_many(x_true, is_gpu=False) + 0.02 * rs.standard_normal((150, 21)), w=w, mu=mu,
                prior=(np.full(3, 0.5), np.diag([0.3, 0.2, 0.1]) + 0.02))


@pytest.mark.parametrize("n_best,kind,with_prior", [(1, None, False), (3, "rows", True), (8, "shared", False)])
def test_first_guess_many_numpy_pc_equals_band_and_truth(small, n_best, kind, with_prior):
    mv, cand = small["mv"], small["cand"]
    prior = small["prior"] if with_prior else None
    a = _first_guess.prior_offset(cand, _first_guess.shared_prior(prior, 3))
    w_pool = None if kind is None else small["w"] if kind == "rows" else small["w"][0]
    pool = dict(dt=np.dtype(F64), B=np.asarray(mv.basis_functions, dtype=F64), mu=small["mu"], o=small["obs"], w=w_pool, a=a,
                P=5, K=21, L=200, M=150)
    rows = pc.separated(pc.band_truth(pool), n_best, 65)
    case = pc.take_rows(pool, rows)
    T = pc.band_truth(case)
    g = pc.band_gate(case, pc.centre(case))
    ratio, want = pc.separation(T, g, n_best)
    print("n_best %d: smallest gap / (sum of the two gates) = %.3g" % (n_best, ratio))
    assert ratio > 1
    got = mv.first_guess_many(cand, case["o"], case["w"], prior, n_best, is_gpu=False, space="pc")
    band = mv.first_guess_many(cand, case["o"], case["w"], prior, n_best, is_gpu=False, space="band")
    lc.check_result(T, g, got[2], got[1], n_best, "pc")
    assert np.array_equal(got[2], want) and np.array_equal(got[2], band[2]) and np.array_equal(got[0], band[0])


def test_rows_the_pc_form_cannot_centre_are_reported_and_routed(small):
    mv, cand = small["mv"], small["cand"]
    obs, w = small["obs"][:6].copy(), small["w"][:6].copy()
    w[1] = 0.0                                           # all masked
    obs[1] = np.nan
    w[3] = 0.0                                           # fewer informative bands (3) than PCs (5)
    w[3, [2, 9, 17]] = 0.05
    obs[4, 5], w[4, 5] = np.nan, 0.05                    # a NaN under a non-zero weight
    index, cost, status = _lib.lut_search_pc_numpy(small["mu"], mv.basis_functions, obs, w, None, 3)
    assert status[1] == 1 and 1 <= status[3] <= 5 and status[4] == 6 and np.all(status[[0, 2, 5]] == 0)
    for m in (1, 3, 4):
        assert np.all(index[m] == -1) and np.all(np.isnan(cost[m]))
    got = mv.first_guess_many(cand, obs, w, None, 3, is_gpu=False, space="pc")
    assert mv.last_routed_rows == 3
    band = mv.first_guess_many(cand, obs, w, None, 3, is_gpu=False, space="band")
    for m in (1, 3, 4):                                  # routed: the band result, bit for bit
        for u, v in zip(got, band):
            lc.same(u[m], v[m])
    assert np.all(band[2][1] == [0, 1, 2]) and np.all(band[1][1] == 0) and np.all(band[2][4] == -1)
    ok = [0, 2, 5]
    alone = mv.first_guess_many(cand, obs[ok], w[ok], None, 3, is_gpu=False, space="pc")
    assert mv.last_routed_rows == 0
    for u, v in zip(got, alone):                         # every other row is the call without those rows
        lc.same(u[ok], v)
    assert np.array_equal(got[2][ok], band[2][ok])


def test_nan_and_infinite_rows_and_a_nan_candidate(small):
    mv = small["mv"]
    B, mu = np.asarray(mv.basis_functions), small["mu"]
    obs, w = small["obs"][:5].copy(), small["w"][:5].copy()
    base = _lib.lut_search_pc_numpy(mu, B, obs, w, None, 3)
    o2, w2 = obs.copy(), w.copy()
    k = int(np.flatnonzero(w2[1])[0])
    o2[1, k] = np.inf
    w2[3, 0] = np.nan
    index, cost, status = _lib.lut_search_pc_numpy(mu, B, o2, w2, None, 3)
    assert status[1] != 0 and status[3] != 0 and np.all(index[[1, 3]] == -1) and np.all(np.isnan(cost[[1, 3]]))
    for m in (0, 2, 4):
        lc.same(index[m], base[0][m]), lc.same(cost[m], base[1][m])
    mu2 = mu.copy()
    mu2[2, int(base[0][0, 0])] = np.nan                  # the best candidate of row 0, out for every row
    index, cost, status = _lib.lut_search_pc_numpy(mu2, B, obs, w, None, 8)
    assert np.all(status == 0) and np.all(index >= 0) and not np.any(index == base[0][0, 0])


def test_argument_errors(small):
    mv, cand = small["mv"], small["cand"]
    B, mu, obs = np.asarray(mv.basis_functions), small["mu"], small["obs"][:3]
    with pytest.raises(ValueError):
        _lib.lut_search_pc_numpy(np.zeros((17, 30)), np.zeros((17, 40)), np.zeros(40))          # P > 16
    for n_best in (0, 9, 201):
        with pytest.raises(ValueError):
            _lib.lut_search_pc_numpy(mu, B, obs, None, None, n_best)
    with pytest.raises(ValueError):
        _lib.lut_search_pc_numpy(mu[:4], B, obs)                                                  # P of mu and basis
    with pytest.raises(ValueError):
        _lib.lut_search_pc_numpy(mu, B, obs[:, :20])
    with pytest.raises(ValueError):
        _lib.lut_search_pc_numpy(mu, B, obs, np.ones((2, 21)))
    with pytest.raises(ValueError):
        mv.first_guess_many(cand, obs, space="pcs", is_gpu=False)
    with pytest.raises(ValueError):
        mv.candidate_table(cand, space="spectra")
    # a table of the other space
    band = _first_guess.DeviceTable(None, F64, object(), (1, 21), 21, cand, mv)
    pcs = _first_guess.DeviceTable(None, F64, object(), (200, 1), 5, cand, mv, space="pc")
    assert band.space == "band" and pcs.space == "pc"
    with pytest.raises(ValueError, match="space"):
        band.check(mv, F64, 5, "pc")
    with pytest.raises(ValueError, match="space"):
        pcs.check(mv, F64, 21)
    pcs.check(mv, F64, 5, "pc"), band.check(mv, F64, 21)
    lib = _lib.load()
    rc = lib.gp_lut_search_pc_device(None, _lib.GP_F64, None, 1, 1, None, None, None, None, None, 0, None, None, None, 1, 1, 1, 1, 0)
    assert rc == -1 and lib.gp_last_error_string().decode() == "null context"
    rc = lib.gp_mv_lut_prepare_device(None, _lib.GP_F64, None, None, 0, None, 0, None, 0, None, None, None, None, 1, 1, 1)
    assert rc == -1 and lib.gp_last_error_string().decode() == "null context"
    assert lib.gp_lut_search_pc_geometry(_lib.GP_F64, 12, None, None, None, ctypes.byref(ctypes.c_int())) == 0


# ---- the launch plan ---------------------------------------------------------------------------------

def test_launch_plan():
    R, LT = 256, 64
    for dt, P, wgs in ((F64, 8, 2), (F64, 12, 1), (F64, 16, 1), (F32, 12, 2), (F32, 16, 2)):
        for cu in (256, 8):
            cap = cu * wgs
            for L in (4096, 32768, LT, 9):
                tiles = -(-L // LT)
                for M in (1, 255, 1000, 100000):
                    p = _lib.launch_plan("lut_search_pc", dt, M, n_pcs=P, n_candidates=L, compute_units=cu)
                    row_tiles = -(-M // R)
                    assert p["kernel"] == "lut_search_pc" and p["rows_per_item"] == R and p["candidate_tile"] == LT
                    assert p["padded_pcs"] == (8 if P <= 8 else 12 if P <= 12 else 16) and p["workgroups_per_cu"] == wgs
                    assert p["items"] == row_tiles * p["slices"] and 1 <= p["slices"] <= tiles
                    assert p["workgroups"] == min(p["items"], cap)
    # by hand, fp64, 12 PCs, 256 compute units: one workgroup per CU, cap 256.  1e5 rows are 391 row tiles, fewer than
    # four rounds: one round wants ceil(256 / 391) = 1 slice, four rounds ceil(1024 / 391) = 3 slices of the 64 tiles
    # (16 >= 3 allow it): slices of ceil(64 / 3) = 22 tiles are 3, items 1173
    p = _lib.launch_plan("lut_search_pc", F64, 100000, n_pcs=12, n_candidates=4096)
    assert p["slices"] == 3 and p["items"] == 1173 and p["workgroups"] == 256
    # fp32, the same call: cap 512, ceil(2048 / 391) = 6 slices of ceil(64 / 6) = 11 tiles -> 6 slices, 2346 items
    p = _lib.launch_plan("lut_search_pc", F32, 100000, n_pcs=12, n_candidates=4096)
    assert p["slices"] == 6 and p["items"] == 2346 and p["workgroups"] == 512
    # 1000 rows x 32768 candidates, fp64, 12 PCs: 4 row tiles, 512 candidate tiles; one round 64 slices, four rounds 256
    # but at most 512 // 4 = 128: slices of 4 tiles, 128 of them, 512 items on 256 workgroups
    p = _lib.launch_plan("lut_search_pc", F64, 1000, n_pcs=12, n_candidates=32768)
    assert p["slices"] == 128 and p["items"] == 512 and p["workgroups"] == 256
    with pytest.raises(_lib.GpuPredictError):
        _lib.launch_plan("lut_search_pc", F64, 10, n_pcs=17, n_candidates=5)
    with pytest.raises(_lib.GpuPredictError):
        _lib.launch_plan("lut_search_pc", F64, 10, n_pcs=0, n_candidates=5)
