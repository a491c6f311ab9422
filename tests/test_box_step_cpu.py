"""The bound-constrained damped Newton step on the host: box_step_numpy returns the minimiser of the damped model in
the box (the KKT certificate of box_step_cases.py, in np.longdouble from the inputs as given), the retrieval loops take
it with bounds_mode="active_set", and return_active reports the active set and the scaled projected gradient."""
import numpy as np
import pytest

import box_step_cases as bc

from gp_emulator_amd import _lib, _retrieve, perband


def numpy_step(case, damping="diagonal"):
    return _lib.box_step_numpy(case["x"], case["grad"], case["A"], case["lam"], damping, case["prior"], case["bounds"])


@pytest.mark.parametrize("prior", [None, "shared", "rows"])
@pytest.mark.parametrize("D", bc.DIMS)
def test_numpy_step_is_a_kkt_point(D, prior):
    """0 %, about 30 % and about 60 % of the components start on a bound; both damping modes; no row reaches the cap."""
    worst, most = 0.0, 0
    for share in bc.SHARES:
        case = bc.seeded(D, 67, np.float64, share, prior)
        for damping in ("diagonal", "identity"):
            out = numpy_step(case, damping)
            assert out[0].dtype == out[1].dtype == np.float64 and out[2].dtype == out[5].dtype == np.int32
            assert out[3].dtype == out[4].dtype == np.uint32
            worst = max(worst, bc.check_kkt(case, *out, damping=damping))
            most = max(most, int(out[5].max()))
    print("D = %d prior %s: worst residual / bound %.3g, most passes %d (cap %d)" % (D, prior, worst, most, 3 * D + 4))


@pytest.mark.parametrize("D", bc.DIMS)
def test_nothing_active_is_the_newton_step_in_one_pass(D):
    """Bounds nothing can touch: one pass, zero masks, and step, trial and status are newton_step_numpy's bit for bit."""
    case = bc.seeded(D, 67, np.float64, 0.0, "shared", wide=True)
    step, trial, status, at_lo, at_hi, passes = numpy_step(case)
    assert np.all(passes == 1) and not at_lo.any() and not at_hi.any() and not status.any()
    ref = _lib.newton_step_numpy(case["x"], case["grad"], case["A"], case["lam"], "diagonal", case["prior"], case["bounds"])
    for a, b in zip((step, trial, status), ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_a_start_outside_the_box_is_moved_in_and_nan_rows_are_poisoned():
    D, M = 3, 9
    case = bc.seeded(D, M, np.float64, 0.3, "shared")
    case["x"][0] = [-0.5, 1.5, 0.5]                      # outside on both sides
    out = numpy_step(case)
    bc.check_kkt(case, *out)
    bad = dict(case, x=case["x"].copy(), grad=case["grad"].copy())
    bad["x"][2, 1], bad["grad"][5, 0] = np.nan, np.inf
    got = numpy_step(bad)
    keep = np.ones(M, bool)
    keep[[2, 5]] = False
    for a, b in zip(got, out):
        assert np.array_equal(a[keep], b[keep])
    for m in (2, 5):
        assert np.all(np.isnan(got[0][m])) and np.all(np.isnan(got[1][m]))
        assert got[2][m] == 0 and got[3][m] == 0 and got[4][m] == 0 and got[5][m] == 0


def test_a_failed_pivot_names_itself():
    """A rank-deficient matrix without damping: status k + 1, step 0, trial x, zero masks."""
    D, M = 4, 5
    case = bc.seeded(D, M, np.float64, 0.0)
    v = np.array([1.0, -2.0, 0.5, 0.0])
    case["A"][3] = np.outer(v, v)                        # rank 1: pivot 1 is exactly 0 (1 * 4 - 2 * 2)
    case["lam"] = np.zeros(M)
    step, trial, status, at_lo, at_hi, passes = numpy_step(case)
    assert status[3] == 2 and not step[3].any() and np.array_equal(trial[3], case["x"][3]) and at_lo[3] == at_hi[3] == 0
    assert not status[[0, 1, 2, 4]].any()


def run(mode, **kw):
    c = bc.loop_case()
    return perband.retrieve_bands(c["gps"], c["X0"], c["obs"], c["weights"], bounds=c["bounds"], is_gpu=False, bounds_mode=mode, **kw)


def test_the_loop_converges_where_the_clamp_creeps():
    """retrieve_bands on truths outside the box, both modes from the same start: the active-set loop has no fewer
    converged rows, and no row ends at a higher F (there is no prior: F is the returned cost) beyond the rounding of F."""
    clamp, box = run("clamp", return_active=True), run("active_set", return_active=True)
    share = lambda out: float(np.mean(out[2] == 1))                                          # noqa: E731
    print("converged: clamp %.0f %%, active set %.0f %%;  median kkt: clamp %.3g, active set %.3g;  median cost %.4g / %.4g"
          % (100 * share(clamp), 100 * share(box), np.median(clamp[-1]), np.median(box[-1]), np.median(clamp[1]), np.median(box[1])))
    assert np.any(box[-2] != 0), "the case does not lean on its bounds"
    assert share(box) >= share(clamp)
    # F is a sum of E = 6 terms 1/2 w r^2 from a GP mean of N = 30 terms: a few hundred roundings of 2^-53 at most
    assert np.all(box[1] <= clamp[1] * (1 + 1024 * 2.0 ** -53))
    c = bc.loop_case()
    assert np.all(box[0] >= c["bounds"][0]) and np.all(box[0] <= c["bounds"][1])
    for a, b in zip(run("clamp"), perband.retrieve_bands(c["gps"], c["X0"], c["obs"], c["weights"], bounds=c["bounds"], is_gpu=False)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_return_active_shapes_and_what_it_says():
    c = bc.loop_case()
    E, D, M = bc.LOOP["E"], bc.LOOP["D"], bc.LOOP["M"]
    prior = (np.full(D, 0.5), 4.0 * np.eye(D))
    out = run("active_set", return_active=True, return_cov=True, return_A=True, prior=prior)
    assert len(out) == 5 + 3 + 1 + 2
    active, kkt = out[-2:]
    assert active.shape == (M, D) and active.dtype == np.int8 and kkt.shape == (M,) and kkt.dtype == np.float64
    X, A = out[0], out[8]
    _, grad, _ = perband.misfit_bands(c["gps"], X, c["obs"], c["weights"], second_order="gauss_newton", is_gpu=False)
    g = grad + (X - prior[0]) @ prior[1].T
    want = np.where((X <= 0.0) & (g > 0), -1, np.where((X >= 1.0) & (g < 0), 1, 0))
    assert np.array_equal(active, want)
    scaled = np.abs(g) / np.sqrt(np.einsum("mii->mi", A) + np.diag(prior[1]))
    assert np.allclose(kkt, np.max(np.where(want == 0, scaled, 0.0), axis=1), rtol=1e-12, atol=0)
    assert np.all(np.isin(active[(X > 0.0) & (X < 1.0)], 0))
    # the plain five are what they are without the argument
    for a, b in zip(out[:5], run("active_set", prior=prior)):
        assert np.array_equal(a, b)


def test_argument_rules():
    c = bc.loop_case()
    args = (c["gps"], c["X0"], c["obs"], c["weights"])
    with pytest.raises(ValueError):
        perband.retrieve_bands(*args, is_gpu=False, bounds_mode="active_set")                 # no bounds
    with pytest.raises(ValueError):
        perband.retrieve_bands(*args, is_gpu=False, return_active=True)                        # no bounds
    with pytest.raises(ValueError):
        perband.retrieve_bands(*args, bounds=c["bounds"], is_gpu=False, bounds_mode="project")
    D = bc.LOOP["D"]
    prior, noise = (np.full(D, 0.5), np.eye(D)), 0.01 * np.eye(D)
    with pytest.raises(ValueError):
        perband.retrieve_bands_joint(c["gps"], c["X0"], c["obs"][None], None, prior, noise, bounds=c["bounds"], is_gpu=False,
                                     bounds_mode="active_set")
    with pytest.raises(ValueError):
        _retrieve.clamp_only("active_set")
    with pytest.raises(ValueError):
        _lib.box_step_numpy(np.zeros((1, 2)), np.zeros((1, 2)), np.eye(2)[None], 1.0)          # the bounds are required
    assert hasattr(_lib.Context, "box_step") and hasattr(_lib.Context, "box_step_device")
    assert "gp_box_step_device" in _lib.SIGNATURES


def test_retrieve_many_takes_the_arguments():
    """MultivariateEmulator.retrieve_many on the same case: the same rules and, on the numpy branch, the same direction."""
    c = bc.mv_case()
    em, obs, Y0, bounds, w = (c[k] for k in ("mv", "obs", "Y0", "bounds", "weights"))
    D = Y0.shape[1]
    with pytest.raises(ValueError):
        em.retrieve_many(Y0, obs, w, is_gpu=False, bounds_mode="active_set")
    with pytest.raises(ValueError):
        em.retrieve_many(Y0, obs, w, is_gpu=False, return_active=True)
    with pytest.raises(ValueError):
        em.retrieve_joint(Y0, obs[None], None, (np.full(D, 0.5), np.eye(D)), 0.01 * np.eye(D), bounds=bounds, is_gpu=False,
                          bounds_mode="active_set")
    clamp = em.retrieve_many(Y0, obs, w, bounds=bounds, is_gpu=False, return_active=True)
    box = em.retrieve_many(Y0, obs, w, bounds=bounds, is_gpu=False, bounds_mode="active_set", return_active=True)
    print("retrieve_many converged: clamp %.0f %%, active set %.0f %%" % (100 * np.mean(clamp[2]), 100 * np.mean(box[2])))
    assert box[-2].shape == Y0.shape and box[-2].dtype == np.int8 and box[-1].shape == (Y0.shape[0],)
    assert np.mean(box[2]) >= np.mean(clamp[2])
    for a, b in zip(clamp[:5], em.retrieve_many(Y0, obs, w, bounds=bounds, is_gpu=False)):
        assert np.array_equal(a, b)
