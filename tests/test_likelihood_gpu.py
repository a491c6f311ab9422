"""The training objective's kernels (gp_likelihood_batch_f64) against the 80-bit truth of likelihood_cases.py.

Every compiled instance runs: launch_likelihood (gp_train_tu.hip) takes likelihood_mfma_kernel<DM> for N <= 256 and
likelihood_kernel + likelihood_grad_kernel<DM> above (or everywhere in a process started with GP_TRAIN_GENERIC=1),
DM = 4, 8, 12, 16 the smallest >= D; the case list holds both ends of every DM class on both algorithms, N mod 16 in
1..8 and 9..16, block rows 7, 8 and 15 of the register-resident kernel, the unpadded 256, and last panels of 1, 4, 7
and 8 pivots in the workspace kernel.  Each printed line names the instance its case ran.

The bound is likelihood_cases' K kappa u with K = 8 for the inverse, invQt, the cost and the gradient (the last
against its term magnitude); equalities between launches (batch size, neighbours, want_inverse, a dirty scratch
buffer) are bitwise: a set's arithmetic does not depend on what else is in the launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import likelihood_cases as lc

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [lc.key_id(k) for k in lc.CASE_KEYS]
NAMES = ("cost", "grad", "invQ", "invQt")


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    assert int(os.environ.get("GP_TRAIN_GENERIC", "0") or 0) == 0, "this file tests the default dispatch"
    return _lib.default_context(0)


def run(ctx, thetas, X, t, inverse=True):
    """dict(cost (E,), grad (E, D + 2)[, invQ (E, N, N), invQt (E, N)]) of one launch."""
    return dict(zip(NAMES, ctx.likelihood_batch(np.atleast_2d(thetas), X, t, want_inverse=inverse)))


def one(res, e):
    return {k: v[e] for k, v in res.items()}


def same_bits(a, b, names=NAMES):
    for k in names:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), k


def label(key, generic=False):
    N, D = lc.case(key)[0].shape
    return "%s%s %s" % ("GP_TRAIN_GENERIC " if generic else "", lc.instance(N, D, generic), lc.key_id(key))


_in_process = {}


def evaluated(ctx, key):
    if key not in _in_process:
        X, t, theta = lc.case(key)
        _in_process[key] = one(run(ctx, theta, X, t), 0)
    return _in_process[key]


# ---- a. every instance against the truth ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", lc.CASE_KEYS, ids=IDS)
def test_every_instance_meets_the_truth(ctx, key):
    got = evaluated(ctx, key)
    lc.check(lc.truth_of(key), label=label(key), **got)
    invQ = got["invQ"]
    if invQ.shape[0] <= 256:         # the mirror image is stored from the same register
        assert np.array_equal(invQ, invQ.T)
    else:
        assert np.max(np.abs(invQ - invQ.T)) <= 1e-15 * np.max(np.abs(invQ))


# ---- b. want_inverse=False ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(16, 4), (17, 6), (24, 9), (8, 13), (257, 4), (257, 8), (264, 12), (257, 13)])
def test_cost_and_gradient_do_not_depend_on_want_inverse(ctx, n, d):
    """One case per instance: without the inverse the register-resident kernel stores the lower triangle only."""
    X, t, theta = lc.case((n, d, -9))
    same_bits(run(ctx, theta, X, t, inverse=False), run(ctx, theta, X, t), ("cost", "grad"))


def test_lower_triangle_only_over_a_dirty_scratch_buffer(ctx):
    """The scratch buffer holds a workspace-kernel batch's matrices when the small case writes its lower triangle over
    them; then the full inverse; then the lower triangle again over that."""
    Xw, tw, thw = lc.case((257, 4, -4))
    run(ctx, np.tile(thw, (3, 1)), Xw, tw, inverse=False)
    X, t, theta = lc.case((24, 9, -4))
    first = run(ctx, theta, X, t, inverse=False)
    full = run(ctx, theta, X, t)
    again = run(ctx, theta, X, t, inverse=False)
    same_bits(first, full, ("cost", "grad"))
    same_bits(again, full, ("cost", "grad"))
    lc.check(lc.truth_of((24, 9, -4)), label="dirty scratch " + label((24, 9, -4)), **one(full, 0))


# ---- c. batch independence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(24, 9), (129, 7), (257, 4)])
def test_a_set_does_not_depend_on_the_rest_of_the_launch(ctx, n, d):
    """E = 1, 2, 5 and 300 (more workgroups than the 256 CUs; 300 x 257^2 doubles of workspace), every set with its own
    theta and targets: sets 0, 1, 255, 256, 257, 299 of the largest launch carry the bits of their solo launches."""
    X, t, theta = lc.case((n, d, -4))
    rs = np.random.RandomState(7 * n + d)
    E = 300
    thetas = theta + 0.05 * rs.standard_normal((E, d + 2))
    tg = t + 0.01 * rs.standard_normal((E, n))
    big = run(ctx, thetas, X, tg)
    for e in (0, 1, 255, 256, 257, 299):
        same_bits(one(big, e), one(run(ctx, thetas[e], X, tg[e:e + 1]), 0))
    for sub in (2, 5):
        part = run(ctx, thetas[:sub], X, tg[:sub])
        for e in range(sub):
            same_bits(one(part, e), one(big, e))
    same_bits(run(ctx, thetas, X, tg, inverse=False), big, ("cost", "grad"))
    for e in (0, 256, 299):
        lc.check(lc.truth(X, tg[e], thetas[e]), label="set %d of %d, %s" % (e, E, lc.instance(n, d)), **one(big, e))
    same_bits(run(ctx, thetas[:5], X, t), run(ctx, thetas[:5], X, np.tile(t, (5, 1))))   # shared targets == tiled


# ---- d. a singular set poisons only itself ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20, 258])
def test_a_singular_set_poisons_only_itself(ctx, n):
    """Duplicated inputs; set 2 has no noise (theta = -800, as test_gpu_objective_reports_a_non_positive_definite_matrix),
    so its matrix is singular and its cost not finite.  Its neighbours keep the bits of their solo launches."""
    X = np.repeat(np.random.RandomState(0).random_sample((n // 2, 2)), 2, axis=0)
    t = np.sin(X.sum(1))
    thetas = np.array([[0.0, 0.0, 0.0, -4.0], [0.1, -0.1, 0.0, -4.0], [0.0, 0.0, 0.0, -800.0], [-0.2, 0.2, 0.1, -3.0]])
    with np.errstate(all="ignore"):
        batch = run(ctx, thetas, X, t)
    assert not np.isfinite(batch["cost"][2])
    for e in (0, 1, 3):
        solo = one(run(ctx, thetas[e], X, t), 0)
        assert np.isfinite(solo["cost"]) and np.all(np.isfinite(solo["invQ"]))
        same_bits(one(batch, e), solo)


# ---- e. the 256 / 257 seam between the two algorithms ---------------------------------------------------------------
@pytest.mark.parametrize("noise", lc.NOISES)
def test_seam_between_the_two_algorithms(ctx, noise):
    """One X of 257 rows: its first 256 rows run the register-resident kernel, all 257 the workspace kernel.  Both meet
    the truth and the two costs differ by what the truth says, within the sum of the two bounds."""
    X, t, theta = lc.case((257, 8, noise))
    hi, tr_hi = evaluated(ctx, (257, 8, noise)), lc.truth_of((257, 8, noise))
    lo, tr_lo = one(run(ctx, theta, X[:256], t[:256]), 0), lc.truth(X[:256], t[:256], theta)
    lc.check(tr_hi, label="seam 257 " + lc.instance(257, 8), **hi)
    lc.check(tr_lo, label="seam 256 " + lc.instance(256, 8), **lo)
    got = lc.LD(float(hi["cost"])) - lc.LD(float(lo["cost"]))
    bound = lc.K * lc.U * (tr_hi["cond"] * max(1, abs(tr_hi["cost"])) + tr_lo["cond"] * max(1, abs(tr_lo["cost"])))
    print("seam noise %d: cost step %.17g, truth %.17g, bound %.3g" % (noise, got, tr_hi["cost"] - tr_lo["cost"], bound))
    assert abs(got - (tr_hi["cost"] - tr_lo["cost"])) <= bound


# ---- f. limits -----------------------------------------------------------------------------------------------------
def test_sizes_past_the_compiled_limits_are_refused(ctx):
    rs = np.random.RandomState(3)
    for n, d in [(513, 3), (10, 17), (513, 17)]:
        X = rs.random_sample((n, d))
        with pytest.raises(_lib.GpuPredictError, match="compiled for n_train <= 512, n_inputs <= 16"):
            ctx.likelihood_batch(np.zeros((1, d + 2)), X, np.sin(X.sum(1)), want_inverse=True)
        key = (24, 9, -4)                                    # the context still works
        X, t, theta = lc.case(key)
        lc.check(lc.truth_of(key), label="after a refused call, " + label(key), **one(run(ctx, theta, X, t), 0))


# ---- g. the A/B switch ----------------------------------------------------------------------------------------------
def test_workspace_kernel_at_small_sizes(ctx, tmp_path):
    """GP_TRAIN_GENERIC=1 is read once per process: ONE fresh child process (likelihood_cases.py as a program) runs
    lc.AB_KEYS through the workspace kernel; its results meet the truth, and the register-resident kernel's results
    of this process within the sum of the two bounds."""
    out = str(tmp_path / "generic.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(lc.__file__), out]
    child = subprocess.run(cmd, env=dict(os.environ, GP_TRAIN_GENERIC="1"), cwd=ROOT, timeout=120,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert child.returncode == 0, "child exited with %d:\n%s" % (child.returncode, child.stdout)
    differ = 0
    with np.load(out, allow_pickle=False) as f:
        for key in lc.AB_KEYS:
            got = {k: f[lc.key_id(key) + "/" + k] for k in NAMES}
            tr = lc.truth_of(key)
            lc.check(tr, label=label(key, generic=True), **got)
            here = evaluated(ctx, key)
            lc.check(tr, label="A/B " + lc.key_id(key), other=here, **got)
            differ += not np.array_equal(got["invQ"], here["invQ"])
    assert differ > 0, "the child computed the parent's bits in every case: did it run the workspace kernel?"
