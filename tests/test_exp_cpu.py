"""Real<double>::exp_ of the kernel header, evaluated on the host against long double expl.

A small host program includes gp_predict_kernel.hpp (exp_ is __host__ __device__ for this purpose) and evaluates
2e6 arguments: uniform in [-760, 1], every half-integer multiple of ln 2 in that range with its neighbours up to
4 ulps either side (where the fused rounding fma(x, log2e, 1.5 2^52) and the parent's rint(x log2e) may pick
different n), -745.2, 0, the top of the range, the largest arguments with a finite result, and arguments with
denormal results.  The yardstick is the PARENT's exp_ (clamp, multiply, round, convert), kept verbatim in this
file's program and run on the same arguments: the new exp_'s maximum relative error may exceed the parent's by at
most 1.2e-16, the one extra rounding a different n can cost on |r| <= ln2/2 + 2^-52 (the degree-10 interpolant does
not degrade at that distance outside its interval).  The maximum is taken twice: over every argument with a non-zero
reference, as stated, where a correctly rounded denormal decides it for both implementations alike, and over the
normal results alone, where the bound bites.  Arguments below the underflow threshold give exactly 0, and so does
exp_clamped for NaN, -inf and -1e300."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gp_emulator_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXTRA = 1.2e-16
N_ARGS = 2000000

PROGRAM = r"""
#include "gp_predict_kernel.hpp"
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

// the parent's Real<double>::exp_, verbatim (Horner form)
static inline double parent_exp(double x) {
    x = __builtin_fmax(x, -1000.0);
    const double n = __builtin_rint(x * 1.4426950408889634);
    double r = fma(n, -6.93147180559945286e-01, x);
    r = fma(n, -2.31904681384629956e-17, r);
    double p = 2.76263485910095559e-07;
    p = fma(p, r, 2.76401812311866076e-06);
    p = fma(p, r, 2.48015043709117912e-05);
    p = fma(p, r, 1.98411702695461072e-04);
    p = fma(p, r, 1.38888889324666632e-03);
    p = fma(p, r, 8.33333338566834801e-03);
    p = fma(p, r, 4.16666666665732183e-02);
    p = fma(p, r, 1.66666666665544028e-01);
    p = fma(p, r, 5.00000000000000555e-01);
    p = fma(p, r, 1.00000000000000666e+00);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform01() {   // splitmix64, 53 bits
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

struct Worst { long double all = 0, normal = 0; double at_all = 0, at_normal = 0; };
static void take(Worst& w, double x, double got, long double ref) {
    const long double rel = fabsl(((long double)got - ref) / ref);
    if (rel > w.all) { w.all = rel; w.at_all = x; }
    if (ref >= (long double)DBL_MIN && rel > w.normal) { w.normal = rel; w.at_normal = x; }
}

int main(int argc, char** argv) {
    const long n_args = argc > 1 ? atol(argv[1]) : 2000000;
    std::vector<double> xs;
    xs.reserve(n_args + 16);
    const long double ln2 = 0.693147180559945309417232121458176568L;
    long n_half = 0;
    for (int m = -1097; m <= 1; ++m) {          // (m + 1/2) ln 2 in [-760, 1], +- 4 ulps
        const double c = (double)(((long double)m + 0.5L) * ln2);
        if (c < -760.0 || c > 1.0) continue;
        double lo = c, hi = c;
        xs.push_back(c);
        for (int u = 0; u < 4; ++u) {
            lo = nextafter(lo, -INFINITY);
            hi = nextafter(hi, INFINITY);
            xs.push_back(lo);
            xs.push_back(hi);
        }
        ++n_half;
    }
    const double special[] = {-745.2, 0.0, -0.0, 1.0, 700.0, 709.0, 709.78, 709.782712893384, -708.0, -708.3964185322641,
                              -708.4, -744.4400719213812, -745.0, -745.13, -745.1332191019411, -745.1332191019412};
    for (double s : special) xs.push_back(s);
    for (int i = 0; i < 20000; ++i) xs.push_back(-745.14 + (745.14 - 708.39) * uniform01());   // denormal results
    while ((long)xs.size() < n_args) xs.push_back(-760.0 + 761.0 * uniform01());

    Worst wp, wn;
    long differ = 0, zeros_bad = 0, zeros = 0, negative = 0;
    for (double x : xs) {
        const double gp_ = parent_exp(x), gn = gpk::Real<double>::exp_(x);
        differ += gp_ != gn;
        negative += !(gn >= 0.0);
        if (x < -745.14) {          // exp(x) < 2^-1075 below -745.1332191019412: rounds to 0
            ++zeros;
            zeros_bad += gn != 0.0;
            continue;
        }
        const long double ref = expl((long double)x);
        take(wp, x, gp_, ref);
        take(wn, x, gn, ref);
    }
    // far below the threshold, up to the bound the row guard leaves: |x log2e| < 2^31
    const double far_[] = {-746.0, -750.0, -760.0, -1000.0, -1075.0, -2.0e4, -1.0e6, -4.0e8, -1.0e9, -1.48e9};
    for (double x : far_) {
        ++zeros;
        zeros_bad += gpk::Real<double>::exp_(x) != 0.0;
    }
    printf("args %ld half_integer_points %ld\n", (long)xs.size(), n_half);
    printf("parent_all %.6Le at %.17g\n", wp.all, wp.at_all);
    printf("new_all %.6Le at %.17g\n", wn.all, wn.at_all);
    printf("parent_normal %.6Le at %.17g\n", wp.normal, wp.at_normal);
    printf("new_normal %.6Le at %.17g\n", wn.normal, wn.at_normal);
    printf("differ %ld\n", differ);
    printf("negative %ld\n", negative);
    printf("zeros %ld zeros_bad %ld\n", zeros, zeros_bad);
    printf("exp0 %.17g exp1 %.17g\n", gpk::Real<double>::exp_(0.0), gpk::Real<double>::exp_(1.0));
    // exp_clamped where its callers need their `poison`: NaN, -inf and an absurdly distant point all give 0
    printf("clamped nan %.17g ninf %.17g far %.17g zero %.17g\n", gpk::Real<double>::exp_clamped(NAN),
           gpk::Real<double>::exp_clamped(-INFINITY), gpk::Real<double>::exp_clamped(-1e300),
           gpk::Real<double>::exp_clamped(0.0));
    return 0;
}
"""


@pytest.fixture(scope="module")
def exp_report(tmp_path_factory):
    if not os.path.exists(HIPCC) and shutil.which(HIPCC) is None:
        pytest.fail("no hipcc to compile the host program with")
    d = tmp_path_factory.mktemp("exp_cpu")
    src, exe = d / "exp_check.hip", d / "exp_check"
    src.write_text(PROGRAM)
    # host pass only: the header's kernels are templates that nothing here instantiates.  Contraction off, so that
    # the host runs the fma calls as written and nothing else fused.
    cmd = [HIPCC, "--offload-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe), str(N_ARGS)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    print(r.stdout)
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] in ("parent_all", "new_all", "parent_normal", "new_normal"):
            out[f[0]] = float(f[1])
            out[f[0] + "_at"] = float(f[3])
        elif f and f[0] == "args":
            out["args"], out["half"] = int(f[1]), int(f[3])
        elif f and f[0] in ("differ", "negative"):
            out[f[0]] = int(f[1])
        elif f and f[0] == "zeros":
            out["zeros"], out["zeros_bad"] = int(f[1]), int(f[3])
        elif f and f[0] == "exp0":
            out["exp0"], out["exp1"] = float(f[1]), float(f[3])
        elif f and f[0] == "clamped":
            out["clamped"] = {f[i]: float(f[i + 1]) for i in range(1, len(f), 2)}
    return out


def test_argument_set(exp_report):
    """2e6 arguments, every half-integer multiple of ln 2 in [-760, 1] among them, and a share below the threshold."""
    assert exp_report["args"] >= N_ARGS
    assert exp_report["half"] >= 1095
    assert exp_report["zeros"] > 10000


def test_error_against_parent(exp_report):
    """Maximum relative error against expl: at most the parent's + 1.2e-16, over all arguments and over the normal
    results alone.  The parent's own error on the normal results is the interpolant's: a few 1e-16."""
    for key in ("all", "normal"):
        parent, new = exp_report["parent_" + key], exp_report["new_" + key]
        print("EXP %-6s parent %.6e (x = %.17g)  new %.6e (x = %.17g)" %
              (key, parent, exp_report["parent_%s_at" % key], new, exp_report["new_%s_at" % key]))
        assert new <= parent + EXTRA, (key, parent, new)
    assert exp_report["parent_normal"] < 1e-15      # the harness measures what it says it does
    print("EXP results that differ from the parent's: %d of %d" % (exp_report["differ"], exp_report["args"]))


def test_exact_zero_below_underflow(exp_report):
    assert exp_report["zeros_bad"] == 0
    assert exp_report["negative"] == 0


def test_exact_points(exp_report):
    assert exp_report["exp0"] == 1.0
    assert abs(exp_report["exp1"] - 2.718281828459045) <= 4.5e-16


def test_exp_clamped_turns_nan_and_infinity_into_zero(exp_report):
    """exp_clamped(NaN), exp_clamped(-inf) and exp_clamped(-1e300) are exactly 0 (the clamp is a max with -1000, which
    drops a NaN): the reason every caller adds its row `poison` (tests/test_far_rows_kernels_gpu.py)."""
    c = exp_report["clamped"]
    assert set(c) == {"nan", "ninf", "far", "zero"}
    assert c["nan"] == 0.0 and c["ninf"] == 0.0 and c["far"] == 0.0
    assert c["zero"] == 1.0
