#!/usr/bin/env python3
"""The variance-gradient kernel (gp_predict_var_grad_device) against the full predict on the same model and rows, in
the same process; one JSON line per result.

    python tools/var_grad_timing.py [--legs time,registers] [--reps 20] [--warmup 5] [--nk 63,80]

  time       N = 250, D = 11, 1e6 rows resident in HBM, fp64 and fp32: median of --reps HIP-event-timed launches after
             --warmup, predict_device, then predict_var_grad_device (whose first warm-up call builds the operand)
  registers  no GPU: compiles gp_var_grad_tu.hip for --nk with the build's flags to assembly and prints VGPRs, spilled
             VGPRs, scratch bytes and LDS bytes of every var_grad_kernel instance
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib, build as gpbuild  # noqa: E402
from oracle import gp_oracle  # noqa: E402
from mean_grad_timing import median_ms  # noqa: E402


def leg_time(a):
    N, D, M = 250, 11, 1_000_000
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(3, N, D, M)
    ctx = _lib.default_context(0)
    for prec in (np.float64, np.float32):
        m = _lib.Model(ctx, np.exp(theta), inputs, invQt, invQ, prec)
        isz = np.dtype(prec).itemsize
        d_t = ctx.to_device(np.ascontiguousarray(testing, dtype=prec))
        d_mu, d_var, d_der = ctx.malloc(M * isz), ctx.malloc(M * isz), ctx.malloc(M * D * isz)
        tp = median_ms(ctx, lambda: m.predict_device(d_t, d_mu, d_var, d_der, M), a.reps, a.warmup)
        tv = median_ms(ctx, lambda: m.predict_var_grad_device(d_t, d_var, d_der, M), a.reps, a.warmup)
        print(json.dumps(dict(leg="resident", dtype=np.dtype(prec).name, n_train=N, n_inputs=D, rows=M,
                              predict_ms=round(tp, 4), var_grad_ms=round(tv, 4), ratio=round(tv / tp, 3),
                              var_grad_points_per_s=round(M / (tv * 1e-3), 0),
                              operand_bytes=m.info()["var_grad_bytes"])), flush=True)
        for p in (d_t, d_mu, d_var, d_der):
            ctx.free(p)
        m.close()


def leg_registers(a):
    with tempfile.TemporaryDirectory() as tmp:
        for nk in [int(x) for x in a.nk.split(",")]:
            for ctype in ("double", "float"):
                out = os.path.join(tmp, "vg_%s_%d.s" % (ctype, nk))
                cmd = [gpbuild.HIPCC] + gpbuild.FLAGS + ["-DGP_T=" + ctype, "-DGP_NK=%d" % nk, "--cuda-device-only", "-S",
                                                         os.path.join(gpbuild.CSRC, "gp_var_grad_tu.hip"), "-o", out]
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                text = open(out).read()
                # the kernels' metadata records: one block of "    .key: value" lines per kernel
                for block in re.split(r"\n  - \.agpr_count:", text)[1:]:
                    rec = dict(re.findall(r"\n\s+\.(\w+):\s+(\S+)", "\n" + block))
                    mt = re.search(r"var_grad_kernelI([df])Li(\d+)ELi(\d+)E", rec.get("name", ""))
                    if not mt:
                        continue
                    print(json.dumps(dict(leg="registers", dtype="float64" if mt.group(1) == "d" else "float32",
                                          kernel_d=int(mt.group(2)), nk=int(mt.group(3)), vgprs=int(rec["vgpr_count"]),
                                          vgprs_spilled=int(rec["vgpr_spill_count"]),
                                          scratch_bytes=int(rec["private_segment_fixed_size"]),
                                          lds_bytes=int(rec["group_segment_fixed_size"]))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="time")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nk", default="63")
    a = ap.parse_args()
    for leg in a.legs.split(","):
        {"time": leg_time, "registers": leg_registers}[leg](a)
