"""Device times of the joint posterior (sls_gp_sample_posterior = predict_cov + chol(cov + j I) + samples) per profiling scope, with
the algorithmic flops of each stage and its share of the fp64 MFMA peak.  Prints ONE JSON line (committed as
profiles/posterior_timing.json).

    python tools/time_posterior.py [--reps 5]

Shapes: (N = 2048, D = 16, M = 4096, S = 64), the C2 shape of BASELINE.md, and (N = 90, D = 32, M = 200, S = 64), the reference's
own regime.  Times are HIP-event device times of the scopes (sls_prof_get), averaged over --reps calls after one warm-up call;
`wall_ms` is the host clock around a whole call (uploads, the jitter's synchronisation and the M x S download included)."""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
from util import sls  # noqa: E402

PEAK_TFLOPS = 78.6      # fp64 MFMA, MI355X
SCOPES = ("cross_gram", "finalize", "post_v", "post_cov", "post_potrf", "post_sample")


def shape(m, ctx, N, D, M, S, kernel, reps, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 1.0, (D, M))
    theta = np.concatenate([[0.5], np.full(D, 0.5)])
    gp = m.GP(ctx, X, y, theta, 0.005, kernel)
    gp.sample_posterior(Xs, S, 1)                  # warm-up: code objects, pooled blocks
    ctx.prof_enable(True)
    ctx.prof_reset()
    t0 = time.perf_counter()
    jit = 0.0
    for r in range(reps):
        _, jit = gp.sample_posterior(Xs, S, 1 + r)
    wall = (time.perf_counter() - t0) / reps * 1e3
    flops = {"post_v": M * N * N, "post_cov": M * M * N, "post_potrf": M ** 3 / 3, "post_sample": M * M * S}
    stages = {}
    for name in SCOPES:
        ms, launches = ctx.prof_get(name)
        ms /= reps
        e = {"ms": round(ms, 4), "launches_per_call": launches / reps}
        if name in flops:
            e["gflop"] = round(flops[name] / 1e9, 3)
            e["tflops"] = round(flops[name] / (ms * 1e-3) / 1e12, 2) if ms > 0 else None
            e["frac_of_peak"] = round(flops[name] / (ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3) if ms > 0 else None
        stages[name] = e
    ctx.prof_enable(False)
    gp.close()
    dev = sum(v["ms"] for v in stages.values())
    tot = sum(flops.values())
    return {"N": N, "D": D, "M": M, "samples": S, "kernel": "SE" if kernel == 0 else "Matern52", "jitter_used": jit,
            "device_ms": round(dev, 4), "wall_ms": round(wall, 3), "total_gflop": round(tot / 1e9, 2),
            "lower_bound_ms_at_peak": round(tot / (PEAK_TFLOPS * 1e12) * 1e3, 4), "stages": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    m = sls()
    ctx = m.Context(0)
    rows = [shape(m, ctx, 2048, 16, 4096, 64, m.KERNEL_SE, args.reps, 11),
            shape(m, ctx, 90, 32, 200, 64, m.KERNEL_MATERN52, args.reps, 12)]
    ctx.close()
    print(json.dumps({"tool": "tools/time_posterior.py", "peak_fp64_mfma_tflops": PEAK_TFLOPS, "reps": args.reps,
                      "shapes": rows}))


if __name__ == "__main__":
    main()
