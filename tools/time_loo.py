"""Device times of leave-one-out cross-validation (sls_nll_loo) per profiling scope, beside sls_nll_eval with gradient on the same
handle in the same run, the symmetric product against the full product of the generic GEMM on the same operands, and the cost of the
300 single value calls of a LOO fit's DIRECT phase.  Writes one JSON document (default profiles/loo_timing.json) and prints it as one
line.

    python tools/time_loo.py [--out FILE]

Shapes: N = 2048, D = 16 and N = 4096, D = 128 (Matern 5/2).  Scope times are HIP-event device times (sls_prof_get), whole calls are
host-clock times around the call (each ends in a synchronisation); every figure is the mean of 3 calls after one warm-up call.  Every
timed call alternates between two noise levels, so that it pays for its own factorisation (a repeated (theta, b) would re-use the
cached factor); `cached` rows repeat (theta, b) on purpose.  `loo_syrk` holds the scaled copy R = Kinv diag(sqrt c) and the product;
SLS_LOO_SYRK=0 switches the product to launch_gemm_plain's full R R^T (every tile) for the comparison.  The fraction of peak is N^3
flop over the scope's time against 78.6 TFLOP/s.  No hardware counters are read."""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
from util import env_switch, sls  # noqa: E402

SCOPES = ("loo_terms", "loo_syrk", "loo_weight")
PEAK_TFLOPS = 78.6
REPS = 3


def mean_of(ctx, call, reps=REPS):
    """Mean wall time (ms) and mean scope times of `reps` calls of call(i) after one warm-up call."""
    call(-1)
    ctx.prof_reset()
    t0 = time.perf_counter()
    for i in range(reps):
        call(i)
    wall = (time.perf_counter() - t0) * 1e3 / reps
    row = {"wall_ms": round(wall, 4)}
    for name in SCOPES:
        ms, launches = ctx.prof_get(name)
        if launches:
            row[name + "_ms"] = round(ms / launches, 4)
    return row


def shape(m, ctx, N, D):
    rng = np.random.default_rng(N + D)
    X = np.asfortranarray(rng.uniform(0.0, 1.0, (D, N)))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    bs = (0.01, 0.011)
    h = m.Nll(ctx, X, m.KERNEL_MATERN52)
    doc = {"N": N, "D": D, "kernel": "matern52"}
    ctx.prof_enable(True)
    doc["nll_eval_grad"] = mean_of(ctx, lambda i: h.eval(y, theta, bs[i & 1]))
    doc["loo_grad"] = mean_of(ctx, lambda i: h.loo(y, theta, bs[i & 1]))
    doc["loo_value_only"] = mean_of(ctx, lambda i: h.loo(y, theta, bs[i & 1], want_grad=False))
    doc["loo_grad_cached"] = mean_of(ctx, lambda i: h.loo(y, theta, bs[0]))
    doc["loo_value_only_cached"] = mean_of(ctx, lambda i: h.loo(y, theta, bs[0], want_grad=False))
    with env_switch("SLS_LOO_SYRK", 0):
        doc["loo_grad_cached_full_product"] = mean_of(ctx, lambda i: h.loo(y, theta, bs[0]))
    # the whole syrk scope = scaled copy + product
    syrk, full = doc["loo_grad_cached"]["loo_syrk_ms"], doc["loo_grad_cached_full_product"]["loo_syrk_ms"]
    doc["loo_syrk_fraction_of_fp64_mfma_peak_at_N3_flop"] = round(float(N) ** 3 / (syrk * 1e-3) / (PEAK_TFLOPS * 1e12), 4)
    doc["loo_syrk_floor_ms"] = round(float(N) ** 3 / (PEAK_TFLOPS * 1e12) * 1e3, 4)
    doc["full_product_over_syrk"] = round(full / syrk, 3)
    doc["loo_grad_over_nll_eval_grad"] = round(doc["loo_grad"]["wall_ms"] / doc["nll_eval_grad"]["wall_ms"], 3)
    # DIRECT phase of a LOO fit: 300 single value-only calls at distinct hyper-parameters (sls_gp_loo_grad without gradient)
    xs = np.exp(rng.uniform(np.log(0.05), np.log(2.0), (300, D + 2)))
    xs[:, 1] = np.exp(rng.uniform(np.log(1e-4), np.log(1e-1), 300))
    h.gp_loo_objective(y, xs[0], want_grad=False)
    t0 = time.perf_counter()
    for x in xs:
        h.gp_loo_objective(y, x, want_grad=False)
    doc["direct_phase_300_value_calls_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    doc["extra_device_memory_bytes"] = {"M": 8 * h_np(N) ** 2, "vectors": 8 * 6 * h_np(N)}
    ctx.prof_enable(False)
    h.close()
    return doc


def h_np(N):
    return (N + 127) // 128 * 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "loo_timing.json"))
    a = ap.parse_args()
    m = sls()
    ctx = m.Context(0)
    doc = {"calls_per_figure": REPS, "fp64_mfma_peak_tflops": PEAK_TFLOPS, "shapes": [shape(m, ctx, 2048, 16), shape(m, ctx, 4096, 128)]}
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
