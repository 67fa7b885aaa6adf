"""Device times of the pathwise posterior draws (sls_path_create / sls_path_maximize / sls_path_eval) per profiling scope, beside the
EI maximiser (sls_acq_maximize) on the same starts, and a rate probe of the random-feature contraction.
Writes one JSON document (default profiles/path_sample_timing.json) and prints it as one line.

    python tools/time_path_samples.py [--reps 3] [--out FILE]

Shapes: N = 2048 and 8192, D = 64, F = 2048, 64 draws x 1024 starts x 50 evaluations (the full-size case of the tests).  Times are
HIP-event device times of the scopes (sls_prof_get), averaged over --reps calls after one warm-up call; `wall_ms` is the host clock
around a whole call.  The EI maximiser runs once (after its own warm-up) on the same 65 536 starts with the same cap.
Rate probe: the every-draw evaluation (path_prior = path_feat_kernel, Theta = X~ Om^T on the matrix cores with its sincos epilogue
writing Phi, then Phi^T W on the tile GEMM) at D = 64 and D = 2 with the same (point, frequency, draw) counts.  The time that does not
depend on D is the epilogue's (one sincos and two stores per (point, frequency)) and the Phi^T W product's; the probe reports the
time ratio and the rates of both parts.  No hardware counters are read."""
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

PEAK_TFLOPS = 78.6      # fp64 (vector and MFMA), MI355X
SCOPES = ("path_setup", "path_solve", "cross_gram", "path_prior", "path_data", "path_grad_gemm", "grad_gemm", "lbfgs", "acq_gemm",
          "finalize")


def problem(N, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    return X, y, theta, rng


def scopes(ctx, reps):
    out = {}
    for name in SCOPES:
        ms, launches = ctx.prof_get(name)
        if launches:
            out[name] = {"ms": round(ms / reps, 3), "launches_per_call": launches / reps}
    return out


def shape(m, ctx, N, D, F, nd, S, n_local, reps):
    X, y, theta, rng = problem(N, D, N + D)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    starts = np.asfortranarray(rng.uniform(0.0, 1.0, (D, nd * S)))
    row = {"N": N, "D": D, "F": F, "draws": nd, "starts_per_draw": S, "n_local": n_local, "kernel": "SE"}
    # create
    m.PathSamples(gp, nd, F, seed=99).close()
    ctx.prof_enable(True)
    ctx.prof_reset()
    t0 = time.perf_counter()
    for r in range(reps):
        m.PathSamples(gp, nd, F, seed=100 + r).close()
    row["create"] = {"wall_ms": round((time.perf_counter() - t0) / reps * 1e3, 3), "stages": scopes(ctx, reps)}
    # maximise
    ps = m.PathSamples(gp, nd, F, seed=7)
    ps.maximize(starts, n_local)
    ctx.prof_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        res = ps.maximize(starts, n_local)
    st = scopes(ctx, reps)
    row["maximize"] = {"wall_ms": round((time.perf_counter() - t0) / reps * 1e3, 3), "device_ms": round(sum(v["ms"] for v in st.values()), 3),
                       "stages": st, "finite": bool(np.all(np.isfinite(res["value"])))}
    ps.close()
    # the EI maximiser on the same starts, same cap
    gp.acq_maximize(starts[:, :1024], n_local, want_all=False)
    ctx.prof_reset()
    t0 = time.perf_counter()
    gp.acq_maximize(starts, n_local, want_all=False)
    st = scopes(ctx, 1)
    row["ei_maximize_same_starts"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                                      "device_ms": round(sum(v["ms"] for v in st.values()), 3), "stages": st,
                                      "evals_issued": gp.last_stats()["evals_issued"]}
    ctx.prof_enable(False)
    gp.close()
    return row


def rate_probe(m, ctx, reps):
    """path_prior alone (eval_all: value only) at D = 64 and D = 2, the same (point, draw, frequency) count."""
    out = {}
    for D in (64, 2):
        X, y, theta, rng = problem(256, D, 5)
        gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
        F, nd, M = 4096, 256, 2048
        ps = m.PathSamples(gp, nd, F, seed=3)
        Xs = rng.uniform(0.0, 1.0, (D, M))
        ps.eval_all(Xs)
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(reps):
            ps.eval_all(Xs)
        ms, _ = ctx.prof_get("path_prior")
        ms /= reps
        ctx.prof_enable(False)
        Dp = (D + 15) // 16 * 16
        Fp = (F + 127) // 128 * 128
        theta_flop = 2.0 * M * Fp * Dp
        phiw_flop = 2.0 * M * 2 * Fp * ((nd + 127) // 128 * 128)
        out[f"D{D}"] = {"points": M, "draws": nd, "F": F, "ms": round(ms, 3),
                        "gflop_theta": round(theta_flop / 1e9, 2), "gflop_phi_w": round(phiw_flop / 1e9, 2),
                        "tflops_both_gemms": round((theta_flop + phiw_flop) / (ms * 1e-3) / 1e12, 2),
                        "gsincos_per_s": round(M * Fp / (ms * 1e-3) / 1e9, 1)}
        ps.close()
        gp.close()
    r = out["D64"]["ms"] / out["D2"]["ms"]
    out["time_ratio_D64_over_D2"] = round(r, 2)
    out["note"] = ("Theta's contraction depth grows 4x (Dp 16 -> 64) from D = 2 to D = 64; a ratio near 1 means the D-independent part "
                   "(sincos epilogue, Phi stores, Phi^T W) dominates")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "path_sample_timing.json"))
    args = ap.parse_args()
    m = sls()
    ctx = m.Context(0)
    doc = {"tool": "tools/time_path_samples.py", "peak_fp64_tflops": PEAK_TFLOPS, "reps": args.reps,
           "shapes": [shape(m, ctx, 2048, 64, 2048, 64, 1024, 50, args.reps), shape(m, ctx, 8192, 64, 2048, 64, 1024, 50, args.reps)],
           "prior_rate_probe": rate_probe(m, ctx, args.reps)}
    ctx.close()
    line = json.dumps(doc)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
