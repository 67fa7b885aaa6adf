"""Device times of the joint entropy search maximiser (sls_jes_maximize) per profiling scope, beside the max-value entropy search
maximiser (sls_mes_maximize) on the same starts in the same process.  Writes one JSON document (default profiles/jes_timing.json) and
prints it as one line.

    python tools/time_jes.py [--out FILE] [--N 8192] [--starts 65536] [--n-local 50]

Shape: N = 8192, D = 64, SE kernel, 65 536 starts, 50 evaluations per start, K = 64 and K = 1024 optima (locations near the best data
points, values around max(y): the cost of no stage depends on where they lie).  Times are HIP-event device times of the scopes
(sls_prof_get) of ONE call after a two-round warm-up call of the same shape; `wall_ms` is the host clock around the call.  Per round:
the scope's time over the rounds the call executed (sls_acq_last_stats); the active set shrinks from round to round, so this is an
average over the set sizes of the run.  MES runs twice: the difference of its two runs is the run-to-run spread the JES figures are
read against.  A single run on a shared machine shows the order of magnitude of a stage, not its third digit.  No hardware counters
are read.  `predicted_share_of_acq_gemm`: the operation count of each of the two JES GEMMs (2 M Np K) over acq_gemm's (M Np^2)."""
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

SCOPES = ("cross_gram", "acq_gemm", "var_gemm", "grad_gemm", "finalize", "mes", "jes_cov", "jes", "jes_agg", "jes_grad", "jes_grad_gemm", "lbfgs")


def timed(ctx, gp, call):
    ctx.prof_reset()
    t0 = time.perf_counter()
    res = call()
    wall = (time.perf_counter() - t0) * 1e3
    st = gp.last_stats()
    row = {"wall_ms": round(wall, 3), "rounds": st["rounds"], "evals_issued": st["evals_issued"], "live_at_end": st["live_at_end"],
           "value": res["value"], "stages": {}}
    for name in SCOPES:
        ms, launches = ctx.prof_get(name)
        if launches:
            row["stages"][name] = {"ms": round(ms, 3), "launches": launches, "ms_per_round": round(ms / st["rounds"], 4)}
    row["device_ms"] = round(sum(v["ms"] for v in row["stages"].values()), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "jes_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--starts", type=int, default=65536)
    ap.add_argument("--n-local", type=int, default=50)
    a = ap.parse_args()
    m = sls()
    N, D, S, n_local = a.N, a.D, a.starts, a.n_local
    rng = np.random.default_rng(N + D)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    b = 0.01
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, b, m.KERNEL_SE)
    starts = np.asfortranarray(rng.uniform(0.0, 1.0, (D, S)))
    mu_best = gp.summary()["mu_best"]
    Np = (N + 127) // 128 * 128
    doc = {"N": N, "D": D, "starts": S, "n_local": n_local, "kernel": "SE", "jes": {}, "mes": {}}
    ctx.prof_enable(True)
    order = np.argsort(y)[::-1]
    for K in (64, 1024):
        xs = np.asfortranarray(np.clip(X[:, order[:K]] + 0.05 * rng.standard_normal((D, K)), 0.0, 1.0))
        fs = np.maximum(y.max() + 0.2 * rng.standard_normal(K), mu_best)
        t0 = time.perf_counter()
        j = gp.jes_create(xs, fs, 1e-8 * theta[0])
        create_ms = (time.perf_counter() - t0) * 1e3
        j.maximize(starts, 2, b, want_all=False)
        row = timed(ctx, gp, lambda: j.maximize(starts, n_local, b, want_all=False))
        row["create_wall_ms"] = round(create_ms, 3)
        row["predicted_share_of_acq_gemm"] = {"jes_cov": round(2 * K / Np, 5), "jes_agg": round(2 * K / Np, 5)}
        st = row["stages"]
        row["measured_share_of_acq_gemm"] = {k: round(st[k]["ms"] / st["acq_gemm"]["ms"], 5) for k in ("jes_cov", "jes", "jes_agg", "jes_grad", "jes_grad_gemm")}
        doc["jes"][f"K={K}"] = row
        j.close()
    ys = np.maximum(y.max() + 0.2 * rng.standard_normal(64), mu_best)
    gp.mes_maximize(ys, starts, 2, want_all=False)
    for rep in ("run1", "run2"):
        doc["mes"][rep] = timed(ctx, gp, lambda: gp.mes_maximize(ys, starts, n_local, want_all=False))
    gp.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
