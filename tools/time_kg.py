"""Device times of the knowledge-gradient maximiser (sls_kg_maximize) per profiling scope, beside the joint entropy search maximiser
(sls_jes_maximize) and the max-value entropy search maximiser (sls_mes_maximize) on the same starts in the same process.  Writes one
JSON document (default profiles/kg_timing.json) and prints it as one line.

    python tools/time_kg.py [--out FILE] [--N 8192] [--starts 65536] [--n-local 50]

Shape: N = 8192, D = 64, SE kernel, 65 536 starts, 50 evaluations per start, K = 64 and K = 1024 fixed points (the data points of
highest y, the host layer's default set; JES conditions on optima near the same points), the candidate's own line included.  Times are
HIP-event device times of the scopes (sls_prof_get) of ONE call after a two-round warm-up call of the same shape; `wall_ms` is the host
clock around the call.  Per round: the scope's time over the rounds the call executed (sls_acq_last_stats); the active set shrinks
from round to round, so this is an average over the set sizes of the run.  A single run on a shared machine shows the order of
magnitude of a stage, not its third digit.  No hardware counters are read.  The knowledge gradient shares the stages "jes_cov",
"jes_agg", "jes_grad" and "jes_grad_gemm" with joint entropy search; its own combiner and finish count under "kg", JES's under "jes"."""
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

SCOPES = ("cross_gram", "acq_gemm", "var_gemm", "grad_gemm", "finalize", "mes", "jes_cov", "jes", "kg", "jes_agg", "jes_grad",
          "jes_grad_gemm", "lbfgs")


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
    ap.add_argument("--out", default=os.path.join(R, "profiles", "kg_timing.json"))
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
    doc = {"N": N, "D": D, "starts": S, "n_local": n_local, "kernel": "SE", "kg": {}, "jes": {}, "mes": {}}
    ctx.prof_enable(True)
    order = np.argsort(y)[::-1]
    for K in (64, 1024):
        keep = np.sort(order[:K])
        t0 = time.perf_counter()
        kg = gp.kg_create(X[:, keep])
        create_ms = (time.perf_counter() - t0) * 1e3
        kg.maximize(starts, 2, b, want_all=False)
        row = timed(ctx, gp, lambda: kg.maximize(starts, n_local, b, want_all=False))
        row["create_wall_ms"] = round(create_ms, 3)
        kg.close()
        xs = np.asfortranarray(np.clip(X[:, order[:K]] + 0.05 * rng.standard_normal((D, K)), 0.0, 1.0))
        fs = np.maximum(y.max() + 0.2 * rng.standard_normal(K), mu_best)
        j = gp.jes_create(xs, fs, 1e-8 * theta[0])
        j.maximize(starts, 2, b, want_all=False)
        jrow = timed(ctx, gp, lambda: j.maximize(starts, n_local, b, want_all=False))
        j.close()
        st, js = row["stages"], jrow["stages"]
        row["kg_over_jes_combiner"] = round(st["kg"]["ms_per_round"] / js["jes"]["ms_per_round"], 4)
        row["kg_over_cov_plus_agg"] = round(st["kg"]["ms_per_round"] / (st["jes_cov"]["ms_per_round"] + st["jes_agg"]["ms_per_round"]), 4)
        row["wall_over_jes"] = round(row["wall_ms"] / jrow["wall_ms"], 4)
        doc["kg"][f"K={K}"] = row
        doc["jes"][f"K={K}"] = jrow
    ys = np.maximum(y.max() + 0.2 * rng.standard_normal(64), mu_best)
    gp.mes_maximize(ys, starts, 2, want_all=False)
    doc["mes"]["run1"] = timed(ctx, gp, lambda: gp.mes_maximize(ys, starts, n_local, want_all=False))
    gp.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
