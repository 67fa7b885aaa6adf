"""Device times of the max-value entropy search maximiser (sls_mes_maximize) per profiling scope, beside the EI maximiser
(sls_acq_maximize) on the same starts.  Writes one JSON document (default profiles/mes_timing.json) and prints it as one line.

    python tools/time_mes.py [--out FILE] [--N 8192] [--starts 65536]

Shape: N = 8192, D = 64, 65 536 starts, 50 evaluations per start, K = 64 and K = 4096 samples of the maximum value (drawn around
max(y) and clamped at mu_best: the combiner's cost does not depend on where they lie).  Times are HIP-event device times of the scopes
(sls_prof_get) of ONE call after a two-round warm-up call of the same shape; `wall_ms` is the host clock around the call.  Per round:
the scope's time over the rounds the call executed (sls_acq_last_stats); the active set shrinks from round to round, so this is an
average over the set sizes of the run.  No hardware counters are read."""
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

SCOPES = ("cross_gram", "acq_gemm", "var_gemm", "grad_gemm", "finalize", "mes", "lbfgs")


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
    ap.add_argument("--out", default=os.path.join(R, "profiles", "mes_timing.json"))
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
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    starts = np.asfortranarray(rng.uniform(0.0, 1.0, (D, S)))
    mu_best = gp.summary()["mu_best"]
    doc = {"N": N, "D": D, "starts": S, "n_local": n_local, "kernel": "SE", "mes": {}}
    ctx.prof_enable(True)
    for K in (64, 4096):
        ys = np.maximum(y.max() + 0.2 * rng.standard_normal(K), mu_best)
        gp.mes_maximize(ys, starts, 2, want_all=False)
        doc["mes"][f"K={K}"] = timed(ctx, gp, lambda: gp.mes_maximize(ys, starts, n_local, want_all=False))
    gp.acq_maximize(starts, 2, want_all=False)
    doc["ei"] = timed(ctx, gp, lambda: gp.acq_maximize(starts, n_local, want_all=False))
    for K in ("K=64", "K=4096"):
        st = doc["mes"][K]["stages"]
        doc["mes"][K]["mes_share_of_acq_gemm"] = round(st["mes"]["ms"] / st["acq_gemm"]["ms"], 5)
    gp.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
