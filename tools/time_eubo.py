"""Device times of the pair maximiser (sls_eubo_maximize: expected utility of the best option) per profiling scope, beside the EI
maximiser (sls_acq_maximize) on twice as many single-point starts.  Writes one JSON document (default profiles/eubo_timing.json) and
prints it as one line.

    python tools/time_eubo.py [--out FILE] [--N 8192] [--pairs 32768] [--sigma-mode 0]

Shape: N = 8192, D = 64, 32 768 start pairs (2D = 128 variables each) against 65 536 EI starts, 50 evaluations per start: the same
number of cross-covariance columns and of acq_gemm tiles per round.  Times are HIP-event device times of the scopes (sls_prof_get) of
ONE call after a two-round warm-up call of the same shape; `wall_ms` is the host clock around the call.  Per round: the scope's time
over the rounds the call executed (sls_acq_last_stats); the active set shrinks from round to round, so this is an average over the set
sizes of the run.  "eubo" is the two kernels the pair objective adds (pair_diff, eubo_finalize).  No hardware counters are read."""
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

SCOPES = ("cross_gram", "acq_gemm", "var_gemm", "grad_gemm", "finalize", "eubo", "lbfgs")


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
    row["device_ms_per_round"] = round(row["device_ms"] / st["rounds"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "eubo_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=32768)
    ap.add_argument("--n-local", type=int, default=50)
    ap.add_argument("--sigma-mode", type=int, default=0)
    a = ap.parse_args()
    m = sls()
    N, D, S, n_local = a.N, a.D, a.pairs, a.n_local
    rng = np.random.default_rng(N + D)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    gp.set_sigma_mode(a.sigma_mode)
    pairs = np.asfortranarray(rng.uniform(0.0, 1.0, (2 * D, S)))
    starts = np.asfortranarray(pairs.reshape((D, 2 * S), order="F"))      # the same coordinates as 2 S single-point starts
    doc = {"N": N, "D": D, "pairs": S, "ei_starts": 2 * S, "n_local": n_local, "kernel": "SE", "sigma_mode": a.sigma_mode}
    ctx.prof_enable(True)
    gp.eubo_maximize(pairs, 2, want_all=False)
    doc["eubo"] = timed(ctx, gp, lambda: gp.eubo_maximize(pairs, n_local, want_all=False))
    gp.acq_maximize(starts, 2, want_all=False)
    doc["ei"] = timed(ctx, gp, lambda: gp.acq_maximize(starts, n_local, want_all=False))
    st = doc["eubo"]["stages"]
    doc["eubo"]["eubo_share_of_round"] = round(st["eubo"]["ms"] / doc["eubo"]["device_ms"], 5)
    doc["eubo"]["eubo_share_of_acq_gemm"] = round(st["eubo"]["ms"] / st["acq_gemm"]["ms"], 5)
    doc["eubo_over_ei_device_ms_per_round"] = round(doc["eubo"]["device_ms_per_round"] / doc["ei"]["device_ms_per_round"], 4)
    gp.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
