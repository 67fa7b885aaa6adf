"""Device times of the multi-start maximiser with log expected improvement (acquisition type 2) per profiling scope, beside expected
improvement (type 0) on the same starts in the same run, and the cost of the missing single-launch route at a small shape.  Writes
one JSON document (default profiles/logei_timing.json) and prints it as one line.

    python tools/time_logei.py [--out FILE] [--N 8192] [--starts 65536]

Headline shape: N = 8192, D = 64, 65 536 starts, 50 evaluations per start.  Times are HIP-event device times of the scopes
(sls_prof_get) of ONE call after a two-round warm-up call of the same shape; `wall_ms` is the host clock around the call.  Per round:
the scope's time over the rounds the call executed (sls_acq_last_stats); the active set shrinks from round to round, so this is an
average over the set sizes of the run.  y is the MES timing's (tools/time_mes.py) and, scaled by 60 (`far`), a run in which expected
improvement is exactly 0 at most starts.

Small shape: N = 64, D = 8, acquisition_func::FindNextPointDirect with 100 DIRECT evaluations and 50 local ones through the pybind11
module, host clock around the call (it ends in a synchronisation), median and range of `--small-reps` calls after three warm-up calls,
the two acquisition types alternating.  Expected improvement takes the single-launch paths there (one wavefront per point / start),
LogEI the tiled evaluation and the lock-step rounds.  No hardware counters are read."""
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

SCOPES = ("cross_gram", "acq_gemm", "var_gemm", "grad_gemm", "finalize", "logei", "lbfgs", "acq_wave")


def timed(ctx, gp, call):
    ctx.prof_reset()
    t0 = time.perf_counter()
    res = call()
    wall = (time.perf_counter() - t0) * 1e3
    st = gp.last_stats()
    row = {"wall_ms": round(wall, 3), "rounds": st["rounds"], "evals_issued": st["evals_issued"], "evals_cap": st["evals_cap"],
           "live_at_end": st["live_at_end"], "value": res["value"], "stages": {}}
    for name in SCOPES:
        ms, launches = ctx.prof_get(name)
        if launches:
            row["stages"][name] = {"ms": round(ms, 3), "launches": launches, "ms_per_round": round(ms / st["rounds"], 4)}
    row["device_ms"] = round(sum(v["ms"] for v in row["stages"].values()), 3)
    return row


def headline(m, a):
    N, D, S, n_local = a.N, a.D, a.starts, a.n_local
    rng = np.random.default_rng(N + D)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    starts = np.asfortranarray(rng.uniform(0.0, 1.0, (D, S)))
    doc = {"N": N, "D": D, "starts": S, "n_local": n_local, "kernel": "SE"}
    ctx = m.Context(0)
    for label, scale in (("as_mes_timing", 1.0), ("far", 60.0)):
        gp = m.GP(ctx, X, scale * y, theta, 0.01, m.KERNEL_SE)
        ei0, dei0 = gp.acq_eval(starts[:, :4096], m.ACQ_EI)
        row = {"y_scale": scale, "ei_exactly_zero_with_zero_gradient_among_first_4096_starts": int(((ei0 == 0) & np.all(dei0 == 0, axis=0)).sum())}
        ctx.prof_enable(True)
        for name, acq in (("logei", m.ACQ_LOG_EI), ("ei", m.ACQ_EI)):
            gp.acq_maximize(starts, 2, acq, want_all=False)
            row[name] = timed(ctx, gp, lambda: gp.acq_maximize(starts, n_local, acq, want_all=False))
        ctx.prof_enable(False)
        st = row["logei"]["stages"]
        row["logei_share_of_acq_gemm"] = round(st["logei"]["ms"] / st["acq_gemm"]["ms"], 6)
        doc[label] = row
        gp.close()
    ctx.close()
    return doc


def small(m, a):
    sys.path.insert(0, os.path.join(R, "sequential-line-search_amd"))
    import pySequentialLineSearch as pysls
    N, D = 64, 8
    rng = np.random.default_rng(N + D)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    kinds = {"ei": pysls.AcquisitionFuncType.ExpectedImprovement, "logei": pysls.AcquisitionFuncType.LogExpectedImprovement}
    ms = {k: [] for k in kinds}
    value = {}
    for rep in range(3 + a.small_reps):
        for name, kind in kinds.items():
            t0 = time.perf_counter()
            _, value[name] = pysls.find_next_point_direct(reg, 100, 50, kind, 1.0)
            if rep >= 3:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    doc = {"N": N, "D": D, "num_global_search_iters": 100, "num_local_search_iters": 50, "calls": a.small_reps}
    for name in kinds:
        doc[name] = {"wall_ms_median": round(float(np.median(ms[name])), 3), "wall_ms_min": round(min(ms[name]), 3),
                     "wall_ms_max": round(max(ms[name]), 3), "value": value[name]}
    doc["logei_over_ei"] = round(doc["logei"]["wall_ms_median"] / doc["ei"]["wall_ms_median"], 3)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "logei_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--starts", type=int, default=65536)
    ap.add_argument("--n-local", type=int, default=50)
    ap.add_argument("--small-reps", type=int, default=20)
    a = ap.parse_args()
    m = sls()
    doc = {"headline": headline(m, a), "find_next_point_direct": small(m, a)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
