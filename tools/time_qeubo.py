"""Device times of the set maximiser (sls_qeubo_maximize: expected utility of the best of q options on posterior draws) per profiling
scope, beside, in the same run, the EI maximiser (sls_acq_maximize) on as many single-point starts as the sets have points, and the
per-draw path maximiser (sls_path_maximize) on 64 draws x 1024 starts.  Writes one JSON document (default
profiles/qeubo_timing.json) and prints it as one line.

    python tools/time_qeubo.py [--out FILE] [--N 8192] [--sets 16384] [--q 4] [--draws 256]

Shape: N = 8192, D = 64, SE, F = 2048, q = 4, 256 draws, 16 384 start sets (65 536 points, qD = 256 variables each), 50 evaluations per
start.  Times are HIP-event device times of the scopes (sls_prof_get) of ONE call after a two-round warm-up call of the same shape;
`wall_ms` is the host clock around the call.  Per round: the scope's time over the rounds the call executed ("lbfgs" is entered once
per round); the active set shrinks from round to round, so this is an average over the set sizes of the run.  "qeubo" is the two
kernels the set objective adds (qeubo_select, qeubo_finish), "qeubo_agg" its two aggregation GEMMs, "qeubo_data_gemm" the K* V GEMM of
the every-draw values ("path_data" is then the gathered data pass on the aggregated weights plus path_grad).  No hardware counters are read."""
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

SCOPES = ("cross_gram", "path_prior", "path_data", "path_grad_gemm", "qeubo", "qeubo_agg", "qeubo_data_gemm", "acq_gemm", "var_gemm", "grad_gemm", "finalize",
          "lbfgs")


def timed(ctx, call):
    ctx.prof_reset()
    t0 = time.perf_counter()
    res = call()
    wall = (time.perf_counter() - t0) * 1e3
    rounds = ctx.prof_get("lbfgs")[1]
    row = {"wall_ms": round(wall, 3), "rounds": rounds, "stages": {}}
    for name in SCOPES:
        ms, launches = ctx.prof_get(name)
        if launches:
            row["stages"][name] = {"ms": round(ms, 3), "launches": launches, "ms_per_round": round(ms / rounds, 4)}
    row["device_ms"] = round(sum(v["ms"] for v in row["stages"].values()), 3)
    row["device_ms_per_round"] = round(row["device_ms"] / rounds, 4)
    return row, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "qeubo_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--q", type=int, default=4)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--sets", type=int, default=16384)
    ap.add_argument("--n-local", type=int, default=50)
    a = ap.parse_args()
    m = sls()
    N, D, F, q, S, n_local = a.N, a.D, a.F, a.q, a.sets, a.n_local
    rng = np.random.default_rng(N + D)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    sets = np.asfortranarray(rng.uniform(0.0, 1.0, (q * D, S)))
    starts = np.asfortranarray(sets.reshape((D, q * S), order="F"))      # the same coordinates as q S single-point starts
    doc = {"N": N, "D": D, "F": F, "q": q, "draws": a.draws, "sets": S, "points": q * S, "n_local": n_local, "kernel": "SE"}
    ctx.prof_enable(True)

    ps = m.PathSamples(gp, a.draws, F, seed=1)
    ps.qeubo_maximize(sets, q, 2, want_all=False)
    row, res = timed(ctx, lambda: ps.qeubo_maximize(sets, q, n_local, want_all=False))
    st = gp.last_stats()
    row.update(evals_issued=st["evals_issued"], live_at_end=st["live_at_end"], value=res["value"])
    new = sum(row["stages"][k]["ms"] for k in ("qeubo", "qeubo_agg"))   # the share the issue asks for; the data GEMM is reported beside it
    row["qeubo_plus_agg_share_of_round"] = round(new / row["device_ms"], 5)
    row["dominant_stage"] = max(row["stages"], key=lambda k: row["stages"][k]["ms"])
    doc["qeubo"] = row
    # one evaluation pass of all sets on its own (value, gradient, win counts), host transfers included in the wall time only
    ctx.prof_reset()
    t0 = time.perf_counter()
    ps.qeubo_eval(sets, q, want_wins=True)
    doc["qeubo_eval"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                         "stages": {k: round(ctx.prof_get(k)[0], 3) for k in SCOPES if ctx.prof_get(k)[1]}}
    # the every-draw values of the same points through sls_path_eval, whose data term is the per-(point, draw) gathered dot
    # (path_data_kernel) where the set objective uses a tile GEMM: ONE pass, to compare with one round's "path_data" above
    ctx.prof_reset()
    ps.eval_all(starts)
    doc["path_eval_all_same_points"] = {"stages": {k: round(ctx.prof_get(k)[0], 3) for k in SCOPES if ctx.prof_get(k)[1]}}
    ps.close()

    gp.acq_maximize(starts, 2, want_all=False)
    row, res = timed(ctx, lambda: gp.acq_maximize(starts, n_local, want_all=False))
    st = gp.last_stats()
    row.update(evals_issued=st["evals_issued"], live_at_end=st["live_at_end"], value=res["value"])
    doc["ei"] = row

    pd, ps_starts = 64, 1024
    ps = m.PathSamples(gp, pd, F, seed=1)
    tstarts = np.asfortranarray(starts[:, :pd * ps_starts])
    ps.maximize(tstarts, 2)
    row, _ = timed(ctx, lambda: ps.maximize(tstarts, n_local))
    row.update(draws=pd, starts_per_draw=ps_starts)
    doc["path_maximize"] = row
    ps.close()

    doc["qeubo_over_ei_device_ms_per_round"] = round(doc["qeubo"]["device_ms_per_round"] / doc["ei"]["device_ms_per_round"], 4)
    doc["qeubo_over_path_device_ms_per_round"] = round(doc["qeubo"]["device_ms_per_round"] / doc["path_maximize"]["device_ms_per_round"], 4)
    gp.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
