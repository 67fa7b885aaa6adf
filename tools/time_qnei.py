"""Device times of the batch maximiser (sls_qnei_maximize: noisy expected improvement of q points on posterior draws) per profiling
scope, with the baseline from sls_path_max_over_points at the N data points, beside, in the same run, the set maximiser
(sls_qeubo_maximize) on the same starts, the incumbent reduction itself, and the live fraction of both maximisations.  Writes one JSON
document (default profiles/qnei_timing.json) and prints it as one line.

    python tools/time_qnei.py [--out FILE] [--N 8192] [--sets 16384] [--q 4] [--draws 256]

Shape: N = 8192, D = 64, SE, F = 2048, q = 4, 256 draws, 16 384 start sets (65 536 points, qD = 256 variables each), 50 evaluations per
start.  Times are HIP-event device times of the scopes (sls_prof_get) of ONE call after a two-round warm-up call of the same shape;
`wall_ms` is the host clock around the call.  Per round: the scope's time over the rounds the call executed ("lbfgs" is entered once
per round); the active set shrinks from round to round -- for qNEI at once: a start set that no draw improves is stationary and
leaves the batch --, so `live_fraction` = evals_issued / evals_cap is reported beside the times.
The cost per set is taken from the FIRST round, where both objectives have all start sets live: a one-evaluation call (n_local = 1) of
each maximiser, the objective's scopes ("lbfgs" left out) over the number of sets; qEUBO's is measured twice, and the difference of
the two is the spread the qNEI figure is compared with.  "qnei" is the two kernels of the objective (the selection against the
baseline, the finish), "path_max" the column reduction of the incumbents.  No hardware counters are read."""
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

SCOPES = ("cross_gram", "path_prior", "path_data", "path_grad_gemm", "qnei", "qeubo", "qeubo_agg", "qeubo_data_gemm", "path_max", "lbfgs")


def timed(ctx, call):
    ctx.prof_reset()
    t0 = time.perf_counter()
    res = call()
    wall = (time.perf_counter() - t0) * 1e3
    rounds = max(1, ctx.prof_get("lbfgs")[1])
    row = {"wall_ms": round(wall, 3), "rounds": rounds, "stages": {}}
    for name in SCOPES:
        ms, launches = ctx.prof_get(name)
        if launches:
            row["stages"][name] = {"ms": round(ms, 3), "launches": launches, "ms_per_round": round(ms / rounds, 4)}
    row["device_ms"] = round(sum(v["ms"] for v in row["stages"].values()), 3)
    row["device_ms_per_round"] = round(row["device_ms"] / rounds, 4)
    return row, res


def maximise(ctx, gp, call, n_sets, n_local):
    row, res = timed(ctx, call)
    st = gp.last_stats()
    row.update(evals_issued=st["evals_issued"], evals_cap=st["evals_cap"], live_at_end=st["live_at_end"], value=res["value"],
               live_fraction=round(st["evals_issued"] / st["evals_cap"], 5))
    assert st["evals_cap"] == n_sets * n_local
    return row


def first_round(ctx, gp, call, n_sets):
    """One evaluation of every start set through the maximiser: the objective's device time per set."""
    row, _ = timed(ctx, call)
    st = gp.last_stats()
    live = st["evals_issued"]                                    # one evaluation per live set
    ms = sum(v["ms"] for k, v in row["stages"].items() if k != "lbfgs")
    return {"objective_ms": round(ms, 3), "live_sets": live, "us_per_set": round(1e3 * ms / live, 4),
            "stages_ms": {k: v["ms"] for k, v in row["stages"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "qnei_timing.json"))
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
    rng = np.random.default_rng(N + D)                           # tools/time_qeubo.py's problem and start sets
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    sets = np.asfortranarray(rng.uniform(0.0, 1.0, (q * D, S)))
    doc = {"N": N, "D": D, "F": F, "q": q, "draws": a.draws, "sets": S, "points": q * S, "n_local": n_local, "kernel": "SE"}
    ctx.prof_enable(True)
    ps = m.PathSamples(gp, a.draws, F, seed=1)

    # the incumbents: every draw's maximum over the N data points
    ps.max_over_points(X)
    ctx.prof_reset()
    t0 = time.perf_counter()
    t, arg = ps.max_over_points(X)
    wall = (time.perf_counter() - t0) * 1e3
    stages = {k: round(ctx.prof_get(k)[0], 3) for k in SCOPES if ctx.prof_get(k)[1]}
    doc["max_over_points"] = {"points": N, "wall_ms": round(wall, 3), "path_max_ms": stages.get("path_max"),
                              "path_max_launches": ctx.prof_get("path_max")[1], "device_ms": round(sum(stages.values()), 3),
                              "stages": stages, "distinct_incumbent_points": int(np.unique(arg).size)}

    qnei = lambda n, **kw: ps.qnei_maximize(sets, q, n, t, want_all=False, **kw)
    qeubo = lambda n, **kw: ps.qeubo_maximize(sets, q, n, want_all=False, **kw)
    qnei(2)
    qeubo(2)
    # the first round: all sets live under both objectives; qEUBO twice for the spread
    one = {"qeubo_a": first_round(ctx, gp, lambda: qeubo(1), S), "qnei": first_round(ctx, gp, lambda: qnei(1), S),
           "qeubo_b": first_round(ctx, gp, lambda: qeubo(1), S)}
    spread = abs(one["qeubo_a"]["us_per_set"] - one["qeubo_b"]["us_per_set"])
    excess = one["qnei"]["us_per_set"] - max(one["qeubo_a"]["us_per_set"], one["qeubo_b"]["us_per_set"])
    one.update(qeubo_spread_us_per_set=round(spread, 4), qnei_minus_slower_qeubo_us_per_set=round(excess, 4),
               qnei_exceeds_qeubo_by_more_than_the_spread=bool(excess > spread))
    doc["first_round"] = one
    # the whole maximisations
    doc["qnei"] = maximise(ctx, gp, lambda: qnei(n_local), S, n_local)
    doc["qeubo"] = maximise(ctx, gp, lambda: qeubo(n_local), S, n_local)
    improving = ps.qnei_eval(sets, q, t, want_grad=False) > 0.0
    doc["start_sets_with_positive_value"] = int(improving.sum())
    ps.close()
    gp.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
