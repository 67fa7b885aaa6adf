"""Device times of the log-space batch maximiser (sls_qlognei_maximize: log-space noisy expected improvement of q points on posterior
draws, default temperatures) per profiling scope, beside, in the same run, sls_qnei_maximize on the same starts and baseline, the
live fraction of both maximisations, and what the log form is for: how many of the start sets whose qNEI is exactly 0 -- which
sls_qnei_maximize returns unmoved -- end at a set with positive qNEI.  Writes one JSON document (default
profiles/qlognei_timing.json) and prints it as one line.

    python tools/time_qlognei.py [--out FILE] [--N 8192] [--sets 16384] [--q 4] [--draws 256] [--gap 0.0]

Shape: tools/time_qnei.py's (N = 8192, D = 64, SE, F = 2048, q = 4, 256 draws, 16 384 start sets, 50 evaluations per start), the
baseline from sls_path_max_over_points at the data plus --gap (a tighter incumbent: more start sets that no draw improves).  Times are
HIP-event device times of the scopes (sls_prof_get) of ONE call after a two-round warm-up call of the same shape; `wall_ms` is the
host clock around the call.  The cost per set is taken from the FIRST round (a one-evaluation call, every start set live under the
log form; under qNEI as many as the maximiser issues).  "qlognei" is the two selection stages and the finish (three kernels per
pass), "qnei" the selection and the finish of qNEI (two), "qeubo_agg" the two aggregation GEMMs the selection feeds.  No hardware
counters are read."""
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

SCOPES = ("cross_gram", "path_prior", "path_data", "path_grad_gemm", "qlognei", "qnei", "qeubo_agg", "qeubo_data_gemm", "lbfgs")


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
    return row, res


def maximise(ctx, gp, call, n_sets, n_local):
    row, res = timed(ctx, call)
    st = gp.last_stats()
    row.update(evals_issued=st["evals_issued"], evals_cap=st["evals_cap"], live_at_end=st["live_at_end"], value=res["value"],
               live_fraction=round(st["evals_issued"] / st["evals_cap"], 5))
    assert st["evals_cap"] == n_sets * n_local
    return row, res


def first_round(ctx, gp, call):
    """One evaluation of every start set through the maximiser: the objective's device time per set."""
    row, _ = timed(ctx, call)
    live = gp.last_stats()["evals_issued"]
    ms = sum(v["ms"] for k, v in row["stages"].items() if k != "lbfgs")
    return {"objective_ms": round(ms, 3), "live_sets": live, "us_per_set": round(1e3 * ms / live, 4),
            "stages_ms": {k: v["ms"] for k, v in row["stages"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "qlognei_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--q", type=int, default=4)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--sets", type=int, default=16384)
    ap.add_argument("--n-local", type=int, default=50)
    ap.add_argument("--gap", type=float, default=0.0)
    a = ap.parse_args()
    m = sls()
    N, D, F, q, S, n_local = a.N, a.D, a.F, a.q, a.sets, a.n_local
    rng = np.random.default_rng(N + D)                           # tools/time_qnei.py's problem and start sets
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    sets = np.asfortranarray(rng.uniform(0.0, 1.0, (q * D, S)))
    doc = {"N": N, "D": D, "F": F, "q": q, "draws": a.draws, "sets": S, "points": q * S, "n_local": n_local, "kernel": "SE",
           "tau_relu": m.QLOGNEI_TAU_RELU, "tau_max": m.QLOGNEI_TAU_MAX, "baseline_gap": a.gap}
    ctx.prof_enable(True)
    ps = m.PathSamples(gp, a.draws, F, seed=1)
    t = ps.max_over_points(X)[0] + a.gap

    qlog = lambda n, **kw: ps.qlognei_maximize(sets, q, n, t, **kw)
    qnei = lambda n, **kw: ps.qnei_maximize(sets, q, n, t, **kw)
    qlog(2, want_all=False)
    qnei(2, want_all=False)
    one = {"qlognei": first_round(ctx, gp, lambda: qlog(1, want_all=False)), "qnei": first_round(ctx, gp, lambda: qnei(1, want_all=False))}
    sel, agg = one["qlognei"]["stages_ms"]["qlognei"], one["qlognei"]["stages_ms"]["qeubo_agg"]
    one.update(qlognei_scope_ms=sel, qnei_scope_ms=one["qnei"]["stages_ms"]["qnei"], qeubo_agg_ms=agg,
               selection_costs_more_than_the_aggregation=bool(sel > agg))
    doc["first_round"] = one
    doc["qlognei"], rl = maximise(ctx, gp, lambda: qlog(n_local), S, n_local)
    doc["qnei"], rn = maximise(ctx, gp, lambda: qnei(n_local), S, n_local)
    at_start = ps.qnei_eval(sets, q, t, want_grad=False)
    dead = at_start == 0.0
    unmoved = np.all(rn["x_stars"][:, dead] == sets[:, dead], axis=0)
    after = ps.qnei_eval(rl["x_stars"], q, t, want_grad=False)
    doc["escape"] = {"start_sets_with_qnei_zero": int(dead.sum()), "returned_unmoved_by_qnei_maximize": int(unmoved.sum()),
                     "of_those_with_positive_qnei_after_qlognei_maximize": int((after[dead] > 0.0).sum()),
                     "best_qnei_of_qnei_maximize": float(rn["y_stars"].max()),
                     "best_qnei_at_the_ends_of_qlognei_maximize": float(after.max()),
                     "qnei_at_the_winner_of_qlognei_maximize": float(after[rl["index"]])}
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
