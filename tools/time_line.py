"""Device times of the slider maximiser (sls_line_maximize: expected utility of the best of q grid positions on a line) per
profiling scope, free and anchored, beside, in the same run, the set maximiser (sls_qeubo_maximize) on the same points -- the start
lines expanded into their q positions -- and the live fraction of every maximisation.  Writes one JSON document (default
profiles/line_timing.json) and prints it as one line.

    python tools/time_line.py [--out FILE] [--N 8192] [--lines 16384] [--q 4 16] [--draws 256]

Shape: N = 8192, D = 64, SE, F = 2048, 256 draws, 16 384 start lines, q = 4 and q = 16 (65 536 and 262 144 points per round; the
maximiser runs over 2D = 128 variables, D = 64 anchored at the best data point, where the set maximiser runs over qD = 256 / 1024),
50 evaluations per start.  Times are HIP-event device times of the scopes (sls_prof_get) of ONE call after a two-round warm-up call of
the same shape; `wall_ms` is the host clock around the call.
The cost per point is taken from the FIRST round, where every start is live under every objective: a one-evaluation call
(n_local = 1) of each maximiser, the objective's scopes ("lbfgs" left out) over the number of points; qEUBO's is measured twice, and
the difference of the two is the spread the line figures are compared with.  "line" is the two kernels the line objective adds
(line_expand, line_fold); `line_share` is its part of the round's objective time.  No hardware counters are read."""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import line_ref  # noqa: E402
from util import sls  # noqa: E402

SCOPES = ("cross_gram", "path_prior", "path_data", "path_grad_gemm", "line", "qeubo", "qeubo_agg", "qeubo_data_gemm", "lbfgs")


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


def maximise(ctx, gp, call, n_starts, n_local):
    row, res = timed(ctx, call)
    st = gp.last_stats()
    row.update(evals_issued=st["evals_issued"], evals_cap=st["evals_cap"], live_at_end=st["live_at_end"], value=res["value"],
               live_fraction=round(st["evals_issued"] / st["evals_cap"], 5))
    assert st["evals_cap"] == n_starts * n_local
    return row


def first_round(ctx, gp, call, q):
    """One evaluation of every start through the maximiser: the objective's device time per point."""
    row, _ = timed(ctx, call)
    live = gp.last_stats()["evals_issued"]                       # one evaluation per live start
    ms = sum(v["ms"] for k, v in row["stages"].items() if k != "lbfgs")
    line_ms = row["stages"].get("line", {}).get("ms", 0.0)
    return {"objective_ms": round(ms, 3), "live_starts": live, "us_per_point": round(1e3 * ms / (live * q), 5),
            "line_ms": line_ms, "line_share": round(line_ms / ms, 5), "stages_ms": {k: v["ms"] for k, v in row["stages"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "line_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--q", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--lines", type=int, default=16384)
    ap.add_argument("--n-local", type=int, default=50)
    a = ap.parse_args()
    m = sls()
    N, D, F, S, n_local = a.N, a.D, a.F, a.lines, a.n_local
    rng = np.random.default_rng(N + D)                           # tools/time_qeubo.py's problem
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    lines = np.asfortranarray(rng.uniform(0.0, 1.0, (2 * D, S)))
    anchor = X[:, int(np.argmax(y))].copy()
    doc = {"N": N, "D": D, "F": F, "draws": a.draws, "lines": S, "n_local": n_local, "kernel": "SE", "by_q": {}}
    ctx.prof_enable(True)
    ps = m.PathSamples(gp, a.draws, F, seed=1)
    for q in a.q:
        free = lambda n: ps.line_maximize(lines, q, n, want_all=False)
        anch = lambda n: ps.line_maximize(lines[D:], q, n, anchor=anchor, want_all=False)
        sets_free = np.asfortranarray(line_ref.expand(lines, q, D))
        sets_anch = np.asfortranarray(line_ref.expand(lines[D:], q, D, anchor))
        qe_free = lambda n: ps.qeubo_maximize(sets_free, q, n, want_all=False)
        qe_anch = lambda n: ps.qeubo_maximize(sets_anch, q, n, want_all=False)
        for f in (free, anch, qe_free):
            f(2)
        # the first round: every start live under every objective, the same q S points; qEUBO twice for the spread
        one = {"qeubo_a": first_round(ctx, gp, lambda: qe_free(1), q), "line_free": first_round(ctx, gp, lambda: free(1), q),
               "qeubo_anchored_points": first_round(ctx, gp, lambda: qe_anch(1), q),
               "line_anchored": first_round(ctx, gp, lambda: anch(1), q), "qeubo_b": first_round(ctx, gp, lambda: qe_free(1), q)}
        spread = abs(one["qeubo_a"]["us_per_point"] - one["qeubo_b"]["us_per_point"])
        slower = max(one["qeubo_a"]["us_per_point"], one["qeubo_b"]["us_per_point"])
        one.update(qeubo_spread_us_per_point=round(spread, 5),
                   line_free_minus_slower_qeubo_us_per_point=round(one["line_free"]["us_per_point"] - slower, 5),
                   line_anchored_minus_qeubo_at_its_points_us_per_point=round(
                       one["line_anchored"]["us_per_point"] - one["qeubo_anchored_points"]["us_per_point"], 5))
        row = {"points": q * S, "variables": {"line_free": 2 * D, "line_anchored": D, "qeubo": q * D}, "first_round": one}
        # the whole maximisations
        row["line_free"] = maximise(ctx, gp, lambda: free(n_local), S, n_local)
        row["line_anchored"] = maximise(ctx, gp, lambda: anch(n_local), S, n_local)
        row["qeubo"] = maximise(ctx, gp, lambda: qe_free(n_local), S, n_local)
        doc["by_q"][str(q)] = row
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
