"""Device times of the gallery maximiser (sls_patch_maximize: expected utility of the best cell of a qs x qt grid on a bilinear patch)
per profiling scope, free and anchored, beside, in the same run, the set maximiser (sls_qeubo_maximize) on the same points -- the
start patches expanded into their qs qt cells -- and the slider maximiser (sls_line_maximize) with as many positions, and the live
fraction of every maximisation.  Writes one JSON document (default profiles/patch_timing.json) and prints it as one line.

    python tools/time_patch.py [--out FILE] [--N 8192] [--patches 16384] [--grid 4 4] [--draws 256]

Shape: N = 8192, D = 64, SE, F = 2048, 256 draws, 16 384 start patches, a 4 x 4 grid (262 144 points per round; the maximiser runs
over 4D = 256 variables, 3D = 192 anchored at the best data point, where the set maximiser runs over 16 D = 1024 and the slider's
over 2D = 128 / D = 64), 50 evaluations per start.  Times are HIP-event device times of the scopes (sls_prof_get) of ONE call after a
two-round warm-up call of the same shape; `wall_ms` is the host clock around the call.
The cost per point is taken from the FIRST round, where every start is live under every objective: a one-evaluation call
(n_local = 1) of each maximiser, the objective's scopes ("lbfgs" left out) over the number of points; qEUBO's is measured twice, and
the difference of the two is the spread the other figures are compared with.  "patch" is the two kernels the patch objective adds
(patch_expand, patch_fold), "line" the slider's two; `share` is their part of the round's objective time.  The two patch kernels move
the same q D doubles per item as the line's and read four corners where those read two, so `bound` records whether the patch
scope's share stays within twice the line scope's share of this run.  No hardware counters are read."""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import patch_ref  # noqa: E402
from util import sls  # noqa: E402

SCOPES = ("cross_gram", "path_prior", "path_data", "path_grad_gemm", "patch", "line", "qeubo", "qeubo_agg", "qeubo_data_gemm", "lbfgs")


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


def first_round(ctx, gp, call, q, scope):
    """One evaluation of every start through the maximiser: the objective's device time per point, and the part of `scope` in it."""
    row, _ = timed(ctx, call)
    live = gp.last_stats()["evals_issued"]                       # one evaluation per live start
    ms = sum(v["ms"] for k, v in row["stages"].items() if k != "lbfgs")
    own = row["stages"].get(scope, {})
    return {"objective_ms": round(ms, 3), "live_starts": live, "us_per_point": round(1e3 * ms / (live * q), 5), "scope": scope,
            "scope_ms": own.get("ms", 0.0), "scope_launches": own.get("launches", 0), "share": round(own.get("ms", 0.0) / ms, 5),
            "stages_ms": {k: v["ms"] for k, v in row["stages"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "patch_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--grid", type=int, nargs=2, default=[4, 4])
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--patches", type=int, default=16384)
    ap.add_argument("--n-local", type=int, default=50)
    a = ap.parse_args()
    m = sls()
    N, D, F, S, n_local = a.N, a.D, a.F, a.patches, a.n_local
    (qs, qt), q = a.grid, a.grid[0] * a.grid[1]
    rng = np.random.default_rng(N + D)                           # tools/time_qeubo.py's problem
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    patches = np.asfortranarray(rng.uniform(0.0, 1.0, (4 * D, S)))
    anchor = X[:, int(np.argmax(y))].copy()
    doc = {"N": N, "D": D, "F": F, "draws": a.draws, "patches": S, "grid": [qs, qt], "n_local": n_local, "kernel": "SE",
           "points": q * S, "variables": {"patch_free": 4 * D, "patch_anchored": 3 * D, "qeubo": q * D, "line_free": 2 * D,
                                          "line_anchored": D}}
    ctx.prof_enable(True)
    ps = m.PathSamples(gp, a.draws, F, seed=1)
    free = lambda n: ps.patch_maximize(patches, qs, qt, n, want_all=False)
    anch = lambda n: ps.patch_maximize(patches[D:], qs, qt, n, anchor=anchor, want_all=False)
    sets = np.asfortranarray(patch_ref.expand(patches, qs, qt, D))
    qeubo = lambda n: ps.qeubo_maximize(sets, q, n, want_all=False)
    # the slider with as many positions, from the patches' first two corners
    line = lambda n: ps.line_maximize(patches[:2 * D], q, n, want_all=False)
    line_anch = lambda n: ps.line_maximize(patches[D:2 * D], q, n, anchor=anchor, want_all=False)
    for f in (free, anch, qeubo, line):
        f(2)
    # the first round: every start live under every objective, q S points each; qEUBO twice for the spread
    one = {"qeubo_a": first_round(ctx, gp, lambda: qeubo(1), q, "qeubo"), "patch_free": first_round(ctx, gp, lambda: free(1), q, "patch"),
           "line_free": first_round(ctx, gp, lambda: line(1), q, "line"),
           "patch_anchored": first_round(ctx, gp, lambda: anch(1), q, "patch"),
           "line_anchored": first_round(ctx, gp, lambda: line_anch(1), q, "line"),
           "qeubo_b": first_round(ctx, gp, lambda: qeubo(1), q, "qeubo")}
    spread = abs(one["qeubo_a"]["us_per_point"] - one["qeubo_b"]["us_per_point"])
    slower = max(one["qeubo_a"]["us_per_point"], one["qeubo_b"]["us_per_point"])
    one.update(qeubo_spread_us_per_point=round(spread, 5),
               patch_free_minus_slower_qeubo_us_per_point=round(one["patch_free"]["us_per_point"] - slower, 5),
               patch_free_minus_line_free_us_per_point=round(one["patch_free"]["us_per_point"] - one["line_free"]["us_per_point"], 5))
    doc["first_round"] = one
    doc["bound"] = {form: {"patch_share": one[f"patch_{form}"]["share"], "line_share": one[f"line_{form}"]["share"],
                           "ratio": round(one[f"patch_{form}"]["share"] / one[f"line_{form}"]["share"], 4),
                           "within_twice_the_line_share": bool(one[f"patch_{form}"]["share"] <= 2.0 * one[f"line_{form}"]["share"])}
                    for form in ("free", "anchored")}
    # the whole maximisations
    doc["patch_free"] = maximise(ctx, gp, lambda: free(n_local), S, n_local)
    doc["patch_anchored"] = maximise(ctx, gp, lambda: anch(n_local), S, n_local)
    doc["qeubo"] = maximise(ctx, gp, lambda: qeubo(n_local), S, n_local)
    doc["line_free"] = maximise(ctx, gp, lambda: line(n_local), S, n_local)
    doc["line_anchored"] = maximise(ctx, gp, lambda: line_anch(n_local), S, n_local)
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
