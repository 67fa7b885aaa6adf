"""Device times of the information-gain maximiser (sls_qbald_maximize: the mutual information between the answer to a q-option choice
query and the latent function, on posterior draws) per profiling scope at two BTL scales, beside, in the same run,
sls_qlognei_maximize on the same start sets -- whose selection is the yardstick: the same geometry, about eight transcendentals per
value against this criterion's three.  Writes one JSON document (default profiles/qbald_timing.json) and prints it as one line.

    python tools/time_qbald.py [--out FILE] [--N 8192] [--sets 16384] [--q 4] [--draws 256] [--scale 0.05] [--scale2 0.01]

Shape: tools/time_qlognei.py's (N = 8192, D = 64, SE, F = 2048, q = 4, 256 draws, 16 384 start sets, 50 evaluations per start).  Times
are HIP-event device times of the scopes (sls_prof_get) of ONE call after a two-round warm-up call of the same shape; `wall_ms` is the
host clock around the call.  The cost per set is taken from the FIRST round (a one-evaluation call: every start set is live).  "qbald"
is the two selection stages and the finish (three kernels per pass), "qlognei" the same of the log form, "qeubo_agg" the two
aggregation GEMMs the selection feeds.  The live fraction is evaluations issued over the cap of sets x evaluations: at a small scale
saturated start sets (one-hot choice probabilities, zero weights) are stationary and leave at once.  No hardware counters are read."""
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

SCOPES = ("cross_gram", "path_prior", "path_data", "path_grad_gemm", "qbald", "qlognei", "qeubo_agg", "qeubo_data_gemm", "lbfgs")


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
    return row


def first_round(ctx, gp, call):
    """One evaluation of every start set through the maximiser: the objective's device time per set."""
    row, _ = timed(ctx, call)
    live = gp.last_stats()["evals_issued"]
    ms = sum(v["ms"] for k, v in row["stages"].items() if k != "lbfgs")
    return {"objective_ms": round(ms, 3), "live_sets": live, "us_per_set": round(1e3 * ms / live, 4),
            "stages_ms": {k: v["ms"] for k, v in row["stages"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "qbald_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--q", type=int, default=4)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--sets", type=int, default=16384)
    ap.add_argument("--n-local", type=int, default=50)
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--scale2", type=float, default=0.01)
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
           "scales": [a.scale, a.scale2], "tau_relu": m.QLOGNEI_TAU_RELU, "tau_max": m.QLOGNEI_TAU_MAX}
    ctx.prof_enable(True)
    ps = m.PathSamples(gp, a.draws, F, seed=1)
    t = ps.max_over_points(X)[0]

    qlog = lambda n, **kw: ps.qlognei_maximize(sets, q, n, t, **kw)
    bald = lambda tau: (lambda n, **kw: ps.qbald_maximize(sets, q, n, tau, **kw))
    qlog(2, want_all=False)
    one = {"qlognei": first_round(ctx, gp, lambda: qlog(1, want_all=False))}
    doc["qlognei"] = maximise(ctx, gp, lambda: qlog(n_local, want_all=False), S, n_local)
    for tau in (a.scale, a.scale2):
        key = f"qbald_scale_{tau:g}"
        bald(tau)(2, want_all=False)
        one[key] = first_round(ctx, gp, lambda: bald(tau)(1, want_all=False))
        doc[key] = maximise(ctx, gp, lambda: bald(tau)(n_local, want_all=False), S, n_local)
        val = ps.qbald_eval(sets, q, tau, want_grad=False)
        doc[key]["value_at_the_starts"] = {"min": float(val.min()), "median": float(np.median(val)), "max": float(val.max())}
    first = one[f"qbald_scale_{a.scale:g}"]["stages_ms"]
    one.update(qbald_scope_ms=first["qbald"], qlognei_scope_ms=one["qlognei"]["stages_ms"]["qlognei"],
               qeubo_agg_ms_under_qbald=first["qeubo_agg"], qeubo_agg_ms_under_qlognei=one["qlognei"]["stages_ms"]["qeubo_agg"])
    doc["first_round"] = one
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
