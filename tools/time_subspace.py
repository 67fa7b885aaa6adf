"""Device times of the subspace maximiser (sls_acq_maximize_sub: x = c + A z, two kernels around the unchanged evaluation) per
profiling scope, beside, in the same run, the plain maximiser (sls_acq_maximize) on the same starts.  Writes one JSON document
(default profiles/subspace_timing.json) and prints it as one line.

    python tools/time_subspace.py [--out FILE] [--N 8192] [--starts 65536] [--n-local 50] [--repeat 3]

Shape: N = 8192, D = 64, Matern 5/2, expected improvement, 65 536 starts, 50 evaluations per start.  Legs:
  plain       sls_acq_maximize over [0,1]^64
  identity    the identity box (d = D, A = I, c = 0): the same search through the two kernels -- same rounds, same live fractions
  regions     64 trust regions (boxes of half-width 0.1 around the 64 best data points) of 1024 starts each, starts grouped by region
  embedding   one d = 8 embedding centred at the middle of the cube, full scale
  plain_again the plain leg once more, after the others: `plain_spread_ms` is the difference of the two plain legs' device times, the
              run-to-run spread that `identity_total_minus_plain_minus_sub_ms` has to be read against
Times are HIP-event device times of the scopes (sls_prof_get), the mean of `repeat` calls after one warm-up call of the same shape;
`wall_ms` is the host clock around a call.  `sub_ms_per_round` is sub_expand + sub_fold per lock-step round (the last expand, for
x_out, included); `sub_share_of_plain_round` compares it with the plain leg's device time per round, `total_minus_plain_ms` the whole
leg with the plain one.  No hardware counters are read."""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import subspace_cases as sc  # noqa: E402
from util import sls  # noqa: E402

SCOPES = ("cross_gram", "acq_gemm", "var_gemm", "grad_gemm", "finalize", "lbfgs", "sub_expand", "sub_fold")


def leg(ctx, gp, call, repeat, n_starts, n_local):
    call()                                                       # warm-up: workspaces, code objects
    ctx.prof_reset()
    t0 = time.perf_counter()
    for _ in range(repeat):
        res = call()
    wall = (time.perf_counter() - t0) * 1e3 / repeat
    st = gp.last_stats()
    assert st["evals_cap"] == n_starts * n_local
    rounds = st["rounds"]
    row = {"wall_ms": round(wall, 3), "rounds": rounds, "evals_issued": st["evals_issued"], "live_at_end": st["live_at_end"],
           "live_fraction": round(st["evals_issued"] / st["evals_cap"], 5), "value": res["value"], "stages": {}}
    for name in SCOPES:
        ms, launches = ctx.prof_get(name)
        if launches:
            row["stages"][name] = {"ms": round(ms / repeat, 4), "launches": launches // repeat, "ms_per_round": round(ms / repeat / rounds, 5)}
    row["device_ms"] = round(sum(v["ms"] for v in row["stages"].values()), 3)
    row["device_ms_per_round"] = round(row["device_ms"] / rounds, 4)
    row["sub_ms"] = round(sum(row["stages"].get(k, {}).get("ms", 0.0) for k in ("sub_expand", "sub_fold")), 4)
    row["sub_ms_per_round"] = round(row["sub_ms"] / rounds, 5)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "subspace_timing.json"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--starts", type=int, default=65536)
    ap.add_argument("--regions", type=int, default=64)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--n-local", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    m = sls()
    N, D, S, n_local, K, d = a.N, a.D, a.starts, a.n_local, a.regions, a.d
    rng = np.random.default_rng(N + D)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    starts = np.asfortranarray(rng.uniform(0.0, 1.0, (D, S)))
    ctx = m.Context(0)
    ctx.set_candidate_chunk(S)                                   # bench.py's setting: one pass per round
    gp = m.GP(ctx, X, y, theta, 0.005, m.KERNEL_MATERN52)
    identity = m.SubMaps(np.eye(D), np.zeros(D))
    A, c = sc.box_maps(X[:, np.argsort(-y)[:K]], K, half=0.1)
    regions = m.SubMaps(A, c, np.repeat(np.arange(K), S // K))
    Ae, ce = sc.centred_maps(rng, D, d, 1)
    embedding = m.SubMaps(Ae, ce)
    calls = {
        "plain": lambda: gp.acq_maximize(starts, n_local, m.ACQ_EI, want_all=False),
        "identity": lambda: gp.acq_maximize_sub(identity, starts, n_local, m.ACQ_EI, want_all=False),
        "regions": lambda: gp.acq_maximize_sub(regions, starts[:, :S // K * K], n_local, m.ACQ_EI, want_all=False),
        "embedding": lambda: gp.acq_maximize_sub(embedding, starts[:d], n_local, m.ACQ_EI, want_all=False),
    }
    calls["plain_again"] = calls["plain"]                        # the plain leg once more, last: its run-to-run spread
    doc = {"N": N, "D": D, "starts": S, "n_local": n_local, "kernel": "matern52", "acq": "EI", "regions": K, "embedding_d": d,
           "repeat": a.repeat, "legs": {}}
    ctx.prof_enable(True)
    for name, call in calls.items():
        doc["legs"][name] = leg(ctx, gp, call, a.repeat, S // K * K if name == "regions" else S, n_local)
    plain = doc["legs"]["plain"]
    again = doc["legs"]["plain_again"]
    doc["plain_spread_ms"] = round(abs(again["device_ms"] - plain["device_ms"]), 3)
    doc["plain_spread_by_stage_ms"] = {k: round(abs(again["stages"][k]["ms"] - v["ms"]), 3) for k, v in plain["stages"].items()}
    for name, row in doc["legs"].items():
        if name not in ("plain", "plain_again"):
            row["sub_share_of_plain_round"] = round(row["sub_ms_per_round"] / plain["device_ms_per_round"], 6)
            row["total_minus_plain_ms"] = round(row["device_ms"] - plain["device_ms"], 3)
    ident = doc["legs"]["identity"]
    doc["identity_same_search"] = bool(ident["rounds"] == plain["rounds"] and ident["evals_issued"] == plain["evals_issued"] and
                                       ident["value"] == plain["value"])
    doc["identity_total_minus_plain_minus_sub_ms"] = round(ident["device_ms"] - plain["device_ms"] - ident["sub_ms"], 3)
    gp.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
