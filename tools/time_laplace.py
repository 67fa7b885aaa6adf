"""Device times of the Laplace posterior for preference data (sls_gp_set_laplace) per profiling scope, beside the plain fit of the same
handle in the same run, and one expected-improvement evaluation round on a Laplace handle against a plain handle in either sigma
mode.  Writes one JSON document (default profiles/laplace_timing.json) and prints it as one line.

    python tools/time_laplace.py [--out FILE] [--sizes 2048,4096,8192]

Shapes: N = 2048, 4096 and 8192, D = 16 (Matern 5/2), about 1.5 N tuple entries (N / 2 tuples of 2-4 options).  Scope times are
HIP-event device times (sls_prof_get), whole calls are host-clock times around the call (each ends in a synchronisation); every
figure is the mean of 3 calls after one warm-up call.  The fit is a new handle per call (sls_gp_create: upload, Gram, factorisation,
inverse, alpha); the set replaces the state of one handle.  The evaluation round is sls_acq_eval with gradient at 4096 points: the
Laplace handle runs the explicit-inverse route with M in the place of K_y^-1.  No hardware counters are read."""
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

LAPLACE_SCOPES = ("laplace_w", "laplace_b", "laplace_potri", "laplace_m")
FIT_SCOPES = ("gram", "potri", "potrf", "trtri", "lauum", "potrf+trtri+lauum")
EVAL_SCOPES = ("cross_gram", "acq_gemm", "var_gemm", "grad_gemm", "finalize")
REPS = 3
M_EVAL = 4096


def mean_of(ctx, call, scopes, reps=REPS):
    """Mean wall time (ms) and mean scope times per call of `reps` calls of call(i) after one warm-up call."""
    call(-1)
    ctx.prof_reset()
    t0 = time.perf_counter()
    for i in range(reps):
        call(i)
    wall = (time.perf_counter() - t0) * 1e3 / reps
    row = {"wall_ms": round(wall, 4)}
    dev = 0.0
    for name in scopes:
        ms, launches = ctx.prof_get(name)
        if launches:
            row[name + "_ms"] = round(ms / reps, 4)
            dev += ms / reps
    row["scopes_ms"] = round(dev, 4)
    return row


def shape(m, ctx, N, D=16):
    rng = np.random.default_rng(N + D)
    X = np.asfortranarray(rng.uniform(0.0, 1.0, (D, N)))
    y = 0.3 * np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.02 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], np.full(D, 0.3 * np.sqrt(D))])
    b = 0.005
    prefs = [tuple(int(i) for i in rng.choice(N, size=int(rng.integers(2, 5)), replace=False)) for _ in range(N // 2)]
    prefs = [tuple(sorted(p, key=lambda i: -y[i])) for p in prefs]      # the chosen point first: the one with the largest y
    Xs = np.asfortranarray(rng.uniform(0.0, 1.0, (D, M_EVAL)))
    doc = {"N": N, "D": D, "kernel": "matern52", "tuples": len(prefs), "tuple_entries": int(sum(len(p) for p in prefs))}
    ctx.prof_enable(True)

    def fit(i):
        g = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
        g.close()
    doc["plain_fit"] = mean_of(ctx, fit, FIT_SCOPES)
    gp = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
    plain = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
    doc["set_laplace"] = mean_of(ctx, lambda i: gp.set_laplace(prefs, 0.01), LAPLACE_SCOPES)
    doc["set_laplace_over_plain_fit_device"] = round(doc["set_laplace"]["scopes_ms"] / doc["plain_fit"]["scopes_ms"], 3)
    doc["ei_round_laplace"] = mean_of(ctx, lambda i: gp.acq_eval(Xs, m.ACQ_EI), EVAL_SCOPES)
    doc["ei_round_plain_explicit_inverse"] = mean_of(ctx, lambda i: plain.acq_eval(Xs, m.ACQ_EI), EVAL_SCOPES)
    plain.set_sigma_mode(m.SIGMA_CHOLESKY_SOLVE)
    doc["ei_round_plain_cholesky_solve"] = mean_of(ctx, lambda i: plain.acq_eval(Xs, m.ACQ_EI), EVAL_SCOPES)
    doc["ei_round_laplace_over_plain_explicit_inverse_device"] = round(
        doc["ei_round_laplace"]["scopes_ms"] / doc["ei_round_plain_explicit_inverse"]["scopes_ms"], 3)
    sm = gp.laplace_summary()
    doc["log_evidence"] = sm["log_evidence"]
    _, sg_l = gp.predict(Xs[:, :256])
    plain.set_sigma_mode(m.SIGMA_EXPLICIT_INVERSE)
    _, sg_p = plain.predict(Xs[:, :256])
    doc["median_sigma_laplace"], doc["median_sigma_plain"] = float(np.median(sg_l)), float(np.median(sg_p))
    np_ = (N + 127) // 128 * 128
    doc["state_device_memory_bytes"] = 5 * 8 * np_ * np_
    ctx.prof_enable(False)
    gp.close()
    plain.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "laplace_timing.json"))
    ap.add_argument("--sizes", default="2048,4096,8192")
    a = ap.parse_args()
    m = sls()
    ctx = m.Context(0)
    doc = {"calls_per_figure": REPS, "eval_points": M_EVAL, "shapes": [shape(m, ctx, int(n)) for n in a.sizes.split(",")]}
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
