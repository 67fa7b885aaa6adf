"""tests/lbfgs_ref.py, the restated bounded L-BFGS that the GPU maximiser tests are held to, is itself held to (a) the oracle's C
implementation of the same algorithm, bit for bit, with the oracle's own evaluation as the callable and (b) a problem whose
answer is known in closed form.  No GPU."""
import numpy as np
import pytest

import lbfgs_ref
import util

# (D, N, S, kernel, acq): both kernels, EI and UCB; D below / at / above a lane group of four, odd and even, one D past 64
ORACLE_CASES = [(1, 20, 24, 0, 0), (6, 60, 48, 1, 0), (17, 90, 36, 1, 1), (18, 100, 30, 0, 1), (70, 130, 24, 1, 0), (6, 45, 33, 0, 1)]
N_LOCAL = 20
UCB_H = 2.0


def _oracle_case(oracle, D, N, S, kernel):
    X, y, theta, b = util.synth_problem(oracle, D, N, seed=1234 + D)
    starts = util.synth_candidates(oracle, D, S, seed=77 + D) * 1.4 - 0.2
    starts[:, ::3] = np.round(starts[:, ::3])            # every third start on a corner of the box
    return oracle.Regressor(X, y, theta, b, kernel=kernel), starts


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """Per (case, tolerance): the oracle's run and the restatement's in both summation orders -- computed once."""
    out = {}
    for case in ORACLE_CASES:
        D, N, S, kernel, acq = case
        ref, starts = _oracle_case(oracle, D, N, S, kernel)
        for tol in (0.0, 1e-6):
            ro = ref.acq_maximize(starts, N_LOCAL, acq, UCB_H, diag=True, ftol_rel=tol, xtol_rel=tol)
            rr = {order: lbfgs_ref.run(lambda T: ref.acq_eval_batch(T, acq, UCB_H), starts, N_LOCAL, ftol_rel=tol, xtol_rel=tol,
                                       order=order) for order in ("sequential", "lanes")}
            out[case, tol] = (ro, rr, starts)
    return out


@pytest.mark.parametrize("tol", [0.0, 1e-6])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: "D%d-N%d-S%d-k%d-a%d" % c)
def test_sequential_order_reproduces_the_oracle_bit_for_bit(oracle_runs, case, tol):
    ro, rr, starts = oracle_runs[case, tol]
    r = rr["sequential"]
    assert np.array_equal(r["x_stars"], ro["x_stars"])
    assert np.array_equal(r["y_stars"], ro["y_stars"])
    assert r["index"] == ro["index"] and r["value"] == ro["value"] and np.array_equal(r["x"], ro["x"])
    tested = np.isfinite(ro["armijo_margin"])
    assert np.array_equal(np.isfinite(r["armijo_margin"]), tested)
    np.testing.assert_allclose(r["armijo_margin"][tested], ro["armijo_margin"][tested], rtol=1e-6, atol=0.0)
    # the cases reach what they are there for: starts outside the box were clamped, the ring filled, steps were rejected
    assert (starts < 0.0).any() and (starts > 1.0).any()
    assert r["x_stars"].min() >= 0.0 and r["x_stars"].max() <= 1.0
    assert r["rounds"] == N_LOCAL and r["evals_issued"] <= starts.shape[1] * N_LOCAL
    assert r["evals_issued"] == r["evals"].sum()


def test_oracle_cases_reach_every_form_of_the_step(oracle_runs):
    ring = max(rr["sequential"]["ring_max"].max() for _, rr, _ in oracle_runs.values())
    rejected = max((rr["sequential"]["evals"] - 1 - rr["sequential"]["accepted"]).max() for _, rr, _ in oracle_runs.values())
    early = min(rr["sequential"]["evals"].min() for _, rr, _ in oracle_runs.values())
    stopped_by_tol = any(oracle_runs[c, 1e-6][1]["sequential"]["evals_issued"] < oracle_runs[c, 0.0][1]["sequential"]["evals_issued"]
                         for c in ORACLE_CASES)
    assert ring == 6 and rejected >= 1 and early < N_LOCAL and stopped_by_tol


@pytest.mark.parametrize("tol", [0.0, 1e-6])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: "D%d-N%d-S%d-k%d-a%d" % c)
def test_lane_order_ends_within_1e9_of_sequential_order(oracle_runs, case, tol):
    _, rr, _ = oracle_runs[case, tol]
    a, b = rr["lanes"]["y_stars"], rr["sequential"]["y_stars"]
    gap = np.abs(a - b).max() / np.abs(b).max()
    print(f"lanes vs sequential, case {case}, tol {tol}: largest end-value gap {gap:.3e} of the largest value")
    assert gap <= 1e-9


def test_coord_sum_orders():
    e = 2.0 ** -53                                        # half an ulp of 1: 1 + e rounds to 1
    a = np.array([[1.0], [e], [-1.0], [e], [e]])
    # sequential: 1, 1, 0, e, 2e.   lanes: q0 = 1 + e = 1 (d = 0, 4), q1 = e, q2 = -1, q3 = e: (1 + e) + (-1 + e) = 1 - (1 - e) = e
    assert lbfgs_ref.coord_sum(a, "sequential")[0] == 2.0 * e
    assert lbfgs_ref.coord_sum(a, "lanes")[0] == e
    two = np.array([[0.1, 1.0], [0.2, 2.0], [0.3, 3.0]])   # fewer coordinates than lanes; columns are independent
    assert np.array_equal(lbfgs_ref.coord_sum(two, "lanes"), [(0.1 + 0.2) + (0.3 + 0.0), 6.0])
    assert np.array_equal(lbfgs_ref.coord_sum(two, "sequential"), [(0.1 + 0.2) + 0.3, 6.0])
    with pytest.raises(ValueError):
        lbfgs_ref.coord_sum(a, "pairwise")


# ---- separable concave quadratic  -sum_d c_d (x_d - z_d)^2: the maximiser over the box is clip(z, 0, 1) -------------------------------
def _quadratic(D, seed):
    """An Armijo search on VALUES cannot see a decrease below eps |f|: coordinate d is resolved to sqrt(eps |f*| / c_d) and no
    better, by any implementation.  The test's 1e-8 therefore needs |f*| / min c <= 0.45: the curvatures span 1 .. 1000 and the two
    vertex coordinates outside the box (one per face) sit 0.1 outside with c = 1 and 1.5, |f*| = 0.025, resolution 2.4e-9.
    D = 1 keeps an interior optimum (f* = 0)."""
    rng = np.random.default_rng(seed)
    c = 10.0 ** rng.uniform(0.0, 3.0, D)                  # three decades
    c[-1], c[0] = 1000.0, 1.0
    z = rng.uniform(0.05, 0.95, D)
    if D > 1:
        z[0], z[1], c[1] = -0.1, 1.1, 1.5
    calls = []

    def evaluate(T):
        calls.append(T.shape[1])
        r = np.ascontiguousarray(T) - z[:, None]          # one memory layout: numpy's summation order follows it
        return -(c[:, None] * r * r).sum(axis=0), -2.0 * c[:, None] * r
    starts = rng.uniform(-0.2, 1.2, (D, 12))
    starts[:, ::3] = np.round(starts[:, ::3])
    return evaluate, c, z, starts, calls


@pytest.mark.parametrize("order", ["lanes", "sequential"])
@pytest.mark.parametrize("history", [1, 3, 8])
@pytest.mark.parametrize("D", [1, 7, 40])
def test_quadratic_every_start_ends_at_the_clipped_vertex(D, history, order):
    evaluate, c, z, starts, calls = _quadratic(D, 5 + D)
    # the budget is no bound: with one pair the method is a two-term recurrence, at condition number 1000 it gains a factor
    # ~(sqrt(1000) - 1) / (sqrt(1000) + 1) = 0.94 per step and every start must STOP ON ITS OWN (live_at_end == 0) well inside it
    r = lbfgs_ref.run(evaluate, starts, 1500, history=history, order=order)
    opt = np.clip(z, 0.0, 1.0)
    assert np.abs(r["x_stars"] - opt[:, None]).max() <= 1e-8
    np.testing.assert_allclose(r["y_stars"], -(c * (opt - z) ** 2).sum(), rtol=1e-12, atol=1e-14)
    assert r["ring_max"].max() <= history
    assert sum(calls) == r["evals_issued"] == r["evals"].sum() and len(calls) == r["rounds"]
    assert r["live_at_end"] == 0 and r["evals"].max() < 1000, "every start stops on its own, long before the budget"
    if history == 3 and D > 1:
        assert r["ring_max"].max() == 3 and r["accepted"].max() > 3, "the ring did not wrap"


@pytest.mark.parametrize("D", [1, 7, 40])
def test_quadratic_one_evaluation(D):
    evaluate, c, z, starts, calls = _quadratic(D, 5 + D)
    r = lbfgs_ref.run(evaluate, starts, 1)
    x0 = np.clip(starts, 0.0, 1.0)
    assert np.array_equal(r["x_stars"], x0)
    assert np.array_equal(r["y_stars"], evaluate(x0)[0])
    assert r["evals_issued"] == starts.shape[1] and r["rounds"] == 1 and r["live_at_end"] == starts.shape[1]
    assert not np.isfinite(r["armijo_margin"]).any() and not r["accepted"].any()


@pytest.mark.parametrize("D", [1, 7, 40])
def test_quadratic_start_on_the_optimum_is_evaluated_once(D):
    evaluate, c, z, starts, calls = _quadratic(D, 5 + D)
    starts[:, 4] = np.clip(z, 0.0, 1.0)
    starts[:, 7] = np.where(z < 0.0, -0.1, np.where(z > 1.0, 1.1, z))   # the same point after the clamp
    r = lbfgs_ref.run(evaluate, starts, 50)
    assert r["evals"][4] == 1 and r["evals"][7] == 1
    assert np.array_equal(r["x_stars"][:, 4], np.clip(z, 0.0, 1.0)) and np.array_equal(r["x_stars"][:, 7], r["x_stars"][:, 4])
    assert (np.delete(r["evals"], [4, 7]) > 1).all()
    assert calls[0] == starts.shape[1] and calls[1] == starts.shape[1] - 2, "a finished start is not evaluated again"


def test_live_columns_arrive_in_increasing_start_order():
    evaluate, c, z, starts, calls = _quadratic(7, 12)
    starts = np.clip(starts, 0.0, 1.0)
    starts[3] = np.linspace(0.05, 0.95, starts.shape[1])             # a coordinate that names the start, kept fixed by a zero gradient
    seen = []

    def tagged(T):
        seen.append(T[3].copy())
        v, g = evaluate(T)
        g[3] = 0.0
        return v, g
    lbfgs_ref.run(tagged, starts, 30)
    assert len(seen) > 3 and seen[-1].size < seen[0].size
    assert all((np.diff(s) > 0).all() and np.isin(s, starts[3]).all() for s in seen)
