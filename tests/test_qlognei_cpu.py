"""Log-space noisy expected improvement on posterior draws without a GPU: the numpy restatement (tests/qlognei_ref.py) against
explicit loops on test_qnei_cpu.py's tiny case, its scalar terms against 50-digit values, central differences, the sandwich against
qNEI, a baseline far above every value, one point and one draw, permuted options, the escape case of the maximiser test
(tests/qlognei_cases.py), the C ABI's declarations and the Python wrapper's argument checks."""
import math
import os
import re

import numpy as np
import pytest

import path_ref as ph
import qlognei_cases as qc
import qlognei_ref as lr
import qnei_ref as nr
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
D, N, F, S, Q, M = 2, 20, 48, 9, 3, 12
TAUS = [(1e-6, 1e-2), (0.05, 0.05)]


def problem(D, N, seed, ell=0.5, a=0.5):
    """tests/test_gpu_path_sample.py's generator."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


@pytest.fixture(scope="module")
def case():
    X, y, theta = problem(D, N, seed=2)
    ref = ph.PathRef(X, y, theta, 0.02, ph.MATERN52, S, F, seed=5)
    sets = np.random.default_rng(3).uniform(0, 1, (Q * D, M))
    t, _, _ = nr.max_over_points(ref, X)
    return ref, X, sets, t


def scalar_L(a):
    if a < -36.0:
        return a
    if a >= 0.0:
        return math.log(a + math.log1p(math.exp(-a)))
    return math.log(math.log1p(math.exp(a)))


def scalar_R(a):
    if a < -36.0:
        return 1.0
    if a >= 0.0:
        return 1.0 / ((1.0 + math.exp(-a)) * (a + math.log1p(math.exp(-a))))
    return math.exp(a) / ((1.0 + math.exp(a)) * math.log1p(math.exp(a)))


@pytest.mark.parametrize("tau0,taum", TAUS)
def test_restatement_against_loops(case, tau0, taum):
    ref, X, sets, t = case
    out = lr.qlognei(ref, sets, Q, t, tau0, taum)
    V = np.stack([ref.eval_all(sets[i * D:(i + 1) * D]) for i in range(Q)])     # Q x M x S
    _, _, rw, _ = nr.qnei(ref, sets, Q, t)
    assert np.array_equal(out["wins"], rw)
    for m in range(M):
        l = np.array([[math.log(tau0) + scalar_L((V[i, m, s] - t[s]) / tau0) for s in range(S)] for i in range(Q)])
        rho = np.array([[scalar_R((V[i, m, s] - t[s]) / tau0) / tau0 for s in range(S)] for i in range(Q)])
        ms, pi = np.empty(S), np.empty((Q, S))
        for s in range(S):
            mq = max(l[:, s])
            z = sum(math.exp((l[i, s] - mq) / taum) for i in range(Q))
            ms[s] = mq + taum * math.log(z)
            pi[:, s] = [math.exp((l[i, s] - mq) / taum) / z for i in range(Q)]
        mx = max(ms)
        z = sum(math.exp(ms[s] - mx) for s in range(S))
        value = mx + math.log(z) - math.log(S)
        om = np.array([math.exp(ms[s] - mx) / z for s in range(S)])
        c = om[None, :] * pi * rho
        g = np.zeros(Q * D)
        gabs = 0.0
        for i in range(Q):
            for s in range(S):
                gs = ref.eval(sets[i * D:(i + 1) * D, m:m + 1], np.array([s]))[1][:, 0]
                g[i * D:(i + 1) * D] += c[i, s] * gs
                gabs += c[i, s] * np.abs(gs).max()
        assert abs(out["val"][m] - value) <= 8 * EPS * (1 + abs(value))
        assert np.abs(out["c"][:, m, :] - c).max() <= 1e-12 * c.max()
        assert abs(out["A"][m] - c.sum()) <= 1e-12 * c.sum() and abs(out["G"][m] - gabs) <= 1e-12 * gabs
        assert np.abs(out["grad"][:, m] - g).max() <= 1e-11 * gabs
        assert out["rho_max"][m] == rho.max()


def test_terms_against_50_digit_values():
    z = np.load(os.path.join(ROOT, "tests", "golden", "qlognei_terms.npz"))
    a, L, R = z["a"], z["L"], z["R"]
    for x in (0.0, 1e-3, 0.5413, 3.0, 35.9999, 36.0001, 40.0, 700.0, 745.2, 800.0, 1e4, 1e9):
        assert x in a and (-x in a)
    assert a.size == 12 + 11 + 400 and np.all(np.isfinite(L)) and np.all(np.isfinite(R)) and np.all(R > 0)
    gL, gR = lr.terms(a)
    eL, eR = np.abs(gL - L) / (EPS * (1 + np.abs(L))), np.abs(gR - R) / (EPS * R)
    print(f"L within {eL.max():.3g} eps (1 + |L|), R within {eR.max():.3g} eps")
    assert eL.max() <= 4 and eR.max() <= 4
    sL, sR = np.array([scalar_L(x) for x in a]), np.array([scalar_R(x) for x in a])    # the branches one number at a time
    assert np.all(np.abs(sL - L) <= 4 * EPS * (1 + np.abs(L))) and np.all(np.abs(sR - R) <= 4 * EPS * R)


@pytest.mark.parametrize("tau0,taum", TAUS)
def test_central_differences(case, tau0, taum):
    """d value / d x by central differences.  The value's curvature along a coordinate is at most about (|grad f| / tau0)^2 (1 + 1/taum)
    (softplus, then the softmax over the options), so a step h = 1e-3 tau0 min(1, taum) moves every argument of an exponential by
    about 1e-3 |grad f| and the difference quotient is good to about 1e-6 |grad f|^2 relative; |grad f| is below 10 here.  Rounding
    adds eps (1 + |value|) / h, and eps x / h relative from x + h itself."""
    ref, X, sets, t = case
    out = lr.qlognei(ref, sets, Q, t, tau0, taum)
    h = 1e-3 * tau0 * min(1.0, taum)
    worst = 0.0
    for r in range(Q * D):
        up, dn = sets.copy(), sets.copy()
        up[r] += h
        dn[r] -= h
        step = up[r] - dn[r]
        vu = lr.qlognei(ref, up, Q, t, tau0, taum, want_G=False)["val"]
        vd = lr.qlognei(ref, dn, Q, t, tau0, taum, want_G=False)["val"]
        cd = (vu - vd) / step
        tol = 1e-3 * out["G"] + 8 * EPS * (1 + np.abs(out["val"])) / h + 4 * EPS / h * out["G"]
        worst = max(worst, (np.abs(cd - out["grad"][r]) / tol).max())
        assert np.all(np.abs(cd - out["grad"][r]) <= tol), (r, cd, out["grad"][r], tol)
    print(f"central differences within {worst:.3g} of the tolerance")


@pytest.mark.parametrize("tau0,taum", TAUS + [(1e-2, 1e-2)])
def test_sandwich_against_qnei(case, tau0, taum):
    ref, X, sets, t = case
    qn = nr.qnei(ref, sets, Q, t)[0]
    assert np.any(qn == 0.0) and np.any(qn > 0.0)
    ev = np.exp(lr.qlognei(ref, sets, Q, t, tau0, taum, want_G=False)["val"])
    hi = Q ** taum * (qn + tau0 * math.log(2.0))
    assert np.all(ev >= qn * (1 - 1e-12)) and np.all(ev <= hi * (1 + 1e-12)), (qn, ev, hi)


@pytest.mark.parametrize("tau0,taum", TAUS)
def test_baseline_far_above_every_value(case, tau0, taum):
    """Every c is positive: log c, the sum of the three factors' logarithms, is finite.  As a double, c is positive at (0.05, 0.05);
    at the default temperatures a factor exp(-x) with x > 745 rounds to 0 for the options and draws far below the set's best (an
    option 1e-5 below the best of its draw has x = 1e-5 / (tau0 taum) = 1000), so there only 3.7 % of the weights are nonzero
    doubles: nothing is negative or non-finite, every set's largest weight is positive, and with it the gradient."""
    ref, X, sets, t = case
    out = lr.qlognei(ref, sets, Q, np.full(S, 1e3), tau0, taum)
    assert np.all(np.isfinite(out["val"])) and np.all(np.isfinite(out["c"])) and np.all(out["c"] >= 0.0)
    assert np.all(np.isfinite(out["log_c"]))
    if (tau0, taum) == (0.05, 0.05):
        assert np.all(out["c"] > 0.0)
    assert np.all(out["c"].max(axis=(0, 2)) > 0.0) and np.all(out["A"] > 0.0)
    assert np.all(np.abs(out["grad"]).max(axis=0) > 0.0)
    assert np.all(out["wins"] == 0)
    assert np.all(nr.qnei(ref, sets, Q, np.full(S, 1e3))[0] == 0.0)


@pytest.mark.parametrize("tau0,taum", TAUS)
def test_one_point_and_one_draw(case, tau0, taum):
    ref, X, sets, t = case
    Xs = sets[:D]
    out = lr.qlognei(ref, Xs, 1, t, tau0, taum)
    a = (ref.eval_all(Xs) - t[None, :]) / tau0
    # one point: the log of the mean of tau0 softplus(a) over the draws -- directly where that mean does not underflow
    with np.errstate(all="ignore"):
        direct = np.log((tau0 * np.exp(lr.terms(a)[0])).mean(axis=1))
    ok = np.isfinite(direct)
    assert ok.any() and np.all(np.abs(out["val"] - direct)[ok] <= 16 * EPS * (1 + np.abs(direct[ok])))
    l = math.log(tau0) + lr.terms(a)[0]
    shifted = l.max(axis=1) + np.log(np.exp(l - l.max(axis=1, keepdims=True)).sum(axis=1)) - math.log(S)
    assert np.all(np.abs(out["val"] - shifted) <= 16 * EPS * (1 + np.abs(shifted)))
    one = ph.PathRef(ref.X, ref.y, ref.theta, ref.b, ref.kernel, 1, F, seed=5)
    t1 = nr.max_over_points(one, X)[0]
    out = lr.qlognei(one, sets, Q, t1 + 0.1, tau0, taum)
    V = np.stack([one.eval_all(sets[i * D:(i + 1) * D]) for i in range(Q)])[:, :, 0]
    l = math.log(tau0) + lr.terms((V - t1[0] - 0.1) / tau0)[0]
    want = l.max(axis=0) + taum * np.log(np.exp((l - l.max(axis=0)) / taum).sum(axis=0))
    assert np.abs(out["val"] - want).max() <= 16 * EPS * (1 + np.abs(want).max())
    assert np.all(np.isfinite(out["grad"])) and np.all(np.abs(out["grad"]).max(axis=0) > 0)


@pytest.mark.parametrize("tau0,taum", TAUS)
def test_option_permutation(case, tau0, taum):
    ref, X, sets, t = case
    a = lr.qlognei(ref, sets, Q, t, tau0, taum, want_G=False)
    order = np.array([2, 0, 1])
    rows = np.concatenate([np.arange(i * D, (i + 1) * D) for i in order])
    b = lr.qlognei(ref, sets[rows], Q, t, tau0, taum, want_G=False)
    assert np.array_equal(b["wins"], a["wins"][order])
    # exact: the sum over the options that divides a draw's weights is the order-free fixed-point sum, the draws keep their order
    assert np.array_equal(b["c"], a["c"][order]) and np.array_equal(b["grad"], a["grad"][rows])
    assert np.all(np.abs(b["val"] - a["val"]) <= 8 * EPS * (1 + np.abs(a["val"])))


def test_escape_case_on_the_cpu():
    """The maximiser test's case (tests/qlognei_cases.py): the asserted starts have qNEI exactly 0 with a margin, and a bounded L-BFGS
    on the restatement of the log form ends them where qNEI is positive."""
    e = qc.escape_case()
    ref, t, starts = e["ref"], e["t"], e["starts"]
    qn = nr.qnei(ref, starts, qc.ESC_Q, t)
    dead = np.flatnonzero(qn[0] == 0.0)
    assert set(qc.ESC_ASSERTED) <= set(dead.tolist())
    assert np.all(qn[3][qc.ESC_ASSERTED] >= 1e-3)       # no value within 1e-3 of its baseline: dead on any device
    ends, vals = qc.escape_cpu_run(e)
    after = nr.qnei(ref, ends, qc.ESC_Q, t)[0]
    print("qNEI at the ends of the asserted starts:", after[qc.ESC_ASSERTED])
    assert np.all(after[qc.ESC_ASSERTED] >= qc.ESC_MARGIN)


def test_header_declares_and_binding_exports():
    txt = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = sls()
    for name in ("sls_qlognei_terms", "sls_qlognei_eval", "sls_qlognei_maximize"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in m.EXPORTS
    assert re.search(r"#define\s+SLS_QLOGNEI_TAU_RELU\s+1e-6\b", code) and re.search(r"#define\s+SLS_QLOGNEI_TAU_MAX\s+1e-2\b", code)
    assert '"qlognei"' in txt and "not built" not in txt and "out of scope here" not in txt
    ps = m.PathSamples.__new__(m.PathSamples)            # refused before anything is allocated or called
    ps.D, ps.n_draws, ps.h = 2, 4, None
    for q in (0, 17, -1):
        with pytest.raises(m.SlsError, match="1 .. 16"):
            ps.qlognei_eval(np.zeros((2, 1)), q, np.zeros(4))
        with pytest.raises(m.SlsError, match="1 .. 16"):
            ps.qlognei_maximize(np.zeros((2, 1)), q, 3, np.zeros(4))
    with pytest.raises(m.SlsError, match="qD x M"):
        ps.qlognei_eval(np.zeros((3, 1)), 2, np.zeros(4))
    with pytest.raises(m.SlsError, match="qD x S"):
        ps.qlognei_maximize(np.zeros((3, 1)), 2, 3, np.zeros(4))
    with pytest.raises(m.SlsError, match="n_draws = 4"):
        ps.qlognei_eval(np.zeros((4, 1)), 2, np.zeros(5))
    with pytest.raises(m.SlsError, match="n_draws = 4"):
        ps.qlognei_maximize(np.zeros((4, 1)), 2, 3, np.zeros(3))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(m.SlsError, match="tau_relu"):
            ps.qlognei_eval(np.zeros((4, 1)), 2, np.zeros(4), tau_relu=bad)
        with pytest.raises(m.SlsError, match="tau_max"):
            ps.qlognei_eval(np.zeros((4, 1)), 2, np.zeros(4), tau_max=bad)
        with pytest.raises(m.SlsError, match="tau_relu"):
            ps.qlognei_maximize(np.zeros((4, 1)), 2, 3, np.zeros(4), tau_relu=bad)
        with pytest.raises(m.SlsError, match="tau_max"):
            ps.qlognei_maximize(np.zeros((4, 1)), 2, 3, np.zeros(4), tau_max=bad)
