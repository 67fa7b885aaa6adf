"""Information gain of a choice query on posterior draws without a GPU: the numpy restatement (tests/qbald_ref.py) against explicit
loops on test_qlognei_cpu.py's tiny case, central differences, the weights of a draw summing to zero, the range [0, ln q], one
option and one draw, permuted options, the sensitivity bound the device test holds the kernels to, the C ABI's declarations and the
Python wrapper's argument checks."""
import math
import os
import re

import numpy as np
import pytest

import path_ref as ph
import qbald_ref as br
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
D, N, F, S, Q, M = 2, 20, 48, 9, 3, 12
SCALES = [0.05, 0.01]


def kappa(q, S):
    """The arithmetic of either side: 64 eps, and 4 eps per term of the sums over the options with |l| <= 1 + ln S."""
    return (64 + 4 * q * (1 + math.log(max(S, 2)))) * EPS


def problem(D, N, seed, ell=0.5, a=0.5):
    """tests/test_gpu_path_sample.py's generator."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


@pytest.fixture(scope="module", autouse=True)
def criterion_is_declared():
    """What is restated here is the library's criterion: its entry points are declared, and the second scale is its default."""
    m = sls()
    assert "sls_qbald_eval" in m.EXPORTS and "sls_qbald_maximize" in m.EXPORTS and m.QBALD_SCALE == SCALES[1]


@pytest.fixture(scope="module")
def case():
    X, y, theta = problem(D, N, seed=2)
    ref = ph.PathRef(X, y, theta, 0.02, ph.MATERN52, S, F, seed=5)
    sets = np.random.default_rng(3).uniform(0, 1, (Q * D, M))
    return ref, X, sets


def draw_gradients(ref, sets, q):
    """(q, M, S, D): the gradient of every draw at every option."""
    Mx = sets.shape[1]
    g = np.empty((q, Mx, ref.n_draws, ref.D))
    for i in range(q):
        for s in range(ref.n_draws):
            g[i, :, s, :] = ref.eval(sets[i * ref.D:(i + 1) * ref.D], np.full(Mx, s))[1].T
    return g


@pytest.mark.parametrize("tau", SCALES)
def test_restatement_against_loops(case, tau):
    ref, X, sets = case
    out = br.qbald(ref, sets, Q, tau)
    V = np.stack([ref.eval_all(sets[i * D:(i + 1) * D]) for i in range(Q)])     # Q x M x S
    gf = draw_gradients(ref, sets, Q)
    kap = kappa(Q, S)
    for m in range(M):
        p = np.empty((Q, S))
        wins = [0] * Q
        for s in range(S):
            top = max(V[i, m, s] for i in range(Q))
            wins[[V[i, m, s] for i in range(Q)].index(top)] += 1
            e = [math.exp((V[i, m, s] - top) / tau) for i in range(Q)]
            p[:, s] = [x / sum(e) for x in e]
        pbar = [sum(p[i, s] for s in range(S)) / S for i in range(Q)]
        l = np.array([[math.log(p[i, s]) - math.log(pbar[i]) if p[i, s] > 0 else 0.0 for s in range(S)] for i in range(Q)])
        kl = [sum(p[i, s] * l[i, s] for i in range(Q)) for s in range(S)]
        value = sum(kl) / S
        # the same number as the difference of entropies
        H = lambda r: -sum(x * math.log(x) for x in r if x > 0)
        assert abs(value - (H(pbar) - sum(H(p[:, s]) for s in range(S)) / S)) <= kap * (1 + math.log(Q))
        c = np.array([[p[i, s] * (l[i, s] - kl[s]) / (S * tau) for s in range(S)] for i in range(Q)])
        g = np.zeros(Q * D)
        G = Pw = 0.0
        for i in range(Q):
            for s in range(S):
                g[i * D:(i + 1) * D] += c[i, s] * gf[i, m, s]
                G += abs(c[i, s]) * np.abs(gf[i, m, s]).max()
                Pw += p[i, s] * np.abs(gf[i, m, s]).max() / (S * tau)
        assert list(out["wins"][:, m]) == wins
        assert abs(out["val"][m] - value) <= kap * (1 + abs(value))
        assert np.abs(out["prob"][:, m] - pbar).max() <= 8 * EPS
        assert np.abs(out["p"][:, m, :] - p).max() <= 8 * EPS
        assert np.abs(out["c"][:, m, :] - c).max() <= kap * (np.abs(c).max() + 1 / (S * tau))
        assert abs(out["A"][m] - np.abs(c).sum()) <= 1e-12 * (np.abs(c).sum() + 1 / tau)
        assert abs(out["G"][m] - G) <= 1e-12 * (G + Pw) and abs(out["P"][m] - Pw) <= 1e-12 * Pw
        assert np.abs(out["grad"][:, m] - g).max() <= 1e-11 * (G + Pw)


@pytest.mark.parametrize("tau", SCALES)
def test_central_differences(case, tau):
    """d value / d x by central differences.  The value is a smooth function of z = v / tau with derivatives of order 1 (times ln S),
    so along a coordinate its third derivative is about (|grad f| / tau)^3 and a step h = 1e-3 tau leaves the quotient good to about
    1e-6 |grad f|^2 of P = sum p |grad f| / (S tau); |grad f| is below 10 here.  Rounding adds eps (1 + |value|) / h."""
    ref, X, sets = case
    out = br.qbald(ref, sets, Q, tau)
    h = 1e-3 * tau
    worst = 0.0
    for r in range(Q * D):
        up, dn = sets.copy(), sets.copy()
        up[r] += h
        dn[r] -= h
        step = up[r] - dn[r]
        vu = br.qbald(ref, up, Q, tau, want_G=False)["val"]
        vd = br.qbald(ref, dn, Q, tau, want_G=False)["val"]
        cd = (vu - vd) / step
        scale = out["G"] + out["P"]
        tol = 1e-3 * scale + 8 * EPS * (1 + np.abs(out["val"])) / h + 4 * EPS / h * scale
        worst = max(worst, (np.abs(cd - out["grad"][r]) / tol).max())
        assert np.all(np.abs(cd - out["grad"][r]) <= tol), (r, cd, out["grad"][r], tol)
    print(f"central differences within {worst:.3g} of the tolerance")
    assert np.all(np.abs(out["grad"]).max(axis=0) > 0)


@pytest.mark.parametrize("tau", SCALES + [1e-9, 1e6])
def test_weights_sum_to_zero_and_the_value_is_in_range(case, tau):
    ref, X, sets = case
    out = br.qbald(ref, sets, Q, tau)
    kap = kappa(Q, S)
    assert np.all(np.abs(out["c"].sum(axis=0)) <= kap * out["p"].max(axis=0) * (1 + math.log(S)) / (S * tau))
    assert np.all(out["val"] >= -kap) and np.all(out["val"] <= math.log(Q) + kap)
    assert np.all(np.abs(out["prob"].sum(axis=0) - 1.0) <= Q * EPS)
    if tau == 1e-9:       # one-hot: the entropy of the win frequencies, no weights
        f = out["wins"] / S
        with np.errstate(all="ignore"):
            H = -np.where(f > 0, f * np.log(f), 0.0).sum(axis=0)
        assert out["gap"].min() > 745 * tau
        assert np.all(np.abs(out["val"] - H) <= kap * (1 + math.log(Q)))
        assert np.all(out["c"] == 0.0) and np.all(out["grad"] == 0.0)
        assert np.all(np.abs(out["prob"] - f) <= 2 * EPS)
    if tau == 1e6:        # every option as likely under every draw: nothing to learn
        assert np.all(np.abs(out["val"]) <= 1e-12) and np.all(np.abs(out["prob"] - 1.0 / Q) <= 1e-6)


@pytest.mark.parametrize("tau", SCALES)
def test_one_option_and_one_draw(case, tau):
    ref, X, sets = case
    out = br.qbald(ref, sets[:D], 1, tau)
    assert np.all(out["val"] == 0.0) and np.all(out["grad"] == 0.0) and np.all(out["prob"] == 1.0) and np.all(out["wins"] == S)
    one = ph.PathRef(ref.X, ref.y, ref.theta, ref.b, ref.kernel, 1, F, seed=5)
    out = br.qbald(one, sets, Q, tau)
    assert np.all(out["val"] == 0.0) and np.all(out["c"] == 0.0) and np.all(out["grad"] == 0.0)
    assert np.array_equal(out["prob"], out["p"][:, :, 0])
    # every option the same point
    same = np.tile(sets[:D], (Q, 1))
    out = br.qbald(ref, same, Q, tau)
    assert np.all(np.abs(out["val"]) <= kappa(Q, S)) and np.all(np.abs(out["prob"] - 1.0 / Q) <= kappa(Q, S))


@pytest.mark.parametrize("tau", SCALES)
def test_option_permutation(case, tau):
    ref, X, sets = case
    a = br.qbald(ref, sets, Q, tau)
    order = np.array([2, 0, 1])
    rows = np.concatenate([np.arange(i * D, (i + 1) * D) for i in order])
    b = br.qbald(ref, sets[rows], Q, tau, want_G=False)
    # exact: Z_s is the order-free fixed-point sum and each pbar_i keeps its own order over the draws
    assert np.array_equal(b["wins"], a["wins"][order]) and np.array_equal(b["prob"], a["prob"][order])
    assert np.array_equal(b["p"], a["p"][order])
    # KL_s is a signed sum in index order: to rounding
    kap = kappa(Q, S)
    assert np.all(np.abs(b["val"] - a["val"]) <= kap * (1 + np.abs(a["val"])))
    assert np.all(np.abs(b["grad"] - a["grad"][rows]).max(axis=0) <= kap * (a["G"] + a["P"]))


@pytest.mark.parametrize("tau", SCALES)
@pytest.mark.parametrize("B", [1e-9, 1e-6])
def test_sensitivity_bound(case, tau, B):
    """The bound tests/test_gpu_qbald.py holds the device to (derived there), with the values moved by +-B and the draws' gradients
    kept (B_v = B, B_g = 0): the value within B A' + kappa (1 + |value|), and sum |c' - c| |grad f|_inf -- which bounds every gradient
    component's move -- within eps (2 G + (10 + 2 ln max(S, 2)) P) + kappa (G + P), eps = 2 B / tau.

    A' = A + eps (2 A + (10 + 2 ln max(S, 2)) / tau) is the value bound's second order, which shows at B = 1e-6 (eps = 2e-4 at
    tau = 0.01): by the mean value theorem the value moves by at most B times the largest sum |c| between the two points, and by the
    gradient bound with |grad f| = 1 (G = A, P = sum p / (S tau) = 1 / tau) that sum is within eps (2 A + (10 + 2 ln S) / tau) of A.
    A set with one contested draw (two weights +x, -x) reaches B A itself whenever both signs fall against it."""
    ref, X, sets = case
    out = br.qbald(ref, sets, Q, tau)
    V = np.stack([ref.eval_all(sets[i * D:(i + 1) * D]) for i in range(Q)])
    gabs = np.abs(draw_gradients(ref, sets, Q)).max(axis=3)                      # Q x M x S
    kap, eps = kappa(Q, S), 2 * B / tau
    tol_v = B * (out["A"] + eps * (2 * out["A"] + (10 + 2 * math.log(max(S, 2))) / tau)) + kap * (1 + np.abs(out["val"]))
    tol_g = eps * (2 * out["G"] + (10 + 2 * math.log(max(S, 2))) * out["P"]) + kap * (out["G"] + out["P"])
    rng = np.random.default_rng(17)
    worst_v = worst_g = 0.0
    for _ in range(20):
        val, c, p, pbar = br.weights(V + B * rng.choice([-1.0, 1.0], V.shape), tau)
        dv = np.abs(val - out["val"])
        dg = (np.abs(c - out["c"]) * gabs).sum(axis=(0, 2))
        worst_v, worst_g = max(worst_v, (dv / tol_v).max()), max(worst_g, (dg / tol_g).max())
        assert np.all(dv <= tol_v) and np.all(dg <= tol_g)
        assert np.all(np.abs(pbar - out["prob"]) <= 2 * eps + kap)
    print(f"tau {tau}, B {B}: value moves by {worst_v:.3g} of its bound, the weighted weights by {worst_g:.3g}")


def test_header_declares_and_binding_exports():
    txt = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = sls()
    for name in ("sls_qbald_eval", "sls_qbald_maximize"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in m.EXPORTS
    assert re.search(r"#define\s+SLS_QBALD_SCALE\s+0\.010\b", code) and m.QBALD_SCALE == 0.010
    assert '"qbald"' in txt
    ps = m.PathSamples.__new__(m.PathSamples)            # refused before anything is allocated or called
    ps.D, ps.n_draws, ps.h = 2, 4, None
    for q in (0, 17, -1):
        with pytest.raises(m.SlsError, match="1 .. 16"):
            ps.qbald_eval(np.zeros((2, 1)), q)
        with pytest.raises(m.SlsError, match="1 .. 16"):
            ps.qbald_maximize(np.zeros((2, 1)), q, 3)
    with pytest.raises(m.SlsError, match="qD x M"):
        ps.qbald_eval(np.zeros((3, 1)), 2)
    with pytest.raises(m.SlsError, match="qD x S"):
        ps.qbald_maximize(np.zeros((3, 1)), 2, 3)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 5e-324):
        with pytest.raises(m.SlsError, match="scale"):
            ps.qbald_eval(np.zeros((4, 1)), 2, scale=bad)
        with pytest.raises(m.SlsError, match="scale"):
            ps.qbald_maximize(np.zeros((4, 1)), 2, 3, scale=bad)
