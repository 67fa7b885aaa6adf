"""Noisy expected improvement on posterior draws without a GPU: the numpy restatement (tests/qnei_ref.py) against brute-force loops on
a tiny case, its limits (a baseline above / below every value, one point, permuted options), the C ABI's declarations and the Python
wrapper's argument checks."""
import os
import re

import numpy as np
import pytest

import path_ref as ph
import qeubo_ref as qr
import qnei_ref as nr
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, N, F, S, Q, M = 2, 20, 48, 9, 3, 12


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
    t, arg, gap = nr.max_over_points(ref, X)
    return ref, X, sets, t, arg, gap


def test_incumbents_against_loops(case):
    ref, X, sets, t, arg, gap = case
    V = ref.eval_all(X)                                                         # N x S
    for s in range(S):
        best, at = -np.inf, -1
        for j in range(N):
            if V[j, s] > best:
                best, at = V[j, s], j
        assert t[s] == best and arg[s] == at
        assert gap[s] == best - np.delete(V[:, s], at).max()
    # a duplicated point: the lower index is reported; one point: itself; a NaN poisons every draw it reaches
    Xd = np.concatenate([X, X[:, :1]], axis=1)
    t2, arg2, gap2 = nr.max_over_points(ref, Xd)
    assert np.abs(t2 - t).max() <= 1e-13 and np.array_equal(arg2, arg) and np.all(gap2[arg == 0] <= 1e-13)
    t1, arg1, gap1 = nr.max_over_points(ref, X[:, 3:4])
    assert np.abs(t1 - V[3]).max() <= 1e-13 and np.all(arg1 == 0) and np.all(np.isinf(gap1))
    Xn = X.copy()
    Xn[1, 4] = np.nan
    with np.errstate(all="ignore"):
        tn, argn, _ = nr.max_over_points(ref, Xn)
    assert np.all(np.isnan(tn)) and np.all(argn == -1)


def test_value_wins_and_gradient_against_loops(case):
    ref, X, sets, t, _, _ = case
    val, grad, wins, gap = nr.qnei(ref, sets, Q, t)
    V = np.stack([ref.eval_all(sets[i * D:(i + 1) * D]) for i in range(Q)])     # Q x M x S
    assert np.all(val >= 0.0)
    assert np.any(val > 0.0) and np.any(wins.sum(axis=0) < S)                   # improving and non-improving draws both occur
    for m in range(M):
        total, cnt, g = 0.0, np.zeros(Q, int), np.zeros(Q * D)
        for s in range(S):
            best, at = t[s], -1
            for i in range(Q):
                if V[i, m, s] > best:
                    best, at = V[i, m, s], i
            total += best - t[s]
            if at >= 0:
                cnt[at] += 1
                g[at * D:(at + 1) * D] += ref.eval(sets[at * D:(at + 1) * D, m:m + 1], np.array([s]))[1][:, 0]
        assert val[m] == total / S
        assert np.array_equal(wins[:, m], cnt)
        assert np.abs(grad[:, m] - g / S).max() <= 1e-12 * (1 + np.abs(g).max())
        d = min(np.abs(V[:, m, :] - t[None, :]).min(), (np.sort(V[:, m, :], axis=0)[-1] - np.sort(V[:, m, :], axis=0)[-2]).min())
        assert gap[m] == d


def test_baseline_above_and_below_every_value(case):
    ref, X, sets, t, _, _ = case
    val, grad, wins, _ = nr.qnei(ref, sets, Q, np.full(S, 1e3))
    assert np.all(val == 0.0) and np.all(grad == 0.0) and np.all(wins == 0)
    assert not np.any(np.signbit(val))
    low = t - 1e3
    val, grad, wins, _ = nr.qnei(ref, sets, Q, low)
    ev, eg, ew, _ = qr.qeubo(ref, sets, Q)
    assert np.array_equal(wins, ew) and np.array_equal(grad, eg)
    assert np.abs(val - (ev - low.mean())).max() <= 8 * S * np.finfo(float).eps * 1e3


def test_one_point_is_the_mean_improvement(case):
    ref, X, sets, t, _, _ = case
    Xs = sets[:D]
    val, grad, wins, gap = nr.qnei(ref, Xs, 1, t)
    imp = np.maximum(ref.eval_all(Xs) - t[None, :], 0.0)
    assert np.abs(val - imp.mean(axis=1)).max() <= 4 * S * np.finfo(float).eps * imp.max()
    assert np.array_equal(wins[0], (imp > 0).sum(axis=1))
    assert np.array_equal(gap, np.abs(ref.eval_all(Xs) - t[None, :]).min(axis=1))


def test_option_permutation(case):
    ref, X, sets, t, _, _ = case
    val, grad, wins, gap = nr.qnei(ref, sets, Q, t)
    order = np.array([2, 0, 1])
    rows = np.concatenate([np.arange(i * D, (i + 1) * D) for i in order])
    vo, go, wo, gapo = nr.qnei(ref, sets[rows], Q, t)
    assert np.array_equal(vo, val) and np.array_equal(go, grad[rows]) and np.array_equal(wo, wins[order]) and np.array_equal(gapo, gap)


def test_header_declares_and_binding_exports():
    txt = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = sls()
    for name in ("sls_path_max_over_points", "sls_qnei_eval", "sls_qnei_maximize"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in m.EXPORTS
    assert '"qnei"' in txt and '"path_max"' in txt
    ps = m.PathSamples.__new__(m.PathSamples)            # refused before anything is allocated or called
    ps.D, ps.n_draws, ps.h = 2, 4, None
    for q in (0, 17, -1):
        with pytest.raises(m.SlsError, match="1 .. 16"):
            ps.qnei_eval(np.zeros((2, 1)), q, np.zeros(4))
        with pytest.raises(m.SlsError, match="1 .. 16"):
            ps.qnei_maximize(np.zeros((2, 1)), q, 3, np.zeros(4))
    with pytest.raises(m.SlsError, match="qD x M"):
        ps.qnei_eval(np.zeros((3, 1)), 2, np.zeros(4))
    with pytest.raises(m.SlsError, match="qD x S"):
        ps.qnei_maximize(np.zeros((3, 1)), 2, 3, np.zeros(4))
    with pytest.raises(m.SlsError, match="n_draws = 4"):
        ps.qnei_eval(np.zeros((4, 1)), 2, np.zeros(5))
    with pytest.raises(m.SlsError, match="n_draws = 4"):
        ps.qnei_maximize(np.zeros((4, 1)), 2, 3, np.zeros(3))
    with pytest.raises(m.SlsError, match="Mb >= 1"):
        ps.max_over_points(np.zeros((2, 0)))
    with pytest.raises(m.SlsError, match="D x Mb"):
        ps.max_over_points(np.zeros((3, 5)))
