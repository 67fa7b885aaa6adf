"""The float64 restatement of the knowledge gradient (tests/kg_ref.py) without a GPU: against the independent mpmath reference (no sort,
no scan), its weights against central differences taken at 50 digits, the slopes against a Gaussian process refitted from scratch
with the hypothetical observation, the closed forms at K = 1, and the degenerate line sets.  The error the restatement shows here is
the yardstick of tests/test_gpu_kg.py."""
import math

import mpmath as mp
import numpy as np
import pytest

import gram_ref
import jes_ref
import kg_cases
import kg_ref

EPS = np.finfo(np.float64).eps


def random_lines(rng, K, own):
    a = rng.standard_normal(K)
    b = rng.standard_normal(K) * rng.uniform(0.01, 2.0)
    if own is not None:
        a = np.append(a, a.max() + own)
        b = np.append(b, abs(rng.standard_normal()))
    return a, b


def breakpoint_error(a, b):
    """What rounding leaves of the breakpoints of the envelope: t = (a - a') / (b' - b) carries eps (|a| + |a'|) / |b' - b| from the
    rounded difference of the intercepts and 2 eps |t| from the difference of the slopes and the division."""
    env, ts = kg_ref.envelope(list(a), list(b))
    worst = 0.0
    for i in range(1, len(env)):
        p, q = env[i - 1], env[i]
        worst = max(worst, EPS * (abs(a[p]) + abs(a[q])) / abs(b[q] - b[p]) + 2 * EPS * abs(ts[i]))
    return worst


@pytest.mark.parametrize("own", [None, 0.7, -0.7], ids=["fixed", "self-above", "self-below"])
@pytest.mark.parametrize("K", [1, 2, 5, 40, 129, 1024])
def test_restatement_against_the_mpmath_reference(K, own):
    rng = np.random.default_rng(7 * K + (0 if own is None else int(10 * own) + 20))
    worst = np.zeros(3)
    for _ in range(6 if K <= 129 else 2):
        a, b = random_lines(rng, K, own)
        v, beta, pi = kg_ref.lines(a, b)
        mv, mb, mpi = kg_ref.lines_mp(a, b)
        dt = breakpoint_error(a, b)
        e = np.array([abs(v - mv), np.abs(beta - mb).max(), np.abs(pi - mpi).max()])
        worst = np.maximum(worst, e)
        # the value is stationary in the breakpoints (the envelope is continuous there): what is left is the rounding of the terms,
        # each (b' - b) f to a few eps, and of their sum; beta and pi move with a breakpoint by at most max |t phi(t)| = 0.242 and
        # max phi = 0.399 per unit of t, at both ends of an interval, plus the rounding of phi and Phi themselves
        assert e[0] <= 8 * EPS * max(1.0, b.max() - b.min() + abs(mv)), (K, own, e[0])
        assert e[1] <= 2 * 0.25 * dt + 4 * EPS and e[2] <= 2 * 0.4 * dt + 4 * EPS, (K, own, e, dt)
        assert abs(pi.sum() - 1.0) <= 4 * EPS and v >= 0.0
    print(f"K {K} self {own}: float64 restatement against mpmath: value {worst[0]:.3g}, beta {worst[1]:.3g}, pi {worst[2]:.3g}")


def emax_mp(a, b):
    v, _, _ = kg_ref._lines_mp(a, b)
    return v + max(mp.mpf(x) for x in a)


@pytest.mark.parametrize("K", [2, 5, 40])
def test_beta_and_pi_against_central_differences(K):
    rng = np.random.default_rng(K)
    a, b = random_lines(rng, K, 0.3)
    _, beta, pi = kg_ref.lines(a, b)
    with mp.workdps(50):
        h = mp.mpf(10) ** -20
        am, bm = [mp.mpf(float(x)) for x in a], [mp.mpf(float(x)) for x in b]
        for j in range(K + 1):
            up, dn = list(am), list(am)
            up[j] += h
            dn[j] -= h
            d_a = float((emax_mp(up, bm) - emax_mp(dn, bm)) / (2 * h))
            up, dn = list(bm), list(bm)
            up[j] += h
            dn[j] -= h
            d_b = float((emax_mp(am, up) - emax_mp(am, dn)) / (2 * h))
            assert abs(pi[j] - d_a) <= 1e-10 and abs(beta[j] - d_b) <= 1e-10, (j, pi[j], d_a, beta[j], d_b)


def kg_value_mp(mu, sg, cov, a, nv, own):
    s = mp.sqrt(sg * sg + nv)
    al, bl = [mp.mpf(float(x)) for x in a], [c / s for c in cov]
    if own:
        al.append(mu)
        bl.append(sg * sg / s)
    return kg_ref._lines_mp(al, bl)[0] + max(al) - max(al[:len(a)])


@pytest.mark.parametrize("nv", [0.05, 0.0])
@pytest.mark.parametrize("own", [True, False])
def test_weights_against_central_differences(own, nv):
    rng = np.random.default_rng(11)
    K, M = 9, 4
    a = rng.standard_normal(K)
    mu = a.max() + np.array([0.4, -0.3, 0.05, -1.0])                               # the self line on both sides of a_max
    sg = rng.uniform(0.3, 1.0, M)
    cov = rng.standard_normal((M, K)) * 0.3
    val, _, info = kg_ref.kg(mu, sg, cov, a, nv, own)
    with mp.workdps(50):
        h = mp.mpf(10) ** -20
        for m in range(M):
            args = [mp.mpf(float(mu[m])), mp.mpf(float(sg[m])), [mp.mpf(float(c)) for c in cov[m]]]
            f = lambda mu_, sg_, cov_: kg_value_mp(mu_, sg_, cov_, a, mp.mpf(nv), own)
            assert abs(val[m] - float(f(*args))) <= 8 * EPS * max(1.0, abs(val[m]))
            d_mu = float((f(args[0] + h, args[1], args[2]) - f(args[0] - h, args[1], args[2])) / (2 * h))
            d_sg = float((f(args[0], args[1] + h, args[2]) - f(args[0], args[1] - h, args[2])) / (2 * h))
            assert abs(info["a_mu"][m] - d_mu) <= 1e-10 and abs(info["a_sigma"][m] - d_sg) <= 1e-10, (m, d_mu, d_sg)
            for k in range(K):
                up, dn = list(args[2]), list(args[2])
                up[k] += h
                dn[k] -= h
                d_c = float((f(args[0], args[1], up) - f(args[0], args[1], dn)) / (2 * h))
                assert abs(info["H"][m, k] - d_c) <= 1e-10, (m, k, d_c)


def test_slopes_against_a_gp_refitted_from_scratch():
    """Append (x, mu + s z) to the data, refit in numpy: the new mean at x_k is a_k + b_k z."""
    rng = np.random.default_rng(3)
    D, N, K, b = 3, 40, 6, 0.05
    X = rng.uniform(0, 1, (D, N))
    y = np.sin(2.0 * X.sum(axis=0)) + 0.05 * rng.standard_normal(N)
    ell = np.full(D, 0.4)
    for kernel in (0, 1):
        f = jes_ref.fit(X, y, ell, 0.5, b, kernel)
        xs = rng.uniform(0, 1, (D, K))
        xs[:, 0] = X[:, 5]
        o = kg_ref.points(f, xs)
        x = rng.uniform(0.2, 0.8, (D, 1))
        p = gram_ref.predict(f, x)
        slope = kg_ref.kg(p["mean"], p["dev"], jes_ref.covariances(f, o, x), o["a"], b)[2]["slope"][0]
        s = math.sqrt(p["dev"][0] ** 2 + b)
        for z in (-2.0, 0.4, 1.3):
            f2 = jes_ref.fit(np.concatenate([X, x], axis=1), np.append(y, p["mean"][0] + s * z), ell, 0.5, b, kernel)
            new = gram_ref.predict(f2, xs)["mean"]
            assert np.abs(new - (o["a"] + slope * z)).max() <= 1e-10, (kernel, z, np.abs(new - (o["a"] + slope * z)).max())


def test_closed_forms_at_one_point():
    assert kg_ref.lines([0.3], [1.7])[0] == 0.0                                    # K = 1 without the self line: exactly 0
    v, beta, pi = kg_ref.lines([0.3], [-2.0])
    assert v == 0.0 and beta[0] == 0.0 and pi[0] == 1.0
    rng = np.random.default_rng(5)
    for _ in range(50):
        a1, mu, bk = rng.standard_normal(), rng.standard_normal(), abs(rng.standard_normal()) + 0.01
        u = (mu - a1) / bk
        expect = (mu - a1) * 0.5 * math.erfc(-u / math.sqrt(2)) + bk * math.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
        got = kg_ref.lines([a1, mu], [0.0, bk])[0] + max(0.0, mu - a1)             # K = 1 plus the self line, b_1 = 0: EI's form
        assert abs(got - expect) <= 8 * EPS * max(1.0, abs(expect))


@pytest.mark.parametrize("name", list(kg_cases.DEGENERATE))
def test_degenerate_line_sets(name):
    a, b = (np.array(v) for v in kg_cases.DEGENERATE[name])
    for bb in (b, -b):
        v, beta, pi = kg_ref.lines(a, bb)
        mv, mb, mpi = kg_ref.lines_mp(a, bb)
        assert abs(v - mv) <= 4 * EPS * max(1.0, abs(mv)) and np.abs(beta - mb).max() <= 4 * EPS and np.abs(pi - mpi).max() <= 4 * EPS
        assert abs(pi.sum() - 1.0) <= 4 * EPS and v >= 0.0 and np.all(np.isfinite(beta))
        if name in ("all slopes equal", "all b = 0"):
            assert v == 0.0 and not beta.any() and pi[int(np.argmax(a))] == 1.0
