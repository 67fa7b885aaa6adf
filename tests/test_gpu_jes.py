"""Joint entropy search on the MI355X (sls_jes_*): the scalar terms against 60-digit values, the conditioned optima against
sls_gp_predict, the covariances against sls_gp_predict_cov and the numpy restatement (tests/jes_ref.py), the combiner and the gradient
on the device's own inputs against an mpmath evaluation of the same formula, the conditioning limit, a real refit, central
differences, the guards, the bit-level contract, stale objects and the argument errors.

The JES entry points always take the tiled evaluation and form sigma as the gradient evaluations do.  Where a test compares with
sls_gp_predict to a few eps it pins SLS_WAVE_PATH=0 and SLS_TRI_PREDICT=0, so that both sides run the same route (tests/test_gpu_mes.py).

Bounds that are measured, not guessed: the device is held to a multiple of the error the float64 restatement itself shows against the
mpmath reference on the same inputs (4x for the scalar terms, 8x for the combiner); both figures are printed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch      # before libsls_hip.so is loaded (tests/test_gpu_device_entry.py): the library binds to the HIP runtime torch brought

import gram_ref
import jes_ref
from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SE, MATERN52 = 0, 1
B = 0.05


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.fixture
def same_route(monkeypatch):
    monkeypatch.setenv("SLS_WAVE_PATH", "0")
    monkeypatch.setenv("SLS_TRI_PREDICT", "0")


def problem(D, N, seed, ell=0.5, a=0.5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


def optima(rng, K, X, y):
    """x* uniform with two of them on data points (one for K = 1), f* around max(y) with every fourth below the mean of y from K = 7
    on, so that gamma < 0 occurs (max_value_samples of tests/test_gpu_mes.py)."""
    D, N = X.shape
    xs = rng.uniform(0, 1, (D, K))
    xs[:, 0] = X[:, N // 3]
    if K > 2:
        xs[:, K // 2] = X[:, N // 2]
    fs = y.max() + 0.2 * rng.standard_normal(K)
    if K >= 7:
        fs[1::4] = y.mean() - 0.1 * np.abs(rng.standard_normal(fs[1::4].size))
    return np.asfortranarray(xs), fs


def term_errors(t, tau, dtau, z):
    return np.abs(tau - z["tau"]) / (EPS * np.maximum(1.0, t * t)), np.abs(dtau - z["dtau"]) / np.abs(z["dtau"])


def test_scalar_terms_against_60_digit_values(ctx):
    z = np.load(os.path.join(ROOT, "tests", "golden", "jes_terms.npz"))
    t = z["t"]
    tv, dv = ctx.jes_terms(t)
    e_t, e_d = term_errors(t, tv, dv, z)
    r_t, r_d = term_errors(t, *jes_ref.terms(t), z)
    msg = (f"tau: device {e_t.max():.3f} eps max(1, t^2) at t = {t[e_t.argmax()]:.5g}, float64 restatement {r_t.max():.3f}; "
           f"tau': device {e_d.max():.3g} relative at t = {t[e_d.argmax()]:.5g}, float64 restatement {r_d.max():.3g}")
    print(msg)
    assert e_t.max() <= 4 * r_t.max() and e_d.max() <= 4 * r_d.max(), msg
    lib, dp = sls().lib(), C.POINTER(C.c_double)
    only = np.empty(t.size)
    assert lib.sls_jes_terms(ctx.h, t.ctypes.data_as(dp), C.c_long(t.size), only.ctypes.data_as(dp), None) == 0
    assert np.array_equal(only, tv)
    assert lib.sls_jes_terms(ctx.h, t.ctypes.data_as(dp), C.c_long(t.size), None, only.ctypes.data_as(dp)) == 0
    assert np.array_equal(only, dv)
    assert lib.sls_jes_terms(ctx.h, None, C.c_long(0), None, None) == 0
    assert lib.sls_jes_terms(ctx.h, t.ctypes.data_as(dp), C.c_long(-1), only.ctypes.data_as(dp), None) == -1


CASES = [(SE, 90, 2), (MATERN52, 700, 16), (SE, 300, 96), (MATERN52, 130, 257)]
_FITS = {}


def case(m, ctx, kernel, N, D):
    """The problem, its float64 fit (computed once, shared, never modified) and cond(K_y)."""
    key = (kernel, N, D)
    if key not in _FITS:
        X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
        f = jes_ref.fit(X, y, theta[1:], theta[0], B, kernel)
        ev = np.linalg.eigvalsh(f["K"])
        _FITS[key] = (X, y, theta, f, ev[-1] / ev[0])
    return _FITS[key]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,N,D", CASES)
def test_optima_and_covariances(m, ctx, same_route, kernel, N, D, mode):
    X, y, theta, f, cond = case(m, ctx, kernel, N, D)
    gp = m.GP(ctx, X, y, theta, B, kernel)
    gp.set_sigma_mode(mode)
    rng = np.random.default_rng(5)
    worst = 0.0
    for K in (1, 7, 129, 1024):
        xs, fs = optima(rng, K, X, y)
        star_noise = 1e-8 * theta[0]
        j = gp.jes_create(xs, fs, star_noise)
        mu_s, v = j.optima()
        mu_p, sg_p = gp.predict(xs)
        # the same route on both sides: mu* bit-equal, and v formed THROUGH sigma (sigma sigma + star_noise): bit-equal too
        assert np.array_equal(mu_s, mu_p) and np.array_equal(v, sg_p * sg_p + star_noise)
        o = jes_ref.condition(f, xs, fs, star_noise)
        for M in (1, 129, 300):
            Xs = rng.uniform(0, 1, (D, M))
            Xs[:, 0] = xs[:, 0]
            val, cov = j.eval(Xs, B, want_grad=False, want_cov=True)
            assert cov.shape == (M, K) and np.all(np.isfinite(cov))
            ref = jes_ref.covariances(f, o, Xs)
            tol, _ = jes_ref.covariance_bounds(f, o, Xs, cond)
            worst = max(worst, (np.abs(cov - ref) / tol).max())
            assert np.all(np.abs(cov - ref) <= tol), (K, M, (np.abs(cov - ref) / tol).max(), cond)
            if M == 300 or K == 7:
                # the off-diagonal block of the joint posterior of [Xs, X*] (another route to the same numbers: V^T V of L^-1 k), in
                # both sigma modes and at every K (one M each: the joint call factorises an (M + K)-point covariance)
                joint = gp.predict_cov(np.concatenate([Xs, xs], axis=1))[1][:M, M:]
                tj = tol + 8 * np.sqrt(cond) * EPS * theta[0] * np.sqrt(N)
                assert np.all(np.abs(cov - joint) <= tj), (K, M, (np.abs(cov - joint) / tj).max())
        j.close()
    print(f"kernel {kernel} N {N} D {D} mode {mode}: cond {cond:.3g}, largest covariance error / bound {worst:.3g}")
    gp.close()


def subset(M, K):
    return np.unique(np.linspace(0, M - 1, 4 if K <= 129 else 2).astype(int))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,N,D", CASES)
def test_combiner_on_the_devices_own_inputs(m, ctx, same_route, kernel, N, D, mode):
    """alpha and its gradient from the device's own mu, sigma, grad mu, grad sigma, cov and optima: the reference is the mpmath
    evaluation of the contract's formula from those float64 inputs, the yardstick the error of the float64 restatement against it."""
    X, y, theta, f, cond = case(m, ctx, kernel, N, D)
    gp = m.GP(ctx, X, y, theta, B, kernel)
    gp.set_sigma_mode(mode)
    rng = np.random.default_rng(7)
    worst = dict(dev_v=0.0, ref_v=0.0, dev_g=0.0, ref_g=0.0, raw_g=0.0, cond_g=0.0)
    for K in (1, 7, 129, 1024):
        xs, fs = optima(rng, K, X, y)
        star_noise = 1e-8 * theta[0]
        j = gp.jes_create(xs, fs, star_noise)
        mu_s, v = j.optima()
        o = jes_ref.condition(f, xs, fs, star_noise)
        for M in (1, 129, 300):
            Xs = rng.uniform(0, 1, (D, M))
            mu, sg = gp.predict(Xs)
            dmu, dsg = gp.predict_grad(Xs)
            val, grad, cov = j.eval(Xs, B, want_cov=True)
            dcov = jes_ref.covariances(f, o, Xs, True)[1]
            _, tol_dc = jes_ref.covariance_bounds(f, o, Xs, cond)
            rv, rg, info = jes_ref.alpha(mu, sg, cov, fs, fs - mu_s, v, B, dmu, dsg, dcov)
            assert not info["bad"].any()
            if K >= 7 and M >= 129:
                assert (info["gamma"] < 0).any() and (info["gamma"] > 0).any()
            s, ds = subset(M, K), np.arange(min(D, 6))                       # the mpmath reference: a few points, a few gradient rows
            sd = np.ix_(ds, s)
            mv, mg = jes_ref.alpha_mp(mu[s], sg[s], cov[s], fs, fs - mu_s, v, B, dmu[sd], dsg[sd], dcov[sd])
            floor_v = EPS * np.maximum(1.0, np.abs(mv))
            e_ref = max(np.abs(rv[s] - mv).max(), floor_v.max())
            e_dev = np.abs(val[s] - mv).max()
            # gradient: the device's grad c differs from the restatement's by the conditioning of K_y: sum_k |h_k| tol_dc
            cterm = np.einsum("km,dmk->dm", np.abs(info["H"]), tol_dc)
            floor_g = EPS * np.maximum(1e-300, np.abs(mg).max())
            g_ref = max(np.abs(rg[sd] - mg).max(), floor_g)
            g_dev = (np.abs(grad[sd] - mg) - cterm[sd]).max()
            for kk, vv in (("dev_v", e_dev / e_ref), ("ref_v", e_ref), ("dev_g", g_dev / g_ref), ("ref_g", g_ref),
                           ("raw_g", np.abs(grad[sd] - mg).max()), ("cond_g", cterm[sd].max())):
                worst[kk] = max(worst[kk], vv)
            assert e_dev <= 8 * e_ref, (K, M, e_dev, e_ref)
            assert g_dev <= 8 * g_ref, (K, M, g_dev, g_ref)
            # every point and row against the float64 restatement, loosely: the same formula in the same precision, whose largest
            # amplification of a rounding error is tau' near t = -30 (1e-7 relative, tests/test_jes_cpu.py) in one of K terms
            assert np.abs(val - rv).max() <= 1e-9 * (1.0 + np.abs(rv).max()), (K, M, np.abs(val - rv).max())
            assert np.all(np.abs(grad - rg) <= 1e-7 * np.abs(rg).max() + cterm), (K, M)
            assert np.array_equal(j.eval(Xs, B, want_grad=False), val)             # val alone
        j.close()
    print(f"kernel {kernel} N {N} D {D} mode {mode}: float64 restatement against mpmath: value {worst['ref_v']:.3g}, gradient "
          f"{worst['ref_g']:.3g}; device error / restatement error: value {worst['dev_v']:.3g}, gradient beyond the conditioning term "
          f"{worst['dev_g']:.3g} (device gradient error {worst['raw_g']:.3g}, conditioning term of grad c up to {worst['cond_g']:.3g})")
    gp.close()


def test_conditioning_limit(m, ctx, same_route):
    """star_noise = 1e300: c / v vanishes and the value depends on mu, sigma alone; no K_y conditioning enters."""
    kernel, N, D = MATERN52, 700, 16
    X, y, theta, f, cond = case(m, ctx, kernel, N, D)
    gp = m.GP(ctx, X, y, theta, B, kernel)
    rng = np.random.default_rng(9)
    K, M = 7, 129
    xs, fs = optima(rng, K, X, y)
    j = gp.jes_create(xs, fs, 1e300)
    Xs = rng.uniform(0, 1, (D, M))
    mu, sg = gp.predict(Xs)
    val = j.eval(Xs, B, want_grad=False)
    zero = np.zeros((M, K))
    ones = np.ones(K)
    mu_s, _ = j.optima()
    # m_k = mu, s_k = sigma: the formula with c = 0 (d does not enter)
    rv = jes_ref.alpha(mu, sg, zero, fs, fs - mu_s, ones, B)[0]
    s = subset(M, K)
    mv = jes_ref.alpha_mp(mu[s], sg[s], zero[s], fs, fs - mu_s, ones, B)[0]
    e_ref = max(np.abs(rv[s] - mv).max(), EPS * np.maximum(1.0, np.abs(mv)).max())
    print(f"conditioning limit: float64 restatement {e_ref:.3g}, device {np.abs(val[s] - mv).max():.3g}")
    assert np.abs(val[s] - mv).max() <= 8 * e_ref and np.abs(val - rv).max() <= 9 * e_ref
    j.close()
    gp.close()


@pytest.mark.parametrize("kernel,N,D", [(SE, 90, 2), (MATERN52, 700, 16)])
def test_conditioning_against_a_real_refit(m, ctx, kernel, N, D):
    """K = 1, star_noise = b: the conditioned moments are the predictions of a GP on the data plus (x*, f*), fitted from scratch and
    grown by sls_gp_append_point; alpha is then a function of (mu, sigma) of the first and (m, s) of the second."""
    X, y, theta, f, cond = case(m, ctx, kernel, N, D)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, B, kernel)
    rng = np.random.default_rng(13)
    xs = rng.uniform(0.2, 0.8, (D, 1))
    fs = np.array([y.max() + 0.1])
    j = gp.jes_create(xs, fs, B)
    M = 129
    Xs = rng.uniform(0, 1, (D, M))
    Xs[:, 0] = xs[:, 0] + 1e-3
    val, cov = j.eval(Xs, B, want_grad=False, want_cov=True)
    mu_s, v = j.optima()
    mu, sg = gp.predict(Xs)
    m1 = mu + cov[:, 0] / v[0] * (fs[0] - mu_s[0])
    s1 = sg ** 2 - cov[:, 0] ** 2 / v[0]
    X2, y2 = np.concatenate([X, xs], axis=1), np.concatenate([y, fs])
    g2 = m.GP(ctx, X2, y2, theta, B, kernel)
    gp3 = m.GP(ctx, X, y, theta, B, kernel)
    gp3.append_point(xs[:, 0], fs[0])
    vs = np.abs(gp.matrix(m.GP_ALPHA)).max()
    tol_mu = 1e-10 * a + 4 * cond * EPS * max(vs, 1.0) * a * np.sqrt(N)       # the idiom of tests/test_gpu_mes.py
    tol_s2 = 1e-10 * a + 8 * cond * EPS * a
    for other, name in ((g2, "refit"), (gp3, "append_point")):
        mu2, sg2 = other.predict(Xs)
        e_m, e_s = np.abs(m1 - mu2).max(), np.abs(s1 - sg2 ** 2).max()
        print(f"N {N} {name}: cond {cond:.3g}; m_k {e_m:.3g} (bound {tol_mu:.3g}), s_k^2 {e_s:.3g} (bound {tol_s2:.3g})")
        assert e_m <= tol_mu and e_s <= tol_s2
        other.close()
    j.close()
    gp.close()


@pytest.mark.parametrize("kernel,N,D,mode", [(SE, 90, 2, 0), (MATERN52, 700, 16, 1), (MATERN52, 130, 257, 0)])
def test_gradient_against_central_differences(m, ctx, kernel, N, D, mode):
    X, y, theta, f, cond = case(m, ctx, kernel, N, D)
    gp = m.GP(ctx, X, y, theta, B, kernel)
    gp.set_sigma_mode(mode)
    rng = np.random.default_rng(17)
    xs, fs = optima(rng, 7, X, y)
    j = gp.jes_create(xs, fs, 1e-8 * theta[0])
    Xs = rng.uniform(0.05, 0.95, (D, 8))
    val, grad = j.eval(Xs, B)
    h = 1e-6
    for d in range(min(D, 4)):
        E = np.zeros((D, 8))
        E[d] = h
        fd = (j.eval(Xs + E, B, want_grad=False) - j.eval(Xs - E, B, want_grad=False)) / (2 * h)
        err = np.abs(fd - grad[d]).max()
        print(f"N {N} D {D} central differences, d = {d}: {err:.3g} (|grad| max {np.abs(grad).max():.3g})")
        assert err <= 1e-6 * (1.0 + np.abs(grad).max())                         # the bound of the MES test
    j.close()
    gp.close()


def test_second_row_block_of_the_solve(m, ctx):
    """Np > 2048: W = K_y^-1 K(X, X*) crosses into the solve's second row block."""
    N, D, K, M = 2100, 3, 5, 129
    X, y, theta = problem(D, N, seed=31, ell=0.2)
    f = jes_ref.fit(X, y, theta[1:], theta[0], B, MATERN52)
    ev = np.linalg.eigvalsh(f["K"])
    cond = ev[-1] / ev[0]
    gp = m.GP(ctx, X, y, theta, B, MATERN52)
    rng = np.random.default_rng(2)
    xs, fs = optima(rng, K, X, y)
    j = gp.jes_create(xs, fs, 1e-8)
    o = jes_ref.condition(f, xs, fs, 1e-8)
    Xs = rng.uniform(0, 1, (D, M))
    val, grad, cov = j.eval(Xs, B, want_cov=True)
    ref, dref = jes_ref.covariances(f, o, Xs, True)
    tol, tol_dc = jes_ref.covariance_bounds(f, o, Xs, cond)
    print(f"N {N}: cond {cond:.3g}, covariance error / bound {(np.abs(cov - ref) / tol).max():.3g}")
    assert np.all(np.abs(cov - ref) <= tol)
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    j.close()
    gp.close()


@pytest.mark.parametrize("kernel", [SE, MATERN52])
def test_beyond_the_gram_guard(m, ctx, kernel):
    """l = 3e-3 at (N, D) = (129, 6) (tests/test_gpu_short_length_scales_paths.py): the handle forms every Gram route from raw
    coordinate differences, and so do K(X, X*), k(x, x*) and the data term of the gradient here."""
    N, D, K = 129, 6, 7
    r = gram_ref.problem(N, D, 3e-3)
    f = jes_ref.fit(r["X"], r["y"], r["ell"], r["a"], r["b"], kernel)
    ev = np.linalg.eigvalsh(f["K"])
    cond = ev[-1] / ev[0]
    gp = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], kernel)
    rng = np.random.default_rng(4)
    # optima and candidates within a length scale of data points (anywhere else the posterior is the prior)
    xs = np.clip(r["X"][:, 41:41 + 3 * K:3] + r["ell"][:, None] * 0.5 * rng.standard_normal((D, K)) / np.sqrt(D), 0, 1)
    fs = r["y"].max() + 0.1 * rng.standard_normal(K)
    fs[1] = r["y"].mean() - 0.1
    Xs = np.clip(r["X"][:, 40:40 + 3 * 24:3] + r["ell"][:, None] * 0.7 * rng.standard_normal((D, 24)) / np.sqrt(D), 0, 1)
    Xs[:, :K] = xs + r["ell"][:, None] * 0.3 * rng.standard_normal((D, K)) / np.sqrt(D)
    Xs = np.clip(Xs, 0, 1)
    j = gp.jes_create(xs, fs, 1e-8)
    o = jes_ref.condition(f, xs, fs, 1e-8)
    val, grad, cov = j.eval(Xs, r["b"], want_cov=True)
    ref = jes_ref.covariances(f, o, Xs)
    tol, _ = jes_ref.covariance_bounds(f, o, Xs, cond)
    assert np.abs(ref).max() > 0.05 * r["a"]                                       # the covariances are there
    print(f"kernel {kernel}: cond {cond:.3g}, covariance error / bound {(np.abs(cov - ref) / tol).max():.3g}")
    assert np.all(np.abs(cov - ref) <= tol)
    h = 1e-9                                                                       # l / 3e6
    sub = np.arange(8)
    for d in range(3):
        E = np.zeros((D, 8))
        E[d] = h
        fd = (j.eval(Xs[:, sub] + E, r["b"], want_grad=False) - j.eval(Xs[:, sub] - E, r["b"], want_grad=False)) / (2 * h)
        err = np.abs(fd - grad[d, sub]).max()
        print(f"  central differences, d = {d}: {err:.3g} (|grad| max {np.abs(grad[:, sub]).max():.3g})")
        # rounding of the difference quotient: cond eps |alpha| / h, against gradients of order 1 / l
        assert err <= 1e-6 * (1.0 + np.abs(grad[:, sub]).max()) + 4 * cond * EPS / h
    j.close()
    gp.close()


def test_guards(m, ctx, same_route):
    """b = 0, query points on the data points (the grid of the MES guard test): wherever the device's sigma is below 1e-10 the value
    and the gradient are exactly 0; everywhere they are finite.  A candidate exactly on an optimum with star_noise = 0 takes the
    collapsed-term rule and is finite."""
    D, N = 2, 25
    g = np.linspace(0.05, 0.95, 5)
    X = np.array([[a, c] for a in g for c in g]).T.copy()
    y = np.sin(3 * X[0]) * np.cos(2 * X[1])
    theta = np.array([0.5, 0.15, 0.15])
    gp = m.GP(ctx, X, y, theta, 0.0, MATERN52)
    Xs = np.concatenate([X, np.full((D, 1), 0.5001)], axis=1)
    _, sg = gp.predict(Xs)
    guard = sg < 1e-10
    assert guard[:N].sum() >= 1 and not guard[N]
    xs = np.array([[0.31, 0.77], [0.62, 0.18], [0.5001, 0.5001]]).T.copy()
    j = gp.jes_create(xs, np.array([y.max() + 0.1, y.max() + 0.3, 0.0]), 0.0)
    val, grad = j.eval(Xs, 1e-4)
    assert np.array_equal(val[guard], np.zeros(guard.sum())) and np.array_equal(grad[:, guard], np.zeros((D, guard.sum())))
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    # Xs[:, N] IS optimum 2 and star_noise = 0: c = v = sigma^2, s^2 = 0: the term is log noise_var
    mu_s, v = j.optima()
    v2, c2 = j.eval(Xs[:, N:], 1e-4, want_grad=False, want_cov=True)
    assert abs(c2[0, 2] - v[2]) <= 64 * EPS * theta[0] and np.isfinite(v2[0]) and v2[0] != 0.0
    j.close()
    gp.close()


def test_bit_contract(m, ctx):
    D, N, M, K = 5, 300, 300, 64
    X, y, theta = problem(D, N, seed=21)
    gp = m.GP(ctx, X, y, theta, B, MATERN52)
    rng = np.random.default_rng(3)
    Xs = rng.uniform(0, 1, (D, M))
    xs, fs = optima(rng, K, X, y)
    j = gp.jes_create(xs, fs, 1e-8)
    val, grad, cov = j.eval(Xs, B, want_cov=True)
    v2, g2, c2 = j.eval(Xs, B, want_cov=True)
    assert np.array_equal(val, v2) and np.array_equal(grad, g2) and np.array_equal(cov, c2)          # repeated call
    perm = rng.permutation(M)
    vp, gpm, cp = j.eval(Xs[:, perm], B, want_cov=True)
    assert np.array_equal(vp, val[perm]) and np.array_equal(gpm, grad[:, perm]) and np.array_equal(cp, cov[perm])
    sub = np.array([7, 200, 131])
    vs, gs, cs = j.eval(Xs[:, sub], B, want_cov=True)
    assert np.array_equal(vs, val[sub]) and np.array_equal(gs, grad[:, sub]) and np.array_equal(cs, cov[sub])
    ctx.set_candidate_chunk(128)
    vc, gc, cc = j.eval(Xs, B, want_cov=True)
    ctx.set_candidate_chunk(16384)
    assert np.array_equal(vc, val) and np.array_equal(gc, grad) and np.array_equal(cc, cov)          # nor the candidate chunk
    assert np.array_equal(j.eval(Xs, B, want_grad=False), val)                                       # val alone
    vg, gg = j.eval(Xs, B)
    assert np.array_equal(vg, val) and np.array_equal(gg, grad)                                      # cov asked for or not
    # the first K' optima of this object against an object of those K' optima: the same conditioned optima, the same covariances
    for Kq in (1, 7):
        jq = gp.jes_create(xs[:, :Kq], fs[:Kq], 1e-8)
        assert all(np.array_equal(a[:Kq], b) for a, b in zip(j.optima(), jq.optima()))
        assert np.array_equal(jq.eval(Xs, B, want_grad=False, want_cov=True)[1], cov[:, :Kq])
        jq.close()
    j.close()
    gp.close()


def test_stale_object_and_argument_errors(m, ctx):
    D, N, K = 2, 30, 3
    X, y, theta = problem(D, N, seed=9)
    gp = m.GP(ctx, X, y, theta, B, SE)
    lib, dp = m.lib(), C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    Xs = np.asfortranarray(np.full((D, 3), 0.5))
    val, grad = np.empty(3), np.empty((D, 3), order="F")
    xs, fs = np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (D, K))), np.array([1.0, 1.2, 1.4])
    x, v, idx = np.empty(D), C.c_double(), C.c_long()

    def refused(rc, word):
        msg = lib.sls_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def create(g, xp, fp, Kc, sn):
        h = C.c_void_p()
        rc = lib.sls_jes_create(g, xp, fp, Kc, C.c_double(sn), C.byref(h))
        assert rc == 0 or not h.value
        return rc, h

    ctx.prof_enable(True)
    ctx.prof_reset()
    refused(create(gp.h, p(xs), p(fs), 0, 0.0)[0], "K = 0")
    refused(create(gp.h, p(xs), p(fs), 1025, 0.0)[0], "K = 1025")
    for bad in (np.nan, np.inf, -np.inf):
        fb, xb = fs.copy(), xs.copy(order="F")
        fb[1] = bad
        xb[1, 2] = bad
        refused(create(gp.h, p(xs), p(fb), K, 0.0)[0], "f_star[1]")
        refused(create(gp.h, p(xb), p(fs), K, 0.0)[0], "optimum 2")
    refused(create(gp.h, p(xs), p(fs), K, -1e-9)[0], "star_noise")
    refused(create(gp.h, p(xs), p(fs), K, np.inf)[0], "star_noise")
    refused(create(gp.h, p(xs), p(fs), K, np.nan)[0], "star_noise")
    refused(create(None, p(xs), p(fs), K, 0.0)[0], "gp is NULL")
    refused(create(gp.h, None, p(fs), K, 0.0)[0], "x_star is NULL")
    refused(create(gp.h, p(xs), None, K, 0.0)[0], "f_star is NULL")
    refused(lib.sls_jes_create(gp.h, p(xs), p(fs), K, C.c_double(0.0), None), "out is NULL")
    for name in ("jes_setup", "jes", "jes_cov", "cross_gram"):
        assert ctx.prof_get(name)[1] == 0, name                                   # nothing was launched
    rc, h = create(gp.h, p(xs), p(fs), K, 0.0)
    assert rc == 0 and h.value

    def ev(hh, nv, Xp, M, vp):
        return lib.sls_jes_eval(hh, C.c_double(nv), Xp, M, vp, p(grad), None)

    def mx(hh, nv, sp, opts=None):
        return lib.sls_jes_maximize(hh, C.c_double(nv), sp, 3, 5, opts, C.c_long(0), p(x), C.byref(v), C.byref(idx), None, None)

    ctx.prof_reset()
    for nv in (0.0, -1.0, np.inf, np.nan):
        refused(ev(h, nv, p(Xs), 3, p(val)), "noise_var")
        refused(mx(h, nv, p(Xs)), "noise_var")
    refused(ev(None, B, p(Xs), 3, p(val)), "j is NULL")
    refused(ev(h, B, None, 3, p(val)), "Xs is NULL")
    refused(ev(h, B, p(Xs), 3, None), "val is NULL")
    refused(ev(h, B, p(Xs), -1, p(val)), "M = -1")
    refused(mx(None, B, p(Xs)), "j is NULL")
    refused(mx(h, B, None), "starts is NULL")
    opts = m.LbfgsOpts()
    opts.struct_size = 999
    refused(mx(h, B, p(Xs), C.byref(opts)), "struct_size")
    refused(lib.sls_jes_optima(None, None, None), "j is NULL")
    for name in ("jes", "jes_cov", "cross_gram"):
        assert ctx.prof_get(name)[1] == 0, name
    assert ev(h, B, None, 0, None) == 0                                           # M = 0: nothing to do
    assert ev(h, B, p(Xs), 3, p(val)) == 0 and np.all(np.isfinite(val))
    assert mx(h, B, p(Xs)) == 0
    assert lib.sls_jes_optima(h, None, None) == 0
    # stale: a refit, a sigma-mode switch, an appended point (each changes the generation); no stale state is used, nothing is launched
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda")
    yd = torch.from_numpy(np.ascontiguousarray(y + 0.01)).to("cuda")
    for change in (lambda: gp.refit_dev(Xd.data_ptr(), yd.data_ptr()), lambda: gp.set_sigma_mode(1),
                   lambda: gp.append_point(np.full(D, 0.3), 0.1)):
        change()
        ctx.prof_reset()
        refused(ev(h, B, p(Xs), 3, p(val)), "sls_jes_create")
        refused(mx(h, B, p(Xs)), "sls_jes_create")
        refused(lib.sls_jes_optima(h, p(val), None), "sls_jes_create")
        assert ctx.prof_get("jes")[1] == 0 and ctx.prof_get("cross_gram")[1] == 0
        assert lib.sls_jes_destroy(h) == 0
        rc, h = create(gp.h, p(xs), p(fs), K, 0.0)
        assert rc == 0 and ev(h, B, p(Xs), 3, p(val)) == 0
    ctx.prof_enable(False)
    assert lib.sls_jes_destroy(h) == 0 and lib.sls_jes_destroy(None) == 0
    gp.close()
