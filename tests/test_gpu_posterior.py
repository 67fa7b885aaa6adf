"""Joint posterior at a set of query points on the MI355X (sls_gp_predict_cov, sls_gp_sample_posterior, sls_random_normal): the
covariance against numpy / scipy fp64 and against scikit-learn's fixtures, its exact symmetry and its diagonal against
sls_gp_predict, growth through sls_gp_append_point, the generator against its numpy restatement, the samples against
mu + chol(cov + j I) Z in numpy, reproducibility, singular covariances, argument errors and the optimisers' pybind surface."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.stats

import posterior_ref as pr
from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def problem(D, N, M, seed, ell=0.5, a=0.5, spread=1.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    Xs = 0.5 + spread * (rng.uniform(0.0, 1.0, (D, M)) - 0.5)
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, Xs, theta


@pytest.mark.parametrize("D,N,M,kernel", [(8, 40, 50, pr.SE), (32, 90, 200, pr.MATERN52), (16, 1000, 700, pr.SE),
                                          (16, 2048, 4096, pr.SE)])
def test_covariance_against_numpy(m, ctx, D, N, M, kernel):
    b = 0.01
    X, y, Xs, theta = problem(D, N, M, seed=D * 1000 + N)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    mu, cov = gp.predict_cov(Xs)
    mu_r, cov_r, cond = pr.posterior(X, y, Xs, theta, b, kernel)
    err = np.abs(cov - cov_r).max()
    if N <= 1000:
        tol = 1e-10 * a
    else:
        # cov = Kss - |L^-1 k|^2: an error of cond(L) eps ||L^-1|| in the triangular inverse moves |L^-1 k|^2 by at most
        # 2 |L^-1 k| cond(L) eps ||L^-1|| |k| <= 2 sqrt(a) sqrt(cond(K_y)) eps sqrt(N) a / sqrt(b)  (|L^-1 k|^2 <= a, ||L^-1|| <= b^-1/2,
        # |k| <= sqrt(N) a); both sides carry such an error, plus the N-term sums of |V|^2 (N eps a each), and a factor 10 covers
        # the constants of the products.  cond(K_y) ~ 2e2 here: tol ~ 2e-11
        tol = 10 * (2 * 2 * np.sqrt(a) * np.sqrt(cond) * EPS * np.sqrt(N) * a / np.sqrt(b) + 2 * N * EPS * a)
    assert err <= tol, (err, tol, cond)
    assert np.abs(mu - mu_r).max() <= 1e-10 * (np.abs(mu_r).max() + a)
    gp.close()


@pytest.mark.parametrize("name", ["se", "matern"])
def test_covariance_against_sklearn_fixtures(m, ctx, name):
    f = np.load(os.path.join(ROOT, "golden", "cov_fixtures.npz"))
    theta = f[f"{name}_theta"]
    gp = m.GP(ctx, f[f"{name}_X"], f[f"{name}_y"], theta, float(f[f"{name}_b"]), int(f[f"{name}_kernel"]))
    mu, cov = gp.predict_cov(f[f"{name}_Xs"])
    assert np.abs(cov - f[f"{name}_cov"]).max() <= 1e-10 * theta[0]
    assert np.abs(mu - f[f"{name}_mu"]).max() <= 1e-10 * (np.abs(f[f"{name}_mu"]).max() + theta[0])
    gp.close()


@pytest.mark.parametrize("N,M,kernel", [(40, 300, pr.SE), (600, 333, pr.MATERN52)])
def test_symmetry_and_diagonal_against_predict(m, ctx, N, M, kernel):
    D, b = 6, 0.005
    X, y, Xs, theta = problem(D, N, M, seed=N + M)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    mu, cov = gp.predict_cov(Xs)
    assert np.array_equal(cov, cov.T)
    d = np.maximum(np.diag(cov), 0.0)
    mu_p, sg_p = gp.predict(Xs)
    assert np.abs(mu - mu_p).max() <= 1e-12 * (np.abs(mu_p).max() + a)
    # default mode (explicit K_y^-1): accurate to cond(K_y) eps a (sls_hip.h, sls_gp_set_sigma_mode)
    ev = np.linalg.eigvalsh(pr.ard_kernel(X, X, theta, kernel) + b * np.eye(N))
    cond = ev[-1] / ev[0]
    assert np.abs(d - sg_p ** 2).max() <= 4 * cond * EPS * a + 1e-12 * a
    gp.set_sigma_mode(m.SIGMA_CHOLESKY_SOLVE)
    mu2, cov2 = gp.predict_cov(Xs)
    assert np.array_equal(cov2, cov)   # the covariance uses the triangular form whatever the mode
    _, sg_c = gp.predict(Xs)
    assert np.abs(d - sg_c ** 2).max() <= 1e-12 * a
    gp.close()


@pytest.mark.parametrize("N0", [100, 300])
def test_grown_handle_matches_fresh_handle(m, ctx, N0):
    D, M, k = 5, 150, 6
    X, y, Xs, theta = problem(D, N0 + k, M, seed=N0)
    a = theta[0]
    grown = m.GP(ctx, X[:, :N0], y[:N0], theta, 0.01, m.KERNEL_MATERN52)
    for i in range(N0, N0 + k):
        grown.append_point(X[:, i], y[i])
    fresh = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_MATERN52)
    mu_g, cov_g = grown.predict_cov(Xs)
    mu_f, cov_f = fresh.predict_cov(Xs)
    assert np.abs(cov_g - cov_f).max() <= 1e-10 * a
    assert np.abs(mu_g - mu_f).max() <= 1e-10 * (np.abs(mu_f).max() + a)
    grown.close()
    fresh.close()


def test_generator_against_numpy_restatement(ctx):
    for seed in (0, 42, 2 ** 63 + 11):
        for off in (0, 1, 3, 5, 2 ** 32 + 1):
            z = ctx.random_normal(seed, off, 13)
            r = pr.normals(seed, off, 13)
            assert pr.ulp_distance(z, r).max() <= 4, (seed, off, z, r)
    # a window is a slice of the stream
    z = ctx.random_normal(9, 0, 64)
    assert np.array_equal(ctx.random_normal(9, 17, 30), z[17:47])


def test_generator_moments():
    c = sls().Context(0)
    z = c.random_normal(20261016, 0, 10 ** 6)
    c.close()
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert abs(scipy.stats.skew(z)) < 5 * np.sqrt(6.0 / n)
    assert abs(scipy.stats.kurtosis(z)) < 5 * np.sqrt(24.0 / n)
    assert scipy.stats.kstest(z, "norm").pvalue > 1e-4


@pytest.mark.parametrize("M", [64, 700])
def test_samples_are_mu_plus_cholesky_times_z(m, ctx, M):
    D, N, S, seed = 8, 50, 37, 1234
    X, y, Xs, theta = problem(D, N, M, seed=M, ell=0.25)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    mu, cov = gp.predict_cov(Xs)
    ev = np.linalg.eigvalsh(cov)
    assert ev[-1] / ev[0] <= 1e6, ev[-1] / ev[0]   # a Cholesky factor's forward error grows with cond(cov)
    F, jit = gp.sample_posterior(Xs, S, seed)
    assert F.shape == (M, S) and jit == 0.0
    Z = ctx.random_normal(seed, 0, M * S).reshape((S, M)).T
    Ls = np.linalg.cholesky(cov + jit * np.eye(M))
    assert np.abs(F - mu[:, None] - Ls @ Z).max() <= 1e-9 * a
    gp.close()


def test_reproducibility_and_prefix_property(m, ctx):
    D, N, M = 4, 64, 4096
    X, y, Xs, theta = problem(D, N, M, seed=5, ell=0.3)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_MATERN52)
    F1, j1 = gp.sample_posterior(Xs, 4100, 77)      # two chunks of samples at this M
    F2, j2 = gp.sample_posterior(Xs, 4097, 77)
    assert j1 == j2
    assert np.array_equal(F1[:, :4097], F2)
    # the second chunk continues the stream: its samples are not the first chunk's over again
    assert not np.any(F1[:, 4096:] == F1[:, :4])
    F3, _ = gp.sample_posterior(Xs, 3, 77)
    assert np.array_equal(F1[:, :3], F3)
    F4, _ = gp.sample_posterior(Xs, 3, 78)
    assert not np.any(F4 == F3)
    gp.close()


def test_duplicate_points_take_the_jitter(m, ctx):
    D, N, M = 3, 30, 40
    X, y, Xs, theta = problem(D, N, M, seed=3)
    Xs[:, 7] = Xs[:, 21]
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    F, jit = gp.sample_posterior(Xs, 50, 5)
    assert jit > 0.0 and jit <= 1e-6 * theta[0]
    assert np.all(np.isfinite(F))
    Z = ctx.random_normal(5, 0, M * 50)
    assert np.abs(F[7] - F[21]).max() <= 10 * np.sqrt(jit) * np.abs(Z).max()
    gp.close()


def test_argument_errors(m, ctx):
    X, y, Xs, theta = problem(2, 10, 3, seed=1)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    lib = m.lib()
    dp = C.POINTER(C.c_double)
    xs = np.asfortranarray(Xs)
    out = np.empty(64 * 64)
    p = lambda a: a.ctypes.data_as(dp)
    assert lib.sls_gp_predict_cov(gp.h, p(xs), 0, None, p(out)) == 0
    assert lib.sls_gp_sample_posterior(gp.h, p(xs), 0, 1, C.c_ulonglong(1), p(out), None) == 0
    assert lib.sls_gp_predict_cov(gp.h, None, 3, None, p(out)) == -1
    assert lib.sls_gp_predict_cov(gp.h, p(xs), 3, None, None) == -1
    assert lib.sls_gp_predict_cov(None, p(xs), 3, None, p(out)) == -1
    assert lib.sls_gp_sample_posterior(gp.h, p(xs), 3, 0, C.c_ulonglong(1), p(out), None) == -1
    assert lib.sls_gp_sample_posterior(gp.h, None, 3, 2, C.c_ulonglong(1), p(out), None) == -1
    assert lib.sls_gp_sample_posterior(gp.h, p(xs), 3, 2, C.c_ulonglong(1), None, None) == -1
    assert lib.sls_random_normal(ctx.h, C.c_ulonglong(1), C.c_long(0), C.c_long(4), None) == -1
    big = np.full((2, 8193), 0.5, order="F")
    assert lib.sls_gp_predict_cov(gp.h, p(big), 8193, None, p(out)) == m.ERR_UNSUPPORTED
    assert lib.sls_gp_sample_posterior(gp.h, p(big), 8193, 1, C.c_ulonglong(1), p(out), None) == m.ERR_UNSUPPORTED
    gp.close()


@pytest.fixture(scope="module")
def pysls():
    sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "sequential-line-search_amd"))
    import pySequentialLineSearch
    return pySequentialLineSearch


def _check_facade(opt, D):
    rng = np.random.default_rng(2)
    P = rng.uniform(0.0, 1.0, (D, 25))
    cov = opt.get_preference_value_covariance(P)
    sd = opt.get_preference_value_stdevs(P)
    assert cov.shape == (25, 25) and np.array_equal(cov, cov.T)
    assert np.abs(np.maximum(np.diag(cov), 0.0) - sd ** 2).max() <= 1e-10 * max(1.0, float(np.abs(cov).max()))
    F = opt.sample_preference_values(P, 6, 99)
    assert F.shape == (25, 6) and np.all(np.isfinite(F))
    assert np.array_equal(F, opt.sample_preference_values(P, 6, 99))


def test_sequential_line_search_facade(pysls):
    pysls.set_random_seed(4)
    opt = pysls.SequentialLineSearchOptimizer(num_dims=3)
    P0 = np.full((3, 5), 0.5)
    assert np.all(opt.get_preference_value_covariance(P0) == 0.0) and opt.get_preference_value_covariance(P0).shape == (5, 5)
    assert opt.sample_preference_values(P0, 4, 1).shape == (5, 4)
    for t in (0.3, 0.7, 0.5):
        opt.submit_feedback_data(t)
    _check_facade(opt, 3)


def test_preferential_bayesian_optimizer_facade(pysls):
    pysls.set_random_seed(5)
    opt = pysls.PreferentialBayesianOptimizer(num_dims=3)
    for i in (0, 1, 0):
        opt.submit_feedback_data(i)
        opt.determine_next_query()
    _check_facade(opt, 3)
