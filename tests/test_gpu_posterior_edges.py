"""Joint posterior (sls_gp_predict_cov, sls_gp_sample_posterior) at the edges of its tiling, against numpy (tests/posterior_ref.py):
D = 1, D > 64 and D > 128 (the depth of post_cov_kernel's prior contraction and the column blocks of XsT), Matern over many N
tiles (C* parked in V's block), M = 1 / 127 / 128 / 129 / 257 (a lone live row next to identity padding), M = 8191 / 8192 (the
limit: 2080 lower tiles) and samples in the second sample chunk (the s0 > 0 stream and output offsets)."""
import numpy as np
import pytest

import path_ref as ph
import posterior_ref as pr
from util import sls

pytestmark = pytest.mark.gpu
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


def cov_tol(a, b, N, cond):
    """The bound of test_gpu_posterior.test_covariance_against_numpy."""
    if N <= 1000:
        return 1e-10 * a
    # cov = Kss - |L^-1 k|^2: an error of cond(L) eps ||L^-1|| in the triangular inverse moves |L^-1 k|^2 by at most
    # 2 |L^-1 k| cond(L) eps ||L^-1|| |k| <= 2 sqrt(a) sqrt(cond(K_y)) eps sqrt(N) a / sqrt(b)  (|L^-1 k|^2 <= a, ||L^-1|| <= b^-1/2,
    # |k| <= sqrt(N) a); both sides carry such an error, plus the N-term sums of |V|^2 (N eps a each), and a factor 10 covers
    # the constants of the products
    return 10 * (2 * 2 * np.sqrt(a) * np.sqrt(cond) * EPS * np.sqrt(N) * a / np.sqrt(b) + 2 * N * EPS * a)


def _report(name, **ratios):
    print("RATIO", name, " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


def _check_against_numpy(m, ctx, D, N, M, kernel, ell, seed, b=0.01):
    X, y, Xs, theta = problem(D, N, M, seed=seed, ell=ell)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    mu, cov = gp.predict_cov(Xs)
    gp.close()
    mu_r, cov_r, cond = pr.posterior(X, y, Xs, theta, b, kernel)
    # not a diagonal matrix: the off-diagonal entries take part in the comparison
    off = np.abs(cov_r - np.diag(np.diag(cov_r)))
    assert M == 1 or off.max() > 1e-3 * a, off.max()
    tol = cov_tol(a, b, N, cond)
    err, err_mu = np.abs(cov - cov_r).max(), np.abs(mu - mu_r).max()
    _report(f"cov[D={D},N={N},M={M},k={kernel}]", cov=err / tol, mu=err_mu / (1e-10 * (np.abs(mu_r).max() + a)), cond=cond)
    assert cov.shape == (M, M) and np.array_equal(cov, cov.T)
    assert err <= tol, (err, tol, cond)
    assert err_mu <= 1e-10 * (np.abs(mu_r).max() + a)


@pytest.mark.parametrize("kernel", [pr.SE, pr.MATERN52])
@pytest.mark.parametrize("D,N,M", [(1, 30, 200), (70, 90, 150), (130, 200, 260), (300, 140, 129)])
def test_covariance_over_d(m, ctx, D, N, M, kernel):
    """Dp = round_up(D, 16) = 16 (one k-slab), 80, 144 and 304; XsT has 128, 128, 256 and 384 columns.  ell = 0.3 sqrt(D) keeps the
    kernel values away from 0 and from a."""
    _check_against_numpy(m, ctx, D, N, M, kernel, ell=0.3 * np.sqrt(D), seed=D * 1000 + N)


@pytest.mark.parametrize("D,N,M", [(6, 1300, 300), (16, 2048, 520)])
def test_matern_over_many_n_tiles(m, ctx, D, N, M):
    """11 and 16 tiles of N: the Matern path parks C* in V's block before the triangular product overwrites it."""
    assert N > 8 * 128
    _check_against_numpy(m, ctx, D, N, M, pr.MATERN52, ell=0.5, seed=D * 1000 + N)


@pytest.mark.parametrize("kernel", [pr.SE, pr.MATERN52])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 257])
def test_m_at_tile_edges(m, ctx, M, kernel):
    D, N, b = 5, 200, 0.005
    X, y, Xs, theta = problem(D, N, M, seed=900 + M)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    mu, cov = gp.predict_cov(Xs)
    mu_r, cov_r, cond = pr.posterior(X, y, Xs, theta, b, kernel)
    assert cov.shape == (M, M) and np.array_equal(cov, cov.T)
    err = np.abs(cov - cov_r).max()
    assert err <= 1e-10 * a, (err, cond)
    assert np.abs(mu - mu_r).max() <= 1e-10 * (np.abs(mu_r).max() + a)
    # the diagonal against sls_gp_predict, as test_symmetry_and_diagonal_against_predict
    d = np.maximum(np.diag(cov), 0.0)
    mu_p, sg_p = gp.predict(Xs)
    assert np.abs(mu - mu_p).max() <= 1e-12 * (np.abs(mu_p).max() + a)
    err_d = np.abs(d - sg_p ** 2).max()
    assert err_d <= 4 * cond * EPS * a + 1e-12 * a       # default mode (explicit K_y^-1): accurate to cond(K_y) eps a
    gp.set_sigma_mode(m.SIGMA_CHOLESKY_SOLVE)
    _, sg_c = gp.predict(Xs)
    err_c = np.abs(d - sg_c ** 2).max()
    _report(f"m_edge[M={M},k={kernel}]", cov=err / (1e-10 * a), diag=err_d / (4 * cond * EPS * a + 1e-12 * a), chol=err_c / (1e-12 * a))
    assert err_c <= 1e-12 * a
    if M == 1:
        assert abs(cov[0, 0] - sg_c[0] ** 2) <= 1e-12 * a
    gp.close()


LIMIT = dict(D=12, N=64, ell=0.3, b=0.01, seed=8192)


@pytest.mark.parametrize("M", [8191, 8192])
def test_covariance_at_the_m_limit(m, ctx, M):
    """POST_MAX_M: 64 tile rows, 2080 lower tiles, the tile enumeration through sqrt(8 t + 1) at its largest t.  The host reference
    is the 256 rows posterior_ref.pick_rows chooses (test_posterior_api_cpu pins posterior_rows against the full form)."""
    D, N, b = LIMIT["D"], LIMIT["N"], LIMIT["b"]
    assert ph.round_up(M, 128) == 8192
    X, y, Xs, theta = problem(D, N, M, seed=LIMIT["seed"], ell=LIMIT["ell"])
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, pr.SE)
    mu, cov = gp.predict_cov(Xs)
    gp.close()
    assert np.array_equal(cov, cov.T)
    rows = pr.pick_rows(M, 256, seed=1, always=(0, 127, 128, 8063, 8190, 8191))
    assert rows.size == 256 and {0, 127, 128, 8063, 8190} <= set(rows.tolist()) and ((M - 1) in rows)
    mu_r, cov_r = pr.posterior_rows(X, y, Xs, theta, b, pr.SE, rows)
    off = np.abs(cov_r)
    off[np.arange(rows.size), rows] = 0.0
    assert off.max() > 1e-3 * a
    err, err_mu = np.abs(cov[rows] - cov_r).max(), np.abs(mu[rows] - mu_r).max()
    _report(f"m_limit[{M}]", cov=err / (1e-10 * a), mu=err_mu / (1e-10 * (np.abs(mu_r).max() + a)))
    assert err <= 1e-10 * a, err
    assert err_mu <= 1e-10 * (np.abs(mu_r).max() + a)


def test_samples_at_the_m_limit(m, ctx):
    """Three samples at M = 8192 (a 64-block factorisation): no jitter (cond(cov) ~ 80 for this problem) and mu + chol(cov) Z."""
    D, N, b, M, S, seed = LIMIT["D"], LIMIT["N"], LIMIT["b"], 8192, 3, 4242
    X, y, Xs, theta = problem(D, N, M, seed=LIMIT["seed"], ell=LIMIT["ell"])
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, pr.SE)
    mu, cov = gp.predict_cov(Xs)
    F, jit = gp.sample_posterior(Xs, S, seed)
    gp.close()
    assert F.shape == (M, S) and jit == 0.0
    Z = ctx.random_normal(seed, 0, M * S).reshape((S, M)).T
    Ls = np.linalg.cholesky(cov)
    err = np.abs(F - mu[:, None] - Ls @ Z).max()
    _report("samples_m_limit", f=err / (1e-9 * a))
    assert err <= 1e-9 * a, err


@pytest.mark.parametrize("kernel", [pr.SE, pr.MATERN52])
def test_samples_in_the_second_chunk(m, ctx, kernel):
    """4100 samples at M = 4096: 4096 samples per device pass, so samples 4096 .. 4099 come from a second pass (s0 = 4096: the
    stream offset s0 M of normal_fill and the output offset s0 M of the copy)."""
    D, N, M, S, b, seed = 16, 64, 4096, 4100, 0.01, 555
    chunk = pr.sample_chunk(ph.round_up(M, 128))
    assert chunk == 4096 and S > chunk
    X, y, Xs, theta = problem(D, N, M, seed=4096 + kernel, ell=0.3)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    mu, cov = gp.predict_cov(Xs)
    ev = np.linalg.eigvalsh(cov)
    assert ev[-1] / ev[0] <= 1e6, ev[-1] / ev[0]   # a Cholesky factor's forward error grows with cond(cov)
    F, jit = gp.sample_posterior(Xs, S, seed)
    gp.close()
    assert F.shape == (M, S) and jit == 0.0
    cols = np.arange(4094, 4100)                   # two samples of the first pass, four of the second
    assert cols[0] < chunk <= cols[2]
    Z = np.stack([ctx.random_normal(seed, int(s) * M, M) for s in cols], axis=1)
    # the generator on the host side: the test does not rest on the device generator alone
    Zh = np.stack([ph.normals(seed, int(s) * M, M) for s in cols], axis=1)
    ulp = pr.ulp_distance(Z, Zh).max()
    Ls = np.linalg.cholesky(cov)
    err = np.abs(F[:, cols] - mu[:, None] - Ls @ Z).max()
    _report(f"second_chunk[{kernel}]", f=err / (1e-9 * a), ulp=ulp / 4, cond=ev[-1] / ev[0])
    assert ulp <= 4, ulp
    assert err <= 1e-9 * a, err
