"""Leave-one-out cross-validation of a GP restated in numpy (Rasmussen & Williams, GPML 5.4.2): what sls_nll_loo, sls_gp_loo_grad
and sls_gp_loo compute, four ways --

  * the closed forms in diag(K_y^-1) and alpha (loo_terms);
  * the gradient of L = sum_i logp_i as ONE weight matrix W against dK/dtheta_p (loo_grad_weight: the form the device uses);
  * the same gradient in GPML's per-parameter form, eq. 5.13, with explicit dK/dtheta_p matrices and one product Z_p = K_y^-1 dK_p per
    parameter (loo_grad_gpml): algebraically independent of the weight form;
  * the brute force of N refits on N - 1 points each (loo_brute).

and the log-normal prior terms of sls_gp_loo_grad (capi_map.hip: log_lognormal with the fixed parameters of sls_gp_nll_grad).
Conventions of the package: X is (D, N), theta = (a, r_1..r_D), x = (a, b, r_1..r_D), kernel 0 = ARD squared exponential, 1 = ARD
Matern 5/2."""
import math

import numpy as np

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
PRIOR_MU = dict(a=math.log(0.5), b=math.log(1e-4), r=math.log(0.5))
PRIOR_S2 = 0.5


def scaled_sqdist(X, ell):
    Z = X / np.asarray(ell)[:, None]
    d = Z[:, :, None] - Z[:, None, :]
    return np.sum(d * d, axis=0)


def kernel_matrix(kernel, X, theta):
    """K_f (N x N, no noise)."""
    a, q = theta[0], scaled_sqdist(X, theta[1:])
    if kernel == 0:
        return a * np.exp(-0.5 * q)
    s = np.sqrt(5.0 * q)
    return a * (1.0 + s + (5.0 / 3.0) * q) * np.exp(-s)


def kernel_derivatives(kernel, X, theta):
    """[dK_f/da, dK_f/dr_1, .., dK_f/dr_D], each N x N."""
    a, ell = theta[0], np.asarray(theta[1:])
    q = scaled_sqdist(X, ell)
    K = kernel_matrix(kernel, X, theta)
    if kernel == 0:
        c = K
    else:
        s = np.sqrt(5.0 * q)
        c = a * (5.0 / 3.0) * (1.0 + s) * np.exp(-s)       # -2 dk/dq
    out = [K / a]
    for d in range(X.shape[0]):
        diff = X[d][:, None] - X[d][None, :]
        out.append(c * diff * diff / ell[d] ** 3)
    return out


def k_y(kernel, X, theta, b):
    return kernel_matrix(kernel, X, theta) + b * np.eye(X.shape[1])


def loo_terms_from(Kinv, y):
    alpha = Kinv @ y
    d = np.diag(Kinv).copy()
    mu = y - alpha / d
    var = 1.0 / d
    logp = 0.5 * np.log(d) - alpha * alpha / (2.0 * d) - HALF_LOG_2PI
    return mu, var, logp


def loo_terms(kernel, X, y, theta, b):
    """(mu_-i, var_-i, logp_i, L) from the closed forms."""
    Kinv = np.linalg.inv(k_y(kernel, X, theta, b))
    Kinv = 0.5 * (Kinv + Kinv.T)
    mu, var, logp = loo_terms_from(Kinv, y)
    return mu, var, logp, math.fsum(logp)


def loo_brute(kernel, X, y, theta, b):
    """The same three vectors from N fits of N - 1 points each (N = 1: the prior)."""
    N = X.shape[1]
    Ky = k_y(kernel, X, theta, b)
    mu, var = np.empty(N), np.empty(N)
    for i in range(N):
        o = np.arange(N) != i
        if N == 1:
            mu[i], var[i] = 0.0, Ky[0, 0]
            continue
        ks = Ky[o, i]
        sol = np.linalg.solve(Ky[np.ix_(o, o)], np.column_stack([y[o], ks]))
        mu[i] = ks @ sol[:, 0]
        var[i] = Ky[i, i] - ks @ sol[:, 1]
    logp = -0.5 * np.log(var) - (y - mu) ** 2 / (2.0 * var) - HALF_LOG_2PI
    return mu, var, logp


def loo_weights(Kinv, y):
    """(W, u): dL/dtheta_p = sum_ij W_ij dK_ij/dtheta_p, dL/db = tr W = sum_i (u_i alpha_i - M_ii)."""
    alpha = Kinv @ y
    d = np.diag(Kinv)
    u = Kinv @ (alpha / d)
    c = 0.5 * (1.0 + alpha * alpha / d) / d
    M = Kinv @ (c[:, None] * Kinv)
    return 0.5 * (np.outer(u, alpha) + np.outer(alpha, u)) - M, u


def loo_grad_weight(kernel, X, y, theta, b):
    """(dL/dtheta (D + 1), dL/db) in the weight form."""
    Kinv = np.linalg.inv(k_y(kernel, X, theta, b))
    Kinv = 0.5 * (Kinv + Kinv.T)
    W, _ = loo_weights(Kinv, y)
    g = np.array([np.sum(W * dK) for dK in kernel_derivatives(kernel, X, theta)])
    return g, float(np.trace(W))


def loo_grad_gpml(kernel, X, y, theta, b):
    """The same in GPML eq. 5.13: per parameter Z = K_y^-1 dK, dL = sum_i [alpha_i (Z alpha)_i - 1/2 (1 + alpha_i^2 / d_i) (Z K_y^-1)_ii] / d_i."""
    N = X.shape[1]
    Kinv = np.linalg.inv(k_y(kernel, X, theta, b))
    alpha = Kinv @ y
    d = np.diag(Kinv)
    out = []
    for dK in kernel_derivatives(kernel, X, theta) + [np.eye(N)]:
        Z = Kinv @ dK
        zk = np.einsum("ij,ji->i", Z, Kinv)
        out.append(float(np.sum((alpha * (Z @ alpha) - 0.5 * (1.0 + alpha * alpha / d) * zk) / d)))
    return np.array(out[:-1]), out[-1]


def log_lognormal(x, mu, s2):
    lx = math.log(x)
    return -lx - 0.5 * math.log(2.0 * math.pi * s2) - (lx - mu) ** 2 / (2.0 * s2)


def log_lognormal_d(x, mu, s2):
    return (mu - s2 - math.log(x)) / (s2 * x)


def gp_loo_objective(kernel, X, y, x, want_grad=True):
    """sls_gp_loo_grad: L + the log-normal priors at x = (a, b, r_1..r_D), and its gradient in x."""
    x = np.asarray(x, dtype=float)
    a, b, r = x[0], x[1], x[2:]
    theta = np.concatenate([[a], r])
    _, _, _, L = loo_terms(kernel, X, y, theta, b)
    val = L + log_lognormal(a, PRIOR_MU["a"], PRIOR_S2) + log_lognormal(b, PRIOR_MU["b"], PRIOR_S2)
    val += sum(log_lognormal(v, PRIOR_MU["r"], PRIOR_S2) for v in r)
    if not want_grad:
        return val
    gth, gb = loo_grad_weight(kernel, X, y, theta, b)
    g = np.empty(len(x))
    g[0] = gth[0] + log_lognormal_d(a, PRIOR_MU["a"], PRIOR_S2)
    g[1] = gb + log_lognormal_d(b, PRIOR_MU["b"], PRIOR_S2)
    g[2:] = gth[1:] + np.array([log_lognormal_d(v, PRIOR_MU["r"], PRIOR_S2) for v in r])
    return val, g


# ---- the problems of the GPU tests (tests/test_gpu_loo.py) and of the fixture (tests/golden/make_loo_fixtures.py) ----------------
# (D, N): the prior; tiny; one ragged tile; one full tile; a second row and column tile holding one point; 3 x 3 tiles; more than one
# 128-column tile of the scaled design matrix (twice).
SHAPES = [(1, 1), (1, 5), (3, 37), (17, 128), (17, 129), (5, 257), (129, 130), (257, 40)]
NOISES = [0.005, 1e-6]
FIXTURE_CASES = [(3, 37, 0.005), (3, 37, 1e-6), (8, 40, 0.005)]


def problem(D, N, seed=None):
    """Points of the unit box on a jittered lattice-free design (uniform, seeded), a smooth target plus noise, and length scales short
    enough that K_f alone is well conditioned: cond(K_y) stays below 1e6 down to b = 1e-6 (tests/test_loo_cpu.py asserts it)."""
    rng = np.random.default_rng(1000 * D + N if seed is None else seed)
    X = rng.random((D, N))
    y = np.sin(3.0 * np.sum(X, axis=0) / math.sqrt(D)) + 0.5 * np.cos(5.0 * X[0]) + 0.05 * rng.standard_normal(N)
    # typical squared distance of two uniform points is D / 6: a length scale that keeps neighbours correlated but not redundant
    base = 0.6 * math.sqrt(D / 6.0) * (6.0 / max(N, 6)) ** (1.0 / (2 * D))
    ell = base * (1.0 + 0.3 * np.cos(np.arange(D)))
    theta = np.concatenate([[0.7], ell])
    return np.asfortranarray(X), y, theta


def scaled_problem(D, N, s):
    """problem(D, N) with every length scale multiplied by s: the same points and targets, K_f ever closer to rank deficient."""
    X, y, theta = problem(D, N)
    theta = theta.copy()
    theta[1:] *= s
    return X, y, theta


# ---- the conditioning ladder (tests/test_gpu_loo_conditioning.py, tests/golden/loo_illcond.npz) ---------------------------------
# Rungs (kernel, D, N, s, b): scaled_problem(D, N, s) at b = 1e-8, s chosen per kernel and shape so that cond(K_y) lands in three
# bands.  The cap: a rung's gradient tolerance 100 cond 2.3e-16 max|g| may not exceed 1e-4 max|g|, so cond <= 4e9 (the Matern rungs
# of (3, 37) could not go much higher anyway: cond <= N a / b = 2.6e9).  tests/test_loo_cpu.py asserts band and cap for every rung
# and that numpy itself meets the ladder's bound there.
CONDITIONING_CAP = 4e9
CONDITIONING_BANDS = [(3e5, 3e6), (3e7, 3e8), (1e9, CONDITIONING_CAP)]        # about 1e6, about 1e8, the highest below the cap
RUNG_NOISE = 1e-8
_RUNG_SCALES = {(0, 3, 37): (2.0, 3.0, 4.5), (0, 5, 130): (1.75, 2.75, 4.0), (1, 3, 37): (5.0, 12.0, 28.0), (1, 5, 130): (4.0, 10.0, 20.0)}
RUNGS = [(k, D, N, s, RUNG_NOISE) for (k, D, N), scales in _RUNG_SCALES.items() for s in scales]


def rung_name(kernel, D, N, s, b):
    return f"k{kernel}_D{D}_N{N}_s{s:g}_b{b:g}"


def rung_band(kernel, D, N, s, b):
    return CONDITIONING_BANDS[_RUNG_SCALES[(kernel, D, N)].index(s)]


def ladder_tolerances(cond):
    """(vector, gradient): the bound tests/test_loo_cpu.py::test_against_mpmath holds numpy to -- 10 cond eps for mu (absolute scale
    max|y|), var, logp and L (scale sum|logp|), 100 cond eps max|g| for the D + 2 derivatives."""
    return 10 * cond * 2.3e-16, 100 * cond * 2.3e-16


def direct_form_problem_tiled(N):
    """(17, 257) or (17, 130): one length scale of 0.01 and near-duplicate pairs (offset 1e-7 in one coordinate) whose members sit
    in different 128-tiles -- (3, 200), (130, 7), (256, 129) at N = 257, and a third copy of point 256 at index 9 (offset -1e-7):
    the first two pairs both join tiles 0 and 1, the third tiles 1 and 2, the copy tiles 0 and 2, so that every off-diagonal tile of
    the 3 x 3 grid, on both sides of the diagonal, holds a strongly weighted entry (tests/test_loo_cpu.py asserts it); at N = 130
    the pairs that fit: (3, 129), (128, 7)."""
    X, y, theta = problem(17, N)
    X = X.copy(order="F")
    pairs = [(3, 200, 1e-7), (130, 7, 1e-7), (256, 129, 1e-7), (256, 9, -1e-7)] if N == 257 else [(3, 129, 1e-7), (128, 7, 1e-7)]
    for (i, j, off) in pairs:
        X[:, j] = X[:, i]
        X[2, j] += off
    theta = theta.copy()
    theta[1 + 2] = 0.01
    return X, y, theta, 0.005


def direct_form_problem():
    """(17, 40): one length scale of 0.01 (beyond the guard of the norm expansion) and a near-duplicate pair (offset 1e-7)."""
    X, y, theta = problem(17, 40)
    X = X.copy(order="F")
    X[:, 7] = X[:, 3]
    X[2, 7] += 1e-7
    theta = theta.copy()
    theta[1 + 2] = 0.01
    return X, y, theta, 0.005
