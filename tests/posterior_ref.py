"""numpy restatements behind the joint-posterior tests (tests/test_gpu_posterior.py, tests/test_gpu_posterior_edges.py,
tests/test_posterior_api_cpu.py): the ARD
kernels, the latent posterior covariance in its triangular form, and the normal generator of sls_random_normal /
sls_gp_sample_posterior (Philox4x64-10 as numpy.random.Philox runs it, the uniform map, Box-Muller)."""
import numpy as np
import scipy.linalg as sla

MASK64 = (1 << 64) - 1
SE, MATERN52 = 0, 1


def ard_kernel(XA, XB, theta, kernel):
    """k(XA[:, i], XB[:, j]) for the columns of XA (D x P) and XB (D x Q): P x Q."""
    ell = np.asarray(theta[1:], dtype=np.float64)[:, None]
    A, B = XA / ell, XB / ell
    q = np.sum(A * A, axis=0)[:, None] + np.sum(B * B, axis=0)[None, :] - 2.0 * A.T @ B
    q = np.maximum(q, 0.0)
    a = theta[0]
    if kernel == SE:
        return a * np.exp(-0.5 * q)
    s = np.sqrt(5.0 * q)
    return a * (1.0 + s + (5.0 / 3.0) * q) * np.exp(-s)


def posterior(X, y, Xs, theta, b, kernel):
    """(mu, cov, cond(K_y)) of the latent function: cov = Kss - W^T W, W = solve_triangular(chol(K_y), K*)."""
    N = X.shape[1]
    Ky = ard_kernel(X, X, theta, kernel) + b * np.eye(N)
    L = np.linalg.cholesky(Ky)
    Ks = ard_kernel(X, Xs, theta, kernel)
    W = sla.solve_triangular(L, Ks, lower=True)
    Kss = ard_kernel(Xs, Xs, theta, kernel)
    mu = Ks.T @ sla.cho_solve((L, True), y)
    ev = np.linalg.eigvalsh(Ky)
    return mu, Kss - W.T @ W, ev[-1] / ev[0]


def pick_rows(M, n, seed, always=()):
    """A fixed set of n distinct rows of 0 .. M - 1 (sorted) that contains every row of `always` below M: the rows at which a test
    compares a covariance too large for a full host reference."""
    keep = sorted({int(r) for r in always if 0 <= r < M})
    rest = np.setdiff1d(np.arange(M), keep)
    extra = np.random.default_rng(seed).choice(rest, size=min(max(n - len(keep), 0), rest.size), replace=False)
    return np.sort(np.concatenate([np.asarray(keep, dtype=np.int64), extra.astype(np.int64)]))


def posterior_rows(X, y, Xs, theta, b, kernel, rows):
    """(mu[rows], cov[rows, :]) of posterior(): K(Xs[rows], Xs) - W[:, rows]^T W, without the M x M prior block."""
    N = X.shape[1]
    rows = np.asarray(rows)
    L = np.linalg.cholesky(ard_kernel(X, X, theta, kernel) + b * np.eye(N))
    Ks = ard_kernel(X, Xs, theta, kernel)
    W = sla.solve_triangular(L, Ks, lower=True)
    mu = Ks[:, rows].T @ sla.cho_solve((L, True), y)
    return mu, ard_kernel(Xs[:, rows], Xs, theta, kernel) - W[:, rows].T @ W


def sample_chunk(Mp):
    """Samples per device pass of sls_gp_sample_posterior at Mp = round_up(M, 128) padded points (capi_post.hip): 2^24 / Mp, rounded
    down to 128, at least 128.  A test of the second chunk restates the rule here and asserts that its shape crosses it."""
    return max(128, ((1 << 24) // Mp) // 128 * 128)


def philox_block(seed, block):
    """The four 64-bit outputs of Philox4x64-10 with key (seed, 0) on counter (block, 0, 0, 0), through numpy.random.Philox.
    numpy increments the 256-bit counter BEFORE it generates (pinned by tests/test_posterior_api_cpu.py), so the state is set to
    one less than the block wanted."""
    c = (block - 1) & ((1 << 256) - 1)
    ctr = np.array([(c >> (64 * i)) & MASK64 for i in range(4)], dtype=np.uint64)
    g = np.random.Philox(key=np.array([seed & MASK64, 0], dtype=np.uint64), counter=ctr)
    return [int(v) for v in g.random_raw(4)]


def philox_rounds(seed, block):
    """The same block from the published round function (Salmon et al., SC 2011), in plain Python integers."""
    M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
    W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
    x = [block & MASK64, 0, 0, 0]
    k0, k1 = seed & MASK64, 0
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK64, (k1 + W1) & MASK64
        p0, p1 = M0 * x[0], M1 * x[2]
        x = [(p1 >> 64) ^ x[1] ^ k0, p1 & MASK64, (p0 >> 64) ^ x[3] ^ k1, p0 & MASK64]
    return x


def uniform(x):
    return ((x >> 11) + 0.5) * 2.0 ** -53


def normals(seed, offset, n):
    """Normal numbers offset .. offset + n - 1 of stream `seed`: block t // 4; Box-Muller on the pairs (0, 1), (2, 3) gives
    r01 cos, r01 sin, r23 cos, r23 sin."""
    out = np.empty(n)
    cache = {}
    for i in range(n):
        t = offset + i
        blk = t >> 2
        if blk not in cache:
            cache = {blk: philox_block(seed, blk)}
        x = cache[blk]
        pair = (t >> 1) & 1
        u0, u1 = uniform(x[2 * pair]), uniform(x[2 * pair + 1])
        r = np.sqrt(-2.0 * np.log(u0))
        th = 2 * np.pi * u1
        out[i] = r * np.sin(th) if t & 1 else r * np.cos(th)
    return out


def ulp_distance(a, b):
    """|a - b| in units of the spacing at max(|a|, |b|)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
