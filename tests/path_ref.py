"""numpy restatement of the pathwise posterior function draws (sls_path_*, tests/test_gpu_path_sample.py,
tests/test_gpu_path_edges.py, tests/test_path_sample_cpu.py), following the generator layout include/sls_hip.h documents:

  f_s(x) = sqrt(a/F) sum_l [ w_{s,l} cos(om_l . x~) + w'_{s,l} sin(om_l . x~) ]  +  sum_i v_{s,i} k(x, x_i)
  v_s    = K_y^-1 ( y - f_prior,s(X) - sqrt(b) eps_s ),   x~ = (x - 0.5) / l

frequency l: normal numbers l D .. l D + D - 1 (z); Matern only: u_l = sum_{j<5} z^2 over numbers F D + 5 l + j, om_l = z sqrt(5 / u_l);
B0 = F D (+ 5 F); draw s starts at B0 + s (2F + N): w_s (F), w'_s (F), eps_s (N)."""
import numpy as np

import posterior_ref as pr

SE, MATERN52 = pr.SE, pr.MATERN52


def normals(seed, offset, n):
    """posterior_ref.normals, vectorised: numpy's Philox run over consecutive blocks (its counter is incremented before each block,
    so the state starts one below the first block), then the same uniform map and Box-Muller.  test_path_sample_cpu pins the two
    against each other."""
    if n <= 0:
        return np.empty(0)
    b0, b1 = offset >> 2, (offset + n - 1) >> 2
    c = (b0 - 1) & ((1 << 256) - 1)
    ctr = np.array([(c >> (64 * i)) & pr.MASK64 for i in range(4)], dtype=np.uint64)
    g = np.random.Philox(key=np.array([seed & pr.MASK64, 0], dtype=np.uint64), counter=ctr)
    raw = g.random_raw(4 * (b1 - b0 + 1)).reshape(-1, 4)
    u = ((raw >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    r01, r23 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t01, t23 = 2 * np.pi * u[:, 1], 2 * np.pi * u[:, 3]
    z = np.stack([r01 * np.cos(t01), r01 * np.sin(t01), r23 * np.cos(t23), r23 * np.sin(t23)], axis=1).ravel()
    s = offset - 4 * b0
    return z[s:s + n]


def round_up(n, k):
    return (n + k - 1) // k * k


def eval_chunk(Np, Fp):
    """Candidates per device pass of sls_path_eval / sls_path_maximize (capi_path.hip, chunk_of): 2^26 / max(Np, 2 Fp), rounded down
    to 128 and clamped to 128 .. 16384; Np = round_up(N, 128), Fp = round_up(F, 128)."""
    return max(128, min(16384, ((1 << 26) // max(Np, 2 * Fp)) // 128 * 128))


def create_rows(Np, Fp):
    """Training rows per block of the prior at the data in sls_path_create: 2^26 / (2 Fp), rounded down to 128, within 128 .. Np."""
    return max(128, min(Np, ((1 << 26) // (2 * Fp)) // 128 * 128))


def block0(D, F, kernel):
    """Length of the draw-independent block (the frequencies)."""
    return F * D + (5 * F if kernel == MATERN52 else 0)


def frequencies(seed, D, F, kernel, gen=normals):
    """om (F x D)."""
    z = gen(seed, 0, F * D).reshape(F, D)
    if kernel == MATERN52:
        u = gen(seed, F * D, 5 * F).reshape(F, 5)
        uu = (((u[:, 0] ** 2 + u[:, 1] ** 2) + u[:, 2] ** 2) + u[:, 3] ** 2) + u[:, 4] ** 2
        z = z * np.sqrt(5.0 / uu)[:, None]
    return z


def draw_normals(seed, D, N, F, kernel, n_draws, gen=normals):
    """(w (F x n_draws), w' (F x n_draws), eps (N x n_draws))."""
    B0 = block0(D, F, kernel)
    E = gen(seed, B0, n_draws * (2 * F + N)).reshape(n_draws, 2 * F + N).T
    return E[:F], E[F:2 * F], E[2 * F:]


def feature_kernel(om, a, XA, XB, ell):
    """(a/F) sum_l cos(om_l . (x~ - x~')): the random-feature approximation of k, P x Q."""
    A, B = (XA - 0.5) / ell[:, None], (XB - 0.5) / ell[:, None]
    TA, TB = om @ A, om @ B
    F = om.shape[0]
    return (a / F) * (np.cos(TA).T @ np.cos(TB) + np.sin(TA).T @ np.sin(TB))


def features(om, a, X, ell):
    """Phi (2F x P): sqrt(a/F) [cos(om x~); sin(om x~)], so that Phi_A^T Phi_B = feature_kernel."""
    T = om @ ((X - 0.5) / ell[:, None])
    return np.sqrt(a / om.shape[0]) * np.vstack([np.cos(T), np.sin(T)])


def kernel_c(XA, XB, theta, kernel):
    """k and the derivative weight c (dk/dx_d = -c (x_d - x'_d) / l_d^2), P x Q each."""
    ell = np.asarray(theta[1:])[:, None]
    A, B = XA / ell, XB / ell
    q = np.maximum(np.sum(A * A, 0)[:, None] + np.sum(B * B, 0)[None, :] - 2.0 * A.T @ B, 0.0)
    a = theta[0]
    if kernel == SE:
        k = a * np.exp(-0.5 * q)
        return k, k
    s = np.sqrt(5.0 * q)
    e = np.exp(-s)
    return a * (1.0 + s + (5.0 / 3.0) * q) * e, a * (5.0 / 3.0) * (1.0 + s) * e


def pathwise_cov(Pss, PsX, PXX, Ks, Ky, b):
    """Covariance of a pathwise draw at the query points for a FIXED feature set, over w, w' and eps:
    Phi*^T Phi* - Phi*^T Phi_X K_y^-1 K* - K*^T K_y^-1 Phi_X^T Phi* + K*^T K_y^-1 (Phi_X^T Phi_X + b I) K_y^-1 K*,
    given the feature Gram blocks Pss = Phi*^T Phi*, PsX = Phi*^T Phi_X, PXX = Phi_X^T Phi_X, K* = k(X, Xs) (N x M), K_y."""
    A = np.linalg.solve(Ky, Ks)                      # K_y^-1 K*
    N = Ky.shape[0]
    return Pss - PsX @ A - A.T @ PsX.T + A.T @ (PXX + b * np.eye(N)) @ A


class PathRef:
    """The n_draws draws of an object made from (X, y, theta, b, kernel) with F frequencies and stream `seed`."""

    def __init__(self, X, y, theta, b, kernel, n_draws, F, seed, gen=normals):
        self.X, self.y, self.theta, self.b, self.kernel = np.asarray(X, float), np.asarray(y, float), np.asarray(theta, float), b, kernel
        self.D, self.N = self.X.shape
        self.a, self.ell = self.theta[0], self.theta[1:]
        self.F, self.n_draws = F, n_draws
        self.om = frequencies(seed, self.D, F, kernel, gen)
        w, wp, self.eps = draw_normals(seed, self.D, self.N, F, kernel, n_draws, gen)
        self.W = np.sqrt(self.a / F) * np.vstack([w, wp])          # 2F x n_draws
        Ky = pr.ard_kernel(self.X, self.X, self.theta, kernel) + b * np.eye(self.N)
        self.Ky = Ky
        r = self.y[:, None] - self.prior_all(self.X) - np.sqrt(b) * self.eps
        self.v = np.linalg.solve(Ky, r)                             # N x n_draws

    def prior_all(self, Xs):
        T = self.om @ ((Xs - 0.5) / self.ell[:, None])              # F x M
        return np.cos(T).T @ self.W[:self.F] + np.sin(T).T @ self.W[self.F:]

    def eval_all(self, Xs):
        """M x n_draws."""
        Xs = np.asarray(Xs, float)
        return self.prior_all(Xs) + pr.ard_kernel(Xs, self.X, self.theta, self.kernel) @ self.v

    def eval(self, Xs, draws):
        """(val (M,), grad (D x M)) of f_{draws[m]} at Xs[:, m]."""
        Xs = np.asarray(Xs, float)
        draws = np.asarray(draws)
        T = self.om @ ((Xs - 0.5) / self.ell[:, None])              # F x M
        wc, ws = self.W[:self.F, draws], self.W[self.F:, draws]     # F x M
        val = np.sum(wc * np.cos(T) + ws * np.sin(T), axis=0)
        g = ws * np.cos(T) - wc * np.sin(T)                         # F x M
        grad = (self.om.T @ g) / self.ell[:, None]
        k, c = kernel_c(Xs, self.X, self.theta, self.kernel)        # M x N
        vm = self.v[:, draws].T                                     # M x N
        val = val + np.sum(k * vm, axis=1)
        cv = c * vm
        l2 = (self.ell ** 2)[:, None]
        grad = grad - (Xs * cv.sum(axis=1)[None, :] - self.X @ cv.T) / l2
        return val, grad

    def data_identity(self, rows=None):
        """y_i - sqrt(b) eps_{s,i} - b v_{s,i} for the training rows `rows` (all by default), rows x n_draws: what f_s(x_i) equals,
        since K v_s = r_s - b v_s and r_s = y - f_prior,s(X) - sqrt(b) eps_s."""
        rows = slice(None) if rows is None else rows
        return self.y[rows, None] - np.sqrt(self.b) * self.eps[rows] - self.b * self.v[rows]
