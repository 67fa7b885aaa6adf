"""numpy restatement of the Laplace posterior for preference data (include/sls_hip.h "Laplace posterior"; tests/test_laplace_cpu.py,
tests/test_gpu_laplace.py, tests/test_gpu_laplace_host.py).

With K_y = K_f + b I = L L^T, alpha = K_y^-1 y, tuples (first index = the chosen point) and s = btl_scale:
  per tuple:  p = softmax(y_i / s) with the maximum subtracted,  H = (diag(p) - p p^T) / s^2
  W        = scatter-sum of every H at (i_j, i_k); a repeated index adds
  B        = I + L^T W L,   Sigma_g = (K_y^-1 + W)^-1 = L B^-1 L^T
  T        = B^-1 (L^T W L)   (product form),   M = L^-T T L^-1
  sigma^2  = max(0, a - k*^T M k*),   grad sigma = -(1 / sigma) J M k*,   cov = K(Xs, Xs) - V^T T V,  V = L^-1 K*
  log_lik  = sum_t log p_t0,   log Z = log_lik - 1/2 y^T alpha - 1/2 log|B|
  path     r_s = y + L L_B^-T z_s - sqrt(b) eps_s - f_prior,s(X);  draw s takes 2F + 2N normal numbers from B0 + s (2F + 2N): w, w', eps, z."""
import numpy as np
import scipy.linalg as sla

import path_ref as ph
import posterior_ref as pr

SE, MATERN52 = pr.SE, pr.MATERN52


def example_prefs(N, rng):
    """Tuples of 2-4 options over the points 0 .. N - 2 (point N - 1 is in none: a zero row of W); point 0 is in twelve; one tuple twice."""
    prefs = [tuple(int(i) for i in rng.choice(N - 1, size=int(rng.integers(2, 5)), replace=False)) for _ in range((2 * N) // 3)]
    for k in range(12):
        other = rng.choice(np.arange(1, N - 1), size=int(rng.integers(1, 4)), replace=False)
        tup = [int(i) for i in other]
        tup.insert(k % len(tup), 0)
        prefs.append(tuple(tup))
    prefs.append(prefs[3])
    assert sum(0 in p for p in prefs) >= 10 and not any(N - 1 in p for p in prefs)
    return prefs


def tuple_probs(y, tup, s):
    v = np.asarray(y, float)[list(tup)] / s
    v = v - v.max()
    e = np.exp(v)
    return e / e.sum(), v[0] - np.log(e.sum())


def w_matrix(prefs, y, s, N):
    """(W, log_lik)."""
    W = np.zeros((N, N))
    ll = 0.0
    for tup in prefs:
        p, lp0 = tuple_probs(y, tup, s)
        H = (np.diag(p) - np.outer(p, p)) / (s * s)
        idx = np.asarray(list(tup))
        np.add.at(W, (idx[:, None], idx[None, :]), H)
        ll += lp0
    return W, ll


def loglik_grad(prefs, y, s, N):
    """d log_lik / dy."""
    g = np.zeros(N)
    for tup in prefs:
        p, _ = tuple_probs(y, tup, s)
        idx = np.asarray(list(tup))
        e0 = np.zeros(len(idx))
        e0[0] = 1.0
        np.add.at(g, idx, (e0 - p) / s)
    return g


def newton_map(X, theta, b, kernel, prefs, s, iters=200, tol=1e-12):
    """The mode of log_lik(y) - 1/2 y^T K_y^-1 y by damped Newton steps (GPML algorithm 3.1's fixed point, with backtracking)."""
    N = X.shape[1]
    Ky = pr.ard_kernel(X, X, theta, kernel) + b * np.eye(N)
    Kinv = np.linalg.inv(Ky)
    y = np.zeros(N)

    def obj(v):
        return w_matrix(prefs, v, s, N)[1] - 0.5 * v @ Kinv @ v
    f = obj(y)
    for _ in range(iters):
        W, _ = w_matrix(prefs, y, s, N)
        g = loglik_grad(prefs, y, s, N) - Kinv @ y
        step = np.linalg.solve(Kinv + W, g)
        t = 1.0
        while t > 1e-10:
            f1 = obj(y + t * step)
            if f1 >= f + 1e-4 * t * (g @ step):
                break
            t *= 0.5
        y = y + t * step
        done = abs(f1 - f) <= tol * max(1.0, abs(f))
        f = f1
        if done:
            break
    return y


class LaplaceRef:
    def __init__(self, X, y, theta, b, kernel, prefs, s):
        self.X, self.y, self.theta, self.b, self.kernel = np.asarray(X, float), np.asarray(y, float), np.asarray(theta, float), b, kernel
        self.prefs, self.s = [tuple(int(i) for i in p) for p in prefs], s
        self.D, self.N = self.X.shape
        N = self.N
        self.a, self.ell = self.theta[0], self.theta[1:]
        self.Ky = pr.ard_kernel(self.X, self.X, self.theta, kernel) + b * np.eye(N)
        self.L = np.linalg.cholesky(self.Ky)
        self.alpha = sla.cho_solve((self.L, True), self.y)
        self.W, self.log_lik = w_matrix(self.prefs, self.y, s, N)
        A = self.L.T @ self.W @ self.L
        A = 0.5 * (A + A.T)
        self.B = np.eye(N) + A
        self.LB = np.linalg.cholesky(self.B)
        self.Binv = sla.cho_solve((self.LB, True), np.eye(N))
        T = self.Binv @ A                                           # the product form: no I - B^-1
        self.T = 0.5 * (T + T.T)
        G = self.Binv @ (self.L.T @ self.W)                         # T L^-1
        M = sla.solve_triangular(self.L, G, lower=True, trans="T")  # L^-T G
        self.M = 0.5 * (M + M.T)
        S = self.L @ self.Binv @ self.L.T
        self.cov_g = 0.5 * (S + S.T)
        self.logdet_B = 2.0 * np.sum(np.log(np.diag(self.LB)))
        self.log_evidence = self.log_lik - 0.5 * self.y @ self.alpha - 0.5 * self.logdet_B
        self.mu_best = float(np.max(self.y - b * self.alpha))       # PredictMaximumPointFromData: mu at the data points

    def ks(self, Xs):
        return pr.ard_kernel(self.X, np.asarray(Xs, float), self.theta, self.kernel)      # N x M

    def predict(self, Xs):
        K = self.ks(Xs)
        return K.T @ self.alpha, np.sqrt(np.maximum(self.a - np.sum(K * (self.M @ K), axis=0), 0.0))

    def sigma_forms(self, Xs):
        """sigma^2 three ways: the product form; the subtractive form with K_y^-1 - K_y^-1 Sigma_g K_y^-1; (a - |v|^2) + v^T B^-1 v."""
        K = self.ks(Xs)
        prod = self.a - np.sum(K * (self.M @ K), axis=0)
        Kinv = sla.cho_solve((self.L, True), np.eye(self.N))
        sub = self.a - np.sum(K * ((Kinv - Kinv @ self.cov_g @ Kinv) @ K), axis=0)
        V = sla.solve_triangular(self.L, K, lower=True)
        third = (self.a - np.sum(V * V, axis=0)) + np.sum(V * (self.Binv @ V), axis=0)
        return prod, sub, third

    def plain_sigma(self, Xs):
        K = self.ks(Xs)
        V = sla.solve_triangular(self.L, K, lower=True)
        return np.sqrt(np.maximum(self.a - np.sum(V * V, axis=0), 0.0))

    def predict_grad(self, Xs):
        """(dmu, dsigma), D x M each."""
        Xs = np.asarray(Xs, float)
        k, c = ph.kernel_c(Xs, self.X, self.theta, self.kernel)      # M x N
        l2 = (self.ell ** 2)[:, None]

        def contract(w):                                             # sum_i dk(x, x_i)/dx w_i, w: M x N
            cw = c * w
            return -(Xs * cw.sum(axis=1)[None, :] - self.X @ cw.T) / l2
        dmu = contract(np.broadcast_to(self.alpha[None, :], k.shape))
        _, sg = self.predict(Xs)
        dsg = -contract(k @ self.M) / sg[None, :]
        return dmu, dsg

    def cov(self, Xs):
        Xs = np.asarray(Xs, float)
        V = sla.solve_triangular(self.L, self.ks(Xs), lower=True)
        return pr.ard_kernel(Xs, Xs, self.theta, self.kernel) - V.T @ self.T @ V

    def acq(self, Xs, acq, ucb_h=1.0):
        """Expected improvement (0) / GP-UCB (1) with the Laplace sigma (src/acquisition-function.cpp:170-196)."""
        from scipy.special import erfc
        mu, sg = self.predict(Xs)
        if acq == 1:
            return mu + ucb_h * sg
        d = mu - self.mu_best
        with np.errstate(divide="ignore", invalid="ignore"):
            u = d / sg
            v = d * 0.5 * erfc(-u / np.sqrt(2.0)) + sg * np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)
        return np.where(sg < 1e-10, 0.0, v)


class LaplacePathRef(ph.PathRef):
    """path_ref.PathRef on a Laplace handle: draw s takes 2F + 2N numbers (w, w', eps, z) and the right-hand side carries the sampled
    deviation of the goodness values L L_B^-T z_s."""

    def __init__(self, lap, n_draws, F, seed, gen=ph.normals):
        self.X, self.y, self.theta, self.b, self.kernel = lap.X, lap.y, lap.theta, lap.b, lap.kernel
        self.D, self.N = self.X.shape
        self.a, self.ell = lap.a, lap.ell
        self.F, self.n_draws = F, n_draws
        N = self.N
        self.om = ph.frequencies(seed, self.D, F, self.kernel, gen)
        B0 = ph.block0(self.D, F, self.kernel)
        E = gen(seed, B0, n_draws * (2 * F + 2 * N)).reshape(n_draws, 2 * F + 2 * N).T
        w, wp, self.eps, self.z = E[:F], E[F:2 * F], E[2 * F:2 * F + N], E[2 * F + N:]
        self.W = np.sqrt(self.a / F) * np.vstack([w, wp])
        self.Ky = lap.Ky
        self.dy = lap.L @ sla.solve_triangular(lap.LB, self.z, lower=True, trans="T")      # L L_B^-T z
        r = (self.y[:, None] + self.dy) - np.sqrt(self.b) * self.eps - self.prior_all(self.X)
        self.v = sla.cho_solve((lap.L, True), r)
