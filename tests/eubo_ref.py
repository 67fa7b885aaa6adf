"""numpy / scipy restatement of the expected utility of the best option of a query pair as include/sls_hip.h states it ("expected
utility of the best option"): EUBO(x, x') = E[max(f(x), f(x'))] with its gradient in both options and the guard, from the data
through a Cholesky solve."""
import numpy as np
import scipy.linalg as sla
from scipy.special import erfc

SE, MATERN52 = 0, 1
RSQRT2 = 1.0 / np.sqrt(2.0)
RSQRT_2PI = 1.0 / np.sqrt(2.0 * np.pi)


def kernel_kc(kernel, a, q):
    """k and the derivative weight c (dk/dx_d = -c (x~_d - x~'_d) inv_ell_d) of the scaled squared distance q."""
    if kernel == SE:
        k = a * np.exp(-0.5 * q)
        return k, k
    s = np.sqrt(5.0 * q)
    e = np.exp(-s)
    return a * (1.0 + s + (5.0 / 3.0) * q) * e, a * (5.0 / 3.0) * (1.0 + s) * e


def scaled_sqdist(A, B):
    """q[i, j] = |A[:, i] - B[:, j]|^2 from the differences themselves (no cancellation for close points)."""
    q = np.zeros((A.shape[1], B.shape[1]))
    for d in range(A.shape[0]):
        df = A[d][:, None] - B[d][None, :]
        q += df * df
    return q


def closed_form(mu, s2, dmu, ds2):
    """The pair's value and gradient from its posterior: mu (2, M), s2 = Var[f(x) - f(x')] (M,), dmu and ds2 (2, D, M) the gradients
    of mu_o and of s2 in option o.  Returns (val (M,), grad (2D, M), s, u, Phi (2, M), phi, bad), the guard applied."""
    with np.errstate(all="ignore"):
        s = np.sqrt(s2)
        u = (mu[0] - mu[1]) / s
        Phi = np.stack([0.5 * erfc(-u * RSQRT2), 0.5 * erfc(u * RSQRT2)])
        phi = np.exp(-0.5 * u * u) * RSQRT_2PI
        val = (mu[0] * Phi[0] + mu[1] * Phi[1]) + s * phi
        grad = np.concatenate([Phi[o][None, :] * dmu[o] + (phi / (2.0 * s))[None, :] * ds2[o] for o in range(2)], axis=0)
        bad = ~(s2 > 0.0) | (s < 1e-10) | np.isnan(val) | np.isnan(grad).any(axis=0)
        val = np.where(bad, np.fmax(mu[0], mu[1]), val)
        grad = np.where(bad[None, :], 0.0, grad)
    return val, grad, s, u, Phi, phi, bad


def eubo(X, y, theta, b, kernel, pairs, s2=None):
    """X (D, N), y (N,), theta = (a, l_1..l_D), noise b, pairs (2D, M): rows 0..D-1 = x, D..2D-1 = x'.
    Returns (val (M,), grad (2D, M), info).  s2 (M,), if given, replaces the reference's own Var[f(x) - f(x')] (the value and the
    factors Phi, phi follow it; the gradient keeps the reference's own ds^2).  info: mu, s2, s, u, Phi (2, M), phi, dmu (2, D, M),
    ds2 (2, D, M), cond (of K_y), alpha, bad -- what the tests' tolerances are formed from."""
    X, y, theta, pairs = (np.asarray(v, dtype=np.float64) for v in (X, y, theta, pairs))
    D, N = X.shape
    M = pairs.shape[1]
    a, il = theta[0], 1.0 / theta[1:]
    Xt = (X - 0.5) * il[:, None]
    q = scaled_sqdist(Xt, Xt)
    Ky = kernel_kc(kernel, a, q)[0] + b * np.eye(N)
    L = np.linalg.cholesky(Ky)
    alpha = sla.cho_solve((L, True), y)
    ev = np.linalg.eigvalsh(Ky)
    with np.errstate(all="ignore"):
        xt = [(pairs[:D] - 0.5) * il[:, None], (pairs[D:] - 0.5) * il[:, None]]
        kc = [kernel_kc(kernel, a, scaled_sqdist(Xt, xt[o])) for o in range(2)]          # (k, c), each N x M
        dvec = kc[0][0] - kc[1][0]
        finite = np.isfinite(dvec).all(axis=0)
        w = np.full((N, M), np.nan)
        if finite.any():
            w[:, finite] = sla.cho_solve((L, True), dvec[:, finite])
        mu = np.stack([kc[o][0].T @ alpha for o in range(2)])
        q12 = np.sum((xt[0] - xt[1]) ** 2, axis=0)
        k12, c12 = kernel_kc(kernel, a, q12)
        own_s2 = (2.0 * a - 2.0 * k12) - np.sum(dvec * w, axis=0)
        s2v = own_s2 if s2 is None else np.asarray(s2, dtype=np.float64)
        e = c12[None, :] * (xt[0] - xt[1]) * il[:, None]
        dmu, ds2 = [], []
        for o in range(2):
            c = kc[o][1]
            ca = c.T @ alpha
            dmu.append(-il[:, None] * (xt[o] * ca[None, :] - (Xt * alpha[None, :]) @ c))
            cw = np.sum(c * w, axis=0)
            T = il[:, None] * (xt[o] * cw[None, :] - Xt @ (c * w))
            ds2.append((2.0 if o == 0 else -2.0) * (e + T))
        dmu, ds2 = np.stack(dmu), np.stack(ds2)
        val, grad, s, u, Phi, phi, bad = closed_form(mu, s2v, dmu, ds2)
    return val, grad, dict(mu=mu, s2=s2v, own_s2=own_s2, s=s, u=u, Phi=Phi, phi=phi, dmu=dmu, ds2=ds2, cond=ev[-1] / ev[0],
                           alpha=alpha, bad=bad)
