"""numpy / scipy restatement of joint entropy search as include/sls_hip.h states it ("joint entropy search"): the scalar terms tau,
tau' of the truncated normal, the conditioned optima, and alpha with its gradient from given mu, sigma, c_k and their gradients; the
whole pipeline from a fit of tests/gram_ref.py; and the same formulas in mpmath (60 digits) from float64 inputs."""
import mpmath as mp
import numpy as np
from scipy.special import erfc, erfcx

import gram_ref

RSQRT2 = 1.0 / np.sqrt(2.0)
SERIES_BELOW = -30.0
V_FLOOR = S2_FLOOR = 1e-20


def terms(t):
    """(tau(t), tau'(t)): tau = 1 - r (t + r), tau' = r ((t + r)(t + 2 r) - 1), r = phi / Phi, in the forms of the contract: t < 0:
    w = r + t, c = 1 + t w (series and w = (c - 1) / t below -30), tau = c - w^2; t >= 0: tau = 1 - r w; tau' = r (w^2 - tau)."""
    t = np.asarray(t, dtype=np.float64)
    neg = t < 0
    with np.errstate(all="ignore"):
        tn = np.where(neg, t, -1.0)             # each branch on arguments of its own side only
        tp = np.where(neg, 1.0, t)
        r_n = np.sqrt(2.0 / np.pi) / erfcx(-tn * RSQRT2)
        w_n = r_n + tn
        c = 1.0 + tn * w_n
        u = 1.0 / (tn * tn)
        series = u * (2.0 + u * (-10.0 + u * (74.0 + u * (-706.0 + u * 8162.0))))
        far = tn < SERIES_BELOW
        c = np.where(far, series, c)
        w_n = np.where(far, (c - 1.0) / tn, w_n)
        tau_n = c - w_n * w_n
        r_p = np.exp(-0.5 * tp * tp) / np.sqrt(2.0 * np.pi) / (0.5 * erfc(-tp * RSQRT2))
        w_p = r_p + tp
        tau_p = 1.0 - r_p * w_p
        r, w, tau = np.where(neg, r_n, r_p), np.where(neg, w_n, w_p), np.where(neg, tau_n, tau_p)
        return tau, r * (w * w - tau)


def terms_mp(t, dps=60):
    """(tau, tau') of one float t as mpmath numbers, from the definition."""
    with mp.workdps(dps):
        t = mp.mpf(float(t))
        r = mp.npdf(t) / mp.ncdf(t)
        return 1 - r * (t + r), r * ((t + r) * (t + 2 * r) - 1)


def alpha(mu, sigma, cov, f_star, d, v, noise_var, dmu=None, dsigma=None, dcov=None):
    """mu, sigma (M,), cov (M, K), f_star, d, v (K,), dmu, dsigma (D, M), dcov (D, M, K) or None:
    (alpha (M,), grad (D, M) or None, info).  Sums over k in increasing k; c / v is formed as c (1 / v).  info: gamma, s2, q, H (K, M),
    A_mu, A_sigma (M,), bad -- what the tests' tolerances are formed from."""
    mu, sigma, cov, f_star, d, v = (np.asarray(a, dtype=np.float64) for a in (mu, sigma, cov, f_star, d, v))
    M, K = cov.shape
    with np.errstate(all="ignore"):
        inv_v = np.where(v < V_FLOOR, 0.0, 1.0 / v)
        s2 = sigma * sigma
        hk = -0.5 / K
        S0, Sm, Ss = np.zeros(M), np.zeros(M), np.zeros(M)
        H, gamma, sk2s, qs = np.zeros((K, M)), np.zeros((K, M)), np.zeros((K, M)), np.zeros((K, M))
        for k in range(K):
            c = cov[:, k]
            ratio = c * inv_v[k]
            mk = mu + ratio * d[k]
            sk2 = s2 - c * ratio
            dead = sk2 < S2_FLOOR
            sk = np.sqrt(np.where(dead, 1.0, sk2))
            gam = (f_star[k] - mk) / sk
            tau, dtau = terms(gam)
            q = noise_var + sk2 * tau
            inv_q = 1.0 / q
            S0 = S0 + np.where(dead, np.log(noise_var), np.log(q))
            Sm = Sm + np.where(dead, 0.0, (-sk * dtau) * inv_q)
            Ss = Ss + np.where(dead, 0.0, (2.0 * sigma * tau - gam * sigma * dtau) * inv_q)
            H[k] = np.where(dead, 0.0, hk * ((-2.0 * ratio * tau + dtau * (gam * ratio - sk * d[k] * inv_v[k])) * inv_q))
            gamma[k], sk2s[k], qs[k] = np.where(dead, np.nan, gam), sk2, np.where(dead, noise_var, q)
        tot = s2 + noise_var
        val = 0.5 * np.log(tot) + hk * S0
        A_mu, A_sg = hk * Sm, sigma / tot + hk * Ss
        bad = (sigma < 1e-10) | np.isnan(val)
        grad = None
        if dmu is not None:
            grad = A_mu[None, :] * np.asarray(dmu) + A_sg[None, :] * np.asarray(dsigma)
            dcov = np.asarray(dcov)
            for k in range(K):
                grad = grad + H[k][None, :] * dcov[:, :, k]
            bad = bad | np.isnan(grad).any(axis=0)
            grad = np.where(bad[None, :], 0.0, grad)
        val = np.where(bad, 0.0, val)
    return val, grad, dict(gamma=gamma, s2=sk2s, q=qs, H=H, A_mu=A_mu, A_sigma=A_sg, bad=bad)


def alpha_mp(mu, sigma, cov, f_star, d, v, noise_var, dmu=None, dsigma=None, dcov=None, dps=50):
    """The same formula (without the guard) in mpmath from the same float64 inputs, one point at a time: (alpha (M,), grad (D, M))
    rounded to float64.  The reference the float64 evaluations are measured against."""
    M, K = np.shape(cov)
    val, grad = np.zeros(M), None if dmu is None else np.zeros(np.shape(dmu))
    with mp.workdps(dps):
        nv = mp.mpf(float(noise_var))
        for m in range(M):
            mu_m, sg = mp.mpf(float(mu[m])), mp.mpf(float(sigma[m]))
            s2 = sg * sg
            S0 = Sm = Ss = mp.mpf(0)
            h = [mp.mpf(0)] * K
            for k in range(K):
                c, vk, dk = mp.mpf(float(cov[m, k])), mp.mpf(float(v[k])), mp.mpf(float(d[k]))
                ratio = mp.mpf(0) if float(v[k]) < V_FLOOR else c / vk
                ivd = mp.mpf(0) if float(v[k]) < V_FLOOR else dk / vk
                sk2 = s2 - c * ratio
                if sk2 < S2_FLOOR:
                    S0 += mp.log(nv)
                    continue
                sk = mp.sqrt(sk2)
                gam = (mp.mpf(float(f_star[k])) - (mu_m + ratio * dk)) / sk
                tau, dtau = terms_mp(gam, dps)
                q = nv + sk2 * tau
                S0 += mp.log(q)
                Sm += -sk * dtau / q
                Ss += (2 * sg * tau - gam * sg * dtau) / q
                h[k] = -(-2 * ratio * tau + dtau * (gam * ratio - sk * ivd)) / q / (2 * K)
            val[m] = float(mp.log(s2 + nv) / 2 - S0 / (2 * K))
            if grad is not None:
                A_mu, A_sg = -Sm / (2 * K), sg / (s2 + nv) - Ss / (2 * K)
                for dd in range(grad.shape[0]):
                    g = A_mu * mp.mpf(float(dmu[dd, m])) + A_sg * mp.mpf(float(dsigma[dd, m]))
                    for k in range(K):
                        g += h[k] * mp.mpf(float(dcov[dd, m, k]))
                    grad[dd, m] = float(g)
    return val, grad


def condition(f, x_star, f_star, star_noise):
    """The per-optimum quantities of a gram_ref.fit: x* clamped into the box, mu*, v, d and W = K_y^-1 k(X, x*) (N x K)."""
    xs = np.clip(np.asarray(x_star, dtype=np.float64), 0.0, 1.0)
    p = gram_ref.predict(f, xs)
    Kx = gram_ref.gram_cross(f["X"], xs, f["ell"], f["a"], f["kernel"])
    W = f["Kinv"] @ Kx
    sg = p["dev"]
    return dict(xs=xs, mu_star=p["mean"], v=sg * sg + star_noise, d=np.asarray(f_star, dtype=np.float64) - p["mean"], W=W,
                f_star=np.asarray(f_star, dtype=np.float64))


def covariances(f, o, Xs, want_grad=False):
    """c_k(x_m) (M, K) and, with want_grad, its gradient in x (D, M, K)."""
    Xs = np.asarray(Xs, dtype=np.float64)
    ell = np.asarray(f["ell"])
    Ks, Cs = gram_ref.kern(gram_ref.sqdist(f["X"], Xs, ell), f["a"], f["kernel"])             # N x M
    kx, cx = gram_ref.kern(gram_ref.sqdist(Xs, o["xs"], ell), f["a"], f["kernel"])            # M x K
    cov = kx - Ks.T @ o["W"]
    if not want_grad:
        return cov
    D, M = Xs.shape
    dcov = np.empty((D, M, o["W"].shape[1]))
    for dd in range(D):
        Jd = -Cs * (Xs[dd][None, :] - f["X"][dd][:, None]) / (ell[dd] * ell[dd])              # N x M: dk(x, X_i) / dx_d
        Jo = -cx * (Xs[dd][:, None] - o["xs"][dd][None, :]) / (ell[dd] * ell[dd])             # M x K: dk(x, x*_k) / dx_d
        dcov[dd] = Jo - Jd.T @ o["W"]
    return cov, dcov


def evaluate(f, o, Xs, noise_var, want_grad=True):
    """alpha (and its gradient) at the columns of Xs from a fit and its conditioned optima: (val, grad, info)."""
    p = gram_ref.predict(f, Xs, want_grad=want_grad)
    if want_grad:
        cov, dcov = covariances(f, o, Xs, True)
        return alpha(p["mean"], p["dev"], cov, o["f_star"], o["d"], o["v"], noise_var, p["dmean"], p["ddev"], dcov)
    return alpha(p["mean"], p["dev"], covariances(f, o, Xs), o["f_star"], o["d"], o["v"], noise_var)


def covariance_bounds(f, o, Xs, cond):
    """What an evaluation in another summation order may differ by from covariances(): (tol_cov (M, K), tol_dcov (D, M, K)).
    w_k = K_y^-1 k(X, x*_k) carries cond(K_y) eps |w_k| (norm-wise) whichever way it is solved, a dot product over N terms N eps of the
    sum of its terms' magnitudes, a kernel value 4 (D + 8) eps a (gram_ref.gram_tolerance)."""
    eps = np.finfo(np.float64).eps
    Xs = np.asarray(Xs, dtype=np.float64)
    ell = np.asarray(f["ell"])
    D, M = Xs.shape
    N = f["X"].shape[1]
    Ks, Cs = gram_ref.kern(gram_ref.sqdist(f["X"], Xs, ell), f["a"], f["kernel"])
    kx, cx = gram_ref.kern(gram_ref.sqdist(Xs, o["xs"], ell), f["a"], f["kernel"])
    W = o["W"]
    wn = np.linalg.norm(W, axis=0)
    base = gram_ref.gram_tolerance(D, f["a"])
    tol_cov = base + 8 * cond * eps * np.linalg.norm(Ks, axis=0)[:, None] * wn[None, :] + 2 * N * eps * (np.abs(Ks).T @ np.abs(W))
    tol_d = np.empty((D, M, W.shape[1]))
    for dd in range(D):
        Jd = np.abs(Cs * (Xs[dd][None, :] - f["X"][dd][:, None])) / (ell[dd] * ell[dd])
        Jo = np.abs(cx * (Xs[dd][:, None] - o["xs"][dd][None, :])) / (ell[dd] * ell[dd])
        tol_d[dd] = (base / ell[dd] + 8 * (D + 8) * eps * Jo + 8 * cond * eps * np.linalg.norm(Jd, axis=0)[:, None] * wn[None, :] +
                     2 * N * eps * (Jd.T @ np.abs(W)))
    return tol_cov, tol_d


def fit(X, y, ell, a, b, kernel):
    """gram_ref.fit's record with LAPACK's factorisation (the larger shapes of the device tests)."""
    from scipy.linalg import solve_triangular
    X, y, ell = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(ell, dtype=np.float64)
    q = gram_ref.sqdist(X, X, ell)
    K = gram_ref.gram(X, ell, a, b, kernel, q=q)
    L = np.linalg.cholesky(K)
    Li = solve_triangular(L, np.eye(K.shape[0]), lower=True)
    return dict(X=X, y=y, ell=ell, a=a, b=b, kernel=kernel, dtype=np.float64, expansion=False, q=q, K=K, Li=Li, Kinv=Li.T @ Li,
                alpha=Li.T @ (Li @ y), logdet=2.0 * np.log(np.diag(L)).sum())
