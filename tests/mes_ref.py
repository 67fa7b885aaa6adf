"""numpy / scipy restatement of max-value entropy search as include/sls_hip.h states it ("max-value entropy search"): the scalar
terms g, g' and alpha with its gradient from given mu, sigma, dmu, dsigma and a sample y_star of the maximum value."""
import numpy as np
from scipy.special import erfc, erfcx

RSQRT2 = 1.0 / np.sqrt(2.0)
SERIES_BELOW = -30.0


def terms(t):
    """(g(t), g'(t)): g = 1/2 t r - log Phi, g' = -1/2 r (1 + t (t + r)), r = phi / Phi; no Phi that can underflow."""
    t = np.asarray(t, dtype=np.float64)
    neg = t < 0
    with np.errstate(all="ignore"):
        tn = np.where(neg, t, -1.0)             # each branch on arguments of its own side only
        tp = np.where(neg, 1.0, t)
        e = erfcx(-tn * RSQRT2)
        r_n = np.sqrt(2.0 / np.pi) / e
        lp_n = np.log(0.5 * e) - 0.5 * tn * tn
        r_p = np.exp(-0.5 * tp * tp) / np.sqrt(2.0 * np.pi) / (0.5 * erfc(-tp * RSQRT2))
        lp_p = np.log1p(-0.5 * erfc(tp * RSQRT2))
        r = np.where(neg, r_n, r_p)
        log_Phi = np.where(neg, lp_n, lp_p)
        c = 1.0 + t * (t + r)
        u = 1.0 / (t * t)
        series = u * (2.0 + u * (-10.0 + u * (74.0 + u * (-706.0 + u * 8162.0))))
        c = np.where(t < SERIES_BELOW, series, c)
        return 0.5 * t * r - log_Phi, -0.5 * r * c


def g(t):
    return terms(t)[0]


def dg(t):
    return terms(t)[1]


def alpha(mu, sigma, y_star, dmu=None, dsigma=None):
    """mu, sigma (M,), y_star (K,), dmu, dsigma (D, M) or None: (alpha (M,), grad (D, M) or None, info).  Sums over k in increasing
    k; the guard of expected improvement: sigma < 1e-10 or a NaN in the value or any gradient component -> value 0, gradient 0.
    info: gamma (K, M), A1, A2 (M,) -- what the tests' tolerances are formed from."""
    mu, sigma, y_star = (np.asarray(v, dtype=np.float64) for v in (mu, sigma, y_star))
    K = y_star.size
    with np.errstate(all="ignore"):
        gamma = (y_star[:, None] - mu[None, :]) / sigma[None, :]
        gv, dv = terms(gamma)
        A0, A1, A2 = np.zeros_like(mu), np.zeros_like(mu), np.zeros_like(mu)
        for k in range(K):
            A0 = A0 + gv[k]
            A1 = A1 + dv[k]
            A2 = A2 + gamma[k] * dv[k]
        A0, A1, A2 = A0 * (1.0 / K), A1 * (1.0 / K), A2 * (1.0 / K)
        bad = (sigma < 1e-10) | np.isnan(A0)
        grad = None
        if dmu is not None:
            grad = -(1.0 / sigma)[None, :] * (A1[None, :] * np.asarray(dmu) + A2[None, :] * np.asarray(dsigma))
            bad = bad | np.isnan(grad).any(axis=0)
            grad = np.where(bad[None, :], 0.0, grad)
        val = np.where(bad, 0.0, A0)
    return val, grad, dict(gamma=gamma, A1=A1, A2=A2, bad=bad)
