"""numpy / scipy restatement of log expected improvement as include/sls_hip.h states it ("log expected improvement"): the scalar
terms log h, B1 = Phi / h, B2 = phi / h of h(u) = phi(u) + u Phi(u), and LogEI with its gradient from given mu, sigma, mu_best, dmu,
dsigma."""
import numpy as np
from scipy.special import erfc, erfcx

RSQRT2 = 1.0 / np.sqrt(2.0)
SERIES_BELOW = -30.0
FLOOR = -1.0e300          # SLS_LOG_EI_FLOOR


def terms(u):
    """(log h(u), Phi / h, phi / h), h = phi + u Phi; no Phi that can underflow."""
    u = np.asarray(u, dtype=np.float64)
    neg = u < 0
    with np.errstate(all="ignore"):
        un = np.where(neg, u, -1.0)             # each branch on arguments of its own side only
        up = np.where(neg, 1.0, u)
        e = erfcx(-un * RSQRT2)
        r_n = np.sqrt(2.0 / np.pi) / e
        w_n = r_n + un
        t = 1.0 / (un * un)
        c = t * (2.0 + t * (-10.0 + t * (74.0 + t * (-706.0 + t * 8162.0))))
        w_n = np.where(un < SERIES_BELOW, (c - 1.0) / un, w_n)
        lh_n = (np.log(0.5 * e) - 0.5 * un * un) + np.log(w_n)
        phi, Phi = np.exp(-0.5 * up * up) / np.sqrt(2.0 * np.pi), 0.5 * erfc(-up * RSQRT2)
        r_p = phi / Phi
        w_p = r_p + up
        lh_p = np.log(phi + up * Phi)
        r, w = np.where(neg, r_n, r_p), np.where(neg, w_n, w_p)
        return np.where(neg, lh_n, lh_p), 1.0 / w, r / w


def logei(mu, sigma, mu_best, dmu=None, dsigma=None):
    """mu, sigma (M,), dmu, dsigma (D, M) or None: (LogEI (M,), grad (D, M) or None, info).  The guard of expected improvement: sigma <
    1e-10 or a NaN in the value or any gradient component -> value FLOOR, gradient 0.  info: u, B1, B2 (M,), bad -- what the tests'
    tolerances are formed from."""
    mu, sigma = (np.asarray(v, dtype=np.float64) for v in (mu, sigma))
    with np.errstate(all="ignore"):
        u = (mu - mu_best) / sigma
        log_h, b1, b2 = terms(u)
        v = np.log(sigma) + log_h
        bad = (sigma < 1e-10) | np.isnan(v)
        grad = None
        if dmu is not None:
            grad = (1.0 / sigma)[None, :] * (b1[None, :] * np.asarray(dmu) + b2[None, :] * np.asarray(dsigma))
            bad = bad | np.isnan(grad).any(axis=0)
            grad = np.where(bad[None, :], 0.0, grad)
        val = np.where(bad, FLOOR, v)
    return val, grad, dict(u=u, B1=b1, B2=b2, bad=bad)
