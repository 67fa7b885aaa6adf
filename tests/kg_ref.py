"""The knowledge gradient on a discrete set (include/sls_hip.h "knowledge gradient") restated in float64, operation by operation as the
device combiner forms it (sort, stack scan, envelope-order sum), and an independent mpmath reference that uses neither the sort nor the
scan: every line's interval of dominance from the pairwise crossings with the flatter and the steeper lines."""
import math

import mpmath as mp
import numpy as np

import gram_ref
import jes_ref

RSQRT2, RSQRT_2PI = 0.70710678118654752440, 0.39894228040143267794
INF = math.inf


def phi(t):
    return math.exp(-0.5 * t * t) * RSQRT_2PI


def tail(t):
    """Phi(-t)"""
    return 0.5 * math.erfc(t * RSQRT2)


def f_neg(u):
    """f(-u) = phi(u) - u Phi(-u), u >= 0"""
    return 0.0 if math.isinf(u) else phi(u) - u * tail(u)


def mass(lo, hi):
    """Phi(hi) - Phi(lo) as a difference of the smaller tails"""
    if hi <= 0.0:
        return tail(-hi) - tail(-lo)
    if lo >= 0.0:
        return tail(lo) - tail(hi)
    return (1.0 - tail(-lo)) - tail(hi)


def envelope(a, b):
    """Frazier's algorithm: (indices of the envelope lines in slope order, their breakpoints t_0 = -inf, t_1, ..)."""
    n = len(a)
    order = sorted(range(n), key=lambda j: (b[j], -a[j], j))
    env, ts = [order[0]], [-INF]
    last_b = b[order[0]]
    for j in order[1:]:
        if b[j] == last_b:
            continue
        last_b = b[j]
        t = -INF
        while env:
            top = env[-1]
            t = (a[top] - a[j]) / (b[j] - b[top])
            if not t <= ts[-1]:
                break
            env.pop()
            ts.pop()
        if not env:
            t = -INF
        env.append(j)
        ts.append(t)
    return env, ts


def lines(a, b):
    """(E max_j (a_j + b_j z) - max_j a_j, beta (n), pi (n)) of one set of lines."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    n = len(a)
    env, ts = envelope(a, b)
    E = len(env)
    beta, pi = np.zeros(n), np.zeros(n)
    val = 0.0
    for i, j in enumerate(env):
        lo, hi = ts[i], ts[i + 1] if i + 1 < E else INF
        beta[j] = phi(lo) - phi(hi)
        pi[j] = mass(lo, hi)
        if i > 0:
            val += (b[j] - b[env[i - 1]]) * f_neg(abs(lo))
    return val, beta, pi


def lines_batch(a, B, a_self=None, b_self=None):
    """sls_kg_lines restated: a (K), B (M, K), own lines (M each): val (M), beta (M, K), prob (M, K), self (M, 2) or None."""
    a, B = np.asarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64)
    M, K = B.shape
    a_max = a.max()
    val, beta, prob = np.empty(M), np.empty((M, K)), np.empty((M, K))
    own = None if a_self is None else np.empty((M, 2))
    for m in range(M):
        if a_self is None:
            val[m], beta[m], prob[m] = lines(a, B[m])
        else:
            v, be, p = lines(np.append(a, a_self[m]), np.append(B[m], b_self[m]))
            val[m], beta[m], prob[m], own[m] = v + max(0.0, a_self[m] - a_max), be[:K], p[:K], (be[K], p[K])
    return val, beta, prob, own


def kg(mu, sigma, cov, a, noise_var, include_self=True, dmu=None, dsigma=None, dcov=None):
    """The combiner and the gradient from mu, sigma (M), cov (M, K), a (K) [, dmu, dsigma (D, M), dcov (D, M, K)]: (val, grad, info)."""
    mu, sigma, cov, a = (np.asarray(v, dtype=np.float64) for v in (mu, sigma, cov, a))
    M, K = cov.shape
    a_max = a.max()
    val, a_mu, a_sg, H, slope = np.empty(M), np.zeros(M), np.zeros(M), np.zeros((M, K)), np.empty((M, K))
    beta_all, pi_all = np.zeros((M, K + 1)), np.zeros((M, K + 1))
    for m in range(M):
        sg = float(sigma[m])
        s2 = sg * sg
        with np.errstate(all="ignore"):
            s = math.sqrt(s2 + noise_var)
            bk = cov[m] / s if s > 0 else np.full(K, np.nan)
        slope[m] = bk
        if np.isnan(bk).any() or np.isnan(mu[m]) or s == 0:
            val[m] = np.nan
            continue
        al, bl = list(a), list(bk)
        if include_self:
            al.append(float(mu[m]))
            bl.append(s2 / s)
        v, beta, pi = lines(al, bl)
        val[m] = v + (max(0.0, float(mu[m]) - a_max) if include_self else 0.0)
        beta_all[m, :len(beta)], pi_all[m, :len(pi)] = beta, pi
        tot = 0.0
        for k in range(K):
            tot += beta[k] * cov[m, k]
        beta_own = beta[K] if include_self else 0.0
        a_mu[m] = pi[K] if include_self else 0.0
        a_sg[m] = (beta_own * (s2 + 2.0 * noise_var) - tot) * (sg / (s * s * s))
        H[m] = beta[:K] / s
    bad = (sigma < 1e-10) | np.isnan(val)
    grad = None
    if dmu is not None:
        grad = a_mu[None, :] * dmu + a_sg[None, :] * dsigma + np.einsum("dmk,mk->dm", dcov, H)
        bad = bad | np.isnan(grad).any(axis=0)
        grad[:, bad] = 0.0
    val[bad] = 0.0
    return val, grad, dict(a_mu=a_mu, a_sigma=a_sg, H=H, slope=slope, beta=beta_all, pi=pi_all, bad=bad)


# ---- the mpmath reference: no sort, no scan ---------------------------------------------------------------------------------------
def _near_extreme(cr, largest):
    """Indices whose float64 crossing is within 1e-9 relative of the extreme one (a float64 crossing carries a few eps relative error,
    so the exact extreme is among them); infinite extremes: the entries equal to it."""
    ext = cr.max() if largest else cr.min()
    if not np.isfinite(ext):
        return np.nonzero(cr == ext)[0]
    tol = 1e-9 * max(abs(ext), 1e-300)
    return np.nonzero(cr >= ext - tol)[0] if largest else np.nonzero(cr <= ext + tol)[0]


def _ncdf(x):
    """mp.ncdf, with the tails beyond |x| = 1e6 (below 1e-200000000000) taken as 0 and 1: mp.erfc fails on huge arguments"""
    return mp.ncdf(x) if abs(x) < 1e6 else mp.mpf(0 if x < 0 else 1)


def _npdf(x):
    return mp.npdf(x) if abs(x) < 1e6 else mp.mpf(0)


def _lines_mp(a, b):
    """lines_mp in the caller's precision, beta and pi as lists of mpf."""
    am, bm = [mp.mpf(v) for v in a], [mp.mpf(v) for v in b]
    af, bf = np.array([float(v) for v in am]), np.array([float(v) for v in bm])
    n = len(am)
    zero = mp.mpf(0)
    beta, pi = [zero] * n, [zero] * n
    total = zero
    idx = np.arange(n)
    for j in range(n):
        tie = [i for i in idx[bf == bf[j]] if i != j]              # equal as float64: settled exactly
        if any(bm[i] == bm[j] and (am[i] > am[j] or (am[i] == am[j] and i < j)) for i in tie):
            continue
        flat, steep = idx[bf < bf[j]], idx[bf > bf[j]]
        flat_x, steep_x = [i for i in tie if bm[i] < bm[j]], [i for i in tie if bm[i] > bm[j]]
        with np.errstate(all="ignore"):
            cf = (af[flat] - af[j]) / (bf[j] - bf[flat])
            cs = (af[j] - af[steep]) / (bf[steep] - bf[j])
        if not flat_x and not steep_x and flat.size and steep.size:
            lo_f, hi_f = cf.max(), cs.min()
            if np.isfinite(lo_f) and np.isfinite(hi_f) and lo_f - hi_f > 1e-9 * (abs(lo_f) + abs(hi_f)) + 1e-300:
                continue                                            # clearly never the maximum
        pick_f = flat_x + ([int(i) for i in flat[_near_extreme(cf, True)]] if flat.size else [])
        pick_s = steep_x + ([int(i) for i in steep[_near_extreme(cs, False)]] if steep.size else [])
        lo = max([(am[i] - am[j]) / (bm[j] - bm[i]) for i in pick_f], default=mp.mpf("-inf"))
        hi = min([(am[j] - am[i]) / (bm[i] - bm[j]) for i in pick_s], default=mp.mpf("inf"))
        if not lo < hi:
            continue
        pi[j] = _ncdf(hi) - _ncdf(lo)
        beta[j] = _npdf(lo) - _npdf(hi)
        total += am[j] * pi[j] + bm[j] * beta[j]
    return total - max(am), beta, pi


def lines_mp(a, b, dps=50):
    """(E max - max_j a_j, beta, pi) of one set of lines at `dps` digits.  a, b: floats or mpf.  Line j owns the z interval (lo_j, hi_j),
    lo_j = the largest crossing with a flatter line, hi_j = the smallest crossing with a steeper line; among equal slopes the larger a,
    then the lower index, dominates.  E max = sum_j [a_j (Phi(hi) - Phi(lo)) + b_j (phi(lo) - phi(hi))] over lo < hi.
    The float64 crossings only choose which pairs are formed at full precision (the near-extreme ones, see _near_extreme)."""
    with mp.workdps(dps):
        v, beta, pi = _lines_mp(a, b)
        return float(v), np.array([float(x) for x in beta]), np.array([float(x) for x in pi])


def kg_mp(mu, sigma, cov, a, noise_var, include_self=True, dmu=None, dsigma=None, dcov=None, dps=50):
    """kg() at `dps` digits from the same float64 inputs, without the guard: (val (M), grad (D, M) or None)."""
    mu, sigma, cov, a = (np.asarray(v, dtype=np.float64) for v in (mu, sigma, cov, a))
    M, K = cov.shape
    val = np.empty(M)
    grad = None if dmu is None else np.empty((dmu.shape[0], M))
    with mp.workdps(dps):
        a_max = max(mp.mpf(float(v)) for v in a)
        nv = mp.mpf(float(noise_var))
        for m in range(M):
            sg, mum = mp.mpf(float(sigma[m])), mp.mpf(float(mu[m]))
            s2 = sg * sg
            s = mp.sqrt(s2 + nv)
            cm = [mp.mpf(float(v)) for v in cov[m]]
            al, bl = [mp.mpf(float(v)) for v in a], [c / s for c in cm]
            if include_self:
                al.append(mum)
                bl.append(s2 / s)
            v, beta, pi = _lines_mp(al, bl)
            val[m] = float(v + max(al) - a_max)
            if grad is not None:
                beta_own = beta[K] if include_self else mp.mpf(0)
                a_mu = pi[K] if include_self else mp.mpf(0)
                a_sg = (beta_own * (s2 + 2 * nv) - sum(beta[k] * cm[k] for k in range(K))) * sg / s ** 3
                for d in range(grad.shape[0]):
                    g = a_mu * mp.mpf(float(dmu[d, m])) + a_sg * mp.mpf(float(dsigma[d, m]))
                    for k in range(K):
                        if beta[k] != 0:
                            g += beta[k] / s * mp.mpf(float(dcov[d, m, k]))
                    grad[d, m] = float(g)
    return val, grad


# ---- the whole criterion from a float64 fit (tests/jes_ref.py's records) ------------------------------------------------------------
def points(f, x_ref):
    """The fixed points of a gram_ref / jes_ref fit: clamped, a_k = mu(x_k), W = K_y^-1 k(X, x_k); the record jes_ref.covariances takes."""
    xs = np.clip(np.asarray(x_ref, dtype=np.float64), 0.0, 1.0)
    p = gram_ref.predict(f, xs)
    Kx = gram_ref.gram_cross(f["X"], xs, f["ell"], f["a"], f["kernel"])
    return dict(xs=xs, a=p["mean"], W=f["Kinv"] @ Kx)


def evaluate(f, o, Xs, noise_var, include_self=True, want_grad=True):
    """KG (and its gradient) at the columns of Xs from a fit and its fixed points: (val, grad, info)."""
    p = gram_ref.predict(f, Xs, want_grad=want_grad)
    if want_grad:
        cov, dcov = jes_ref.covariances(f, o, Xs, True)
        return kg(p["mean"], p["dev"], cov, o["a"], noise_var, include_self, p["dmean"], p["ddev"], dcov)
    return kg(p["mean"], p["dev"], jes_ref.covariances(f, o, Xs), o["a"], noise_var, include_self)
