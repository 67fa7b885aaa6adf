"""Plain numpy restatement of the two kernel functions and of the GP quantities built on their Gram
matrices, for the short-length-scale tests (test_gram_ref_cpu.py, test_gpu_short_length_scales.py).

q_ij = sum_d ((x_id - x_jd) / l_d)^2 from the RAW coordinates: differenced first, divided by l afterwards.  A near-duplicate pair's
difference is then exact (Sterbenz) and q carries a relative error of (D + 4) eps whatever l is; differencing scaled coordinates
leaves eps / l, the norm expansion |x~_i|^2 + |x~_j|^2 - 2 x~_i . x~_j leaves eps D / (2 l^2) ABSOLUTE (gram_expansion below
emulates that form so that the CPU test can show the cases would expose it).

Every function takes dtype = numpy.float64 or numpy.longdouble; the inputs are fp64 values either way (what the device is given)."""
import math

import numpy as np

A, B = 0.7, 5e-3                                       # signal variance and noise level of every case
EPS = float(np.finfo(np.float64).eps)
ELL_CASES = (0.3, 3e-2, 3e-3, 1e-5, 1e-8, "ard")       # isotropic l, and one ARD case: one l = 1e-5 among 0.3s
SIZES = ((100, 6), (129, 6), (300, 6), (300, 33), (300, 64), (200, 65))   # both sides of N = 128, D = 32 / 64, D % 16
# D > 128 (a second and a third 128-column tile of the gradient contraction, no one-wavefront route, no single-launch fit): the
# smallest shapes with two row tiles or two / three column tiles.  l = 0.3 sqrt(D) keeps the problem dense (every gradient row is
# non-trivial); the last two lie beyond the guard of the norm expansion.
WIDE_DENSE = ((130, 129, 3.4), (90, 257, 4.8), (200, 192, 4.2))
WIDE_CASES = WIDE_DENSE + ((130, 129, 3e-3), (90, 257, "ard"))
WIDE_SIZES = tuple((N, D) for (N, D, _) in WIDE_DENSE)
N_PAIRS = 20
N_CAND = 40                                            # 0..15 ordinary, 16..27 outside the box, 28..37 against training points, 38/39 a pair
CAND_NEAR = range(28, 38)
CAND_PAIR = (38, 39)


def ell_vector(case, D):
    if case == "ard":
        ell = np.full(D, 0.3)
        ell[D // 2] = 1e-5
        return ell
    return np.full(D, float(case))


def gram_tolerance(D, a=A):
    """|dK| <= 4 (D + 8) eps a: the direct form's q has relative error <= (D + 4) eps, q e^(-q/2) <= 2/e (Matern: (5/6) q (1 + s) e^-s
    < 0.6), the rest is room for exp and sqrt."""
    return 4.0 * (D + 8) * EPS * a


def _offset(rng, ell, s, D):
    return ell * s * rng.normal(size=D) / math.sqrt(D)


def problem(N, D, case, seed=0):
    """Uniform points in [0, 1]^D; N_PAIRS near-duplicate pairs X[:, j+1] = X[:, j] + l s g / sqrt(D), s in [0.1, 1] (the pair's true q
    is s^2 |g|^2 / D = O(1) at that l, per dimension for ARD); targets; candidates of the four kinds listed at N_CAND."""
    rng = np.random.default_rng(1000 * N + 10 * D + seed)
    ell = ell_vector(case, D)
    X = rng.uniform(0, 1, (D, N))
    for p in range(N_PAIRS):
        j = 2 * p
        X[:, j + 1] = np.clip(X[:, j] + _offset(rng, ell, rng.uniform(0.1, 1.0), D), 0.0, 1.0)
    y = 0.5 * np.sin(3.0 * X.sum(axis=0) / math.sqrt(D)) + 0.05 * rng.normal(size=N)
    Xs = rng.uniform(0, 1, (D, N_CAND))
    Xs[:, 16:28] = Xs[:, 16:28] * 1.6 - 0.3                                   # norms beyond the box bound
    for k, c in enumerate(CAND_NEAR):
        Xs[:, c] = X[:, 41 + 3 * k] + _offset(rng, ell, 0.7, D)               # q ~ 0.5 from a training point that has no twin
    Xs[:, CAND_PAIR[1]] = Xs[:, CAND_PAIR[0]] + _offset(rng, ell, 0.7, D)
    return dict(X=np.asfortranarray(X), y=y, Xs=np.asfortranarray(Xs), ell=ell, theta=np.concatenate([[A], ell]), a=A, b=B)


def sqdist(Xa, Xb, ell, dtype=np.float64):
    """q[i, j] between the columns of Xa (D x Na) and Xb (D x Nb), dimension by dimension in index order."""
    Xa, Xb, ell = np.asarray(Xa, dtype=dtype), np.asarray(Xb, dtype=dtype), np.asarray(ell, dtype=dtype)
    q = np.zeros((Xa.shape[1], Xb.shape[1]), dtype=dtype)
    for d in range(Xa.shape[0]):
        t = (Xa[d][:, None] - Xb[d][None, :]) / ell[d]
        q += t * t
    return q


def sqdist_expansion(Xa, Xb, ell):
    """fp64 emulation of the matrix-core form: x~ = (x - 0.5) / l, q = |x~_i|^2 + |x~_j|^2 - 2 x~_i . x~_j, clamped at 0.  The
    arithmetic form only: the kernels' accumulation order differs."""
    Ta, Tb = (np.asarray(Xa) - 0.5) * (1.0 / ell)[:, None], (np.asarray(Xb) - 0.5) * (1.0 / ell)[:, None]
    q = (Ta * Ta).sum(axis=0)[:, None] + (Tb * Tb).sum(axis=0)[None, :] - 2.0 * (Ta.T @ Tb)
    return np.maximum(q, 0.0)


def kern(q, a, kernel, dtype=np.float64):
    """(k, c) with dk/dx_a = -c d / l^2 (Appendix A): SE k = c = a e^(-q/2); Matern-5/2 k = a (1 + s + s^2/3) e^-s, c = a 5/3 (1 + s) e^-s."""
    q, a = np.asarray(q, dtype=dtype), dtype(a)
    if kernel == 0:
        k = a * np.exp(-q / dtype(2))
        return k, k
    s = np.sqrt(dtype(5) * q)
    e = np.exp(-s)
    return a * (dtype(1) + s + dtype(5) * q / dtype(3)) * e, a * (dtype(5) / dtype(3)) * (dtype(1) + s) * e


def gram(X, ell, a, b, kernel, dtype=np.float64, q=None):
    """K_y = K_f + b I (N x N).  q: a precomputed distance matrix."""
    K = kern(sqdist(X, X, ell, dtype) if q is None else q, a, kernel, dtype)[0]
    N = K.shape[0]
    K[np.arange(N), np.arange(N)] = dtype(a) + dtype(b)
    return K


def gram_cross(X, Xs, ell, a, kernel, dtype=np.float64, q=None):
    """K* (N x M)."""
    return kern(sqdist(X, Xs, ell, dtype) if q is None else q, a, kernel, dtype)[0]


def cholesky(K):
    """Lower factor, column by column, in K's own type (numpy.linalg has no longdouble)."""
    L = np.array(K, copy=True)
    N = L.shape[0]
    for j in range(N):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return np.tril(L)


def solve_lower(L, Bm):
    """L^-1 B by forward substitution, row by row."""
    Y = np.array(Bm, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        if i:
            Y[i] -= L[i, :i] @ Y[:i]
        Y[i] /= L[i, i]
    return Y


def fit(X, y, ell, a, b, kernel, dtype=np.float64, expansion=False):
    """alpha = K_y^-1 y, K_y^-1, log|K_y| and what predict() needs.  expansion=True (fp64 only): the Gram matrices come from the
    emulated norm expansion."""
    assert not expansion or dtype is np.float64
    q = sqdist_expansion(X, X, ell) if expansion else sqdist(X, X, ell, dtype)
    K = gram(X, ell, a, b, kernel, dtype, q=q)
    L = cholesky(K)
    Li = solve_lower(L, np.eye(K.shape[0], dtype=dtype))
    Kinv = Li.T @ Li
    alpha = Li.T @ (Li @ np.asarray(y, dtype=dtype))
    return dict(X=X, y=np.asarray(y, dtype=dtype), ell=ell, a=a, b=b, kernel=kernel, dtype=dtype, expansion=expansion, q=q, K=K, Li=Li,
                Kinv=Kinv, alpha=alpha, logdet=dtype(2) * np.log(np.diag(L)).sum())


def predict(f, Xs, want_grad=False):
    """Posterior mean, deviation sqrt(a - k^T K_y^-1 k) and joint covariance at the columns of Xs; with want_grad the gradients of
    mean and deviation (D x M)."""
    dt = f["dtype"]
    qs = sqdist_expansion(f["X"], Xs, f["ell"]) if f["expansion"] else sqdist(f["X"], Xs, f["ell"], dt)
    Ks, Cs = kern(qs, f["a"], f["kernel"], dt)
    V = f["Li"] @ Ks
    qss = sqdist_expansion(Xs, Xs, f["ell"]) if f["expansion"] else sqdist(Xs, Xs, f["ell"], dt)
    Kss = kern(qss, f["a"], f["kernel"], dt)[0]
    M = Kss.shape[0]
    Kss[np.arange(M), np.arange(M)] = dt(f["a"])
    cov = Kss - V.T @ V
    mean = Ks.T @ f["alpha"]
    dev = np.sqrt(np.maximum(dt(f["a"]) - (V * V).sum(axis=0), dt(0)))
    out = dict(mean=mean, dev=dev, cov=cov)
    if want_grad:
        W = f["Kinv"] @ Ks                                                  # N x M
        Xd, Xsd, ell = np.asarray(f["X"], dtype=dt), np.asarray(Xs, dtype=dt), np.asarray(f["ell"], dtype=dt)
        dmean, ddev = np.empty(Xsd.shape, dtype=dt), np.empty(Xsd.shape, dtype=dt)
        for d in range(Xsd.shape[0]):
            J = -Cs * (Xsd[d][None, :] - Xd[d][:, None]) / (ell[d] * ell[d])    # dk(x*, x_i) / dx*_d
            dmean[d] = (J * f["alpha"][:, None]).sum(axis=0)
            ddev[d] = -(J * W).sum(axis=0) / dev
        out.update(dmean=dmean, ddev=ddev)
    return out


def acquisition(f, Xs, acq, ucb_h=1.0, pred=None):
    """EI (acq 0: Delta Phi(u) + sigma phi(u) against mu+ = max_i (y_i - b alpha_i), gradient Phi grad mu + phi grad sigma) or UCB
    (acq 1: mu + h sigma).  Phi and phi are evaluated in fp64 from u in either type (there is no longdouble erfc): what this file
    pins is the posterior that goes into them."""
    dt = f["dtype"]
    p = predict(f, Xs, want_grad=True) if pred is None else pred
    if acq == 1:
        return p["mean"] + dt(ucb_h) * p["dev"], p["dmean"] + dt(ucb_h) * p["ddev"]
    mu_best = (f["y"] - dt(f["b"]) * f["alpha"]).max()
    diff = p["mean"] - mu_best
    u = np.asarray(diff / p["dev"], dtype=np.float64)
    Phi = np.array([0.5 * math.erfc(-v / math.sqrt(2.0)) for v in u]).astype(dt)
    phi = (np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)).astype(dt)
    return diff * Phi + p["dev"] * phi, Phi[None, :] * p["dmean"] + phi[None, :] * p["ddev"]


def _log_lognormal(x, m, v, dt):
    return -np.log(x) - dt(0.5) * np.log(dt(2) * dt(np.pi) * v) - (np.log(x) - m) ** 2 / (dt(2) * v)


def _log_lognormal_derivative(x, m, v):
    return (m - v - np.log(x)) / (v * x)


def gp_map_objective(X, y, hyp, kernel, dtype=np.float64, f=None):
    """The GP MAP objective at hyp = (a, b, l_1..l_D): log marginal likelihood plus the log-normal priors a ~ LN(ln 0.5, 0.5),
    b ~ LN(ln 1e-4, 0.5), l ~ LN(ln 0.5, 0.5), and its gradient (D + 2), g_p = 1/2 sum_ij (alpha alpha^T - K_y^-1)_ij dK_ij/dtheta_p.
    f: the fit() of the same data and hyper-parameters, when the caller has it."""
    dt = dtype
    hyp = np.asarray(hyp, dtype=dt)
    a, b, ell = hyp[0], hyp[1], hyp[2:]
    if f is None:
        f = fit(X, y, ell, a, b, kernel, dt)
    N, D = f["K"].shape[0], ell.size
    v2, ma, mb, mr = dt(0.5), np.log(dt(0.5)), np.log(dt(1e-4)), np.log(dt(0.5))
    val = (-dt(0.5) * (f["y"] @ f["alpha"]) - dt(0.5) * f["logdet"] - dt(0.5) * dt(N) * np.log(dt(2) * dt(np.pi)) +
           _log_lognormal(a, ma, v2, dt) + _log_lognormal(b, mb, v2, dt) + _log_lognormal(ell, mr, v2, dt).sum())
    W = np.outer(f["alpha"], f["alpha"]) - f["Kinv"]
    k, c = kern(f["q"], a, kernel, dt)
    g = np.empty(D + 2, dtype=dt)
    g[0] = dt(0.5) * (W * k).sum() / a + _log_lognormal_derivative(a, ma, v2)
    g[1] = dt(0.5) * np.trace(W) + _log_lognormal_derivative(b, mb, v2)
    Xd = np.asarray(X, dtype=dt)
    Wc = W * c
    for d in range(D):
        t = (Xd[d][:, None] - Xd[d][None, :]) / ell[d]
        g[2 + d] = dt(0.5) * (Wc * t * t).sum() / ell[d] + _log_lognormal_derivative(ell[d], mr, v2)
    return val, g


_CACHE = {}


def reference(N, D, case, kernel, dtype=np.float64, expansion=False):
    """Everything the tests compare against for one case, computed once per session and shared (callers must not modify it):
    the problem, fit(), predict() with gradients at the candidates, EI and UCB (h = 2), and the MAP objective at (a, b, l)."""
    key = (N, D, case, kernel, dtype, expansion)
    if key not in _CACHE:
        p = problem(N, D, case)
        f = fit(p["X"], p["y"], p["ell"], A, B, kernel, dtype, expansion)
        r = dict(p, fit=f, Ks=gram_cross(p["X"], p["Xs"], p["ell"], A, kernel, dtype,
                                         q=sqdist_expansion(p["X"], p["Xs"], p["ell"]) if expansion else None),
                 pred=predict(f, p["Xs"], want_grad=True), hyp=np.concatenate([[A, B], p["ell"]]))
        r.update(ei=acquisition(f, p["Xs"], 0, pred=r["pred"]), ucb=acquisition(f, p["Xs"], 1, 2.0, pred=r["pred"]))
        if not expansion:
            r["map"] = gp_map_objective(p["X"], p["y"], r["hyp"], kernel, dtype, f=f)
        _CACHE[key] = r
    return _CACHE[key]


def errors(got, ref):
    """The measured errors of `got` against `ref` (both with the keys of check()), as plain floats for util.record."""
    out = {}
    for k in got:
        g, r = np.asarray(got[k], dtype=np.longdouble), np.asarray(ref[k], dtype=np.longdouble)
        out[k] = dict(max_abs=float(np.abs(g - r).max()), scale=float(np.abs(r).max()))
    return out


def check(got, ref, D, y_max):
    """Hold `got` to `ref` at the tolerances of the issue, key by key (only the keys present in `got`):
    K, Ks: 4 (D + 8) eps a per entry.  alpha: rtol 1e-6, atol 1e-7 |y|max.  Kinv: 1e-9 of its largest entry.  logdet: rtol 1e-10.
    mean / cov: rtol 1e-8, atol 1e-10.  dev: rtol 1e-7, atol 1e-10.  acquisition values and gradients: rtol 1e-6, atol 1e-9 of the
    largest (so too the gradients of mean and deviation).  MAP value 1e-8 max(1, |v|); MAP gradient rtol 1e-6, atol 1e-8 max(1, |g|max)."""
    def close(k, rtol, atol):
        g, r = np.asarray(got[k], dtype=np.longdouble), np.asarray(ref[k], dtype=np.longdouble)
        bad = np.abs(g - r) > atol + rtol * np.abs(r)
        assert not bad.any(), (k, int(bad.sum()), float(np.abs(g - r).max()), float(np.abs(r).max()), rtol, atol)
    for k in got:
        rmax = float(np.abs(np.asarray(ref[k], dtype=np.longdouble)).max())
        if k in ("K", "Ks"):
            close(k, 0.0, gram_tolerance(D))
        elif k == "alpha":
            close(k, 1e-6, 1e-7 * y_max)
        elif k == "Kinv":
            close(k, 0.0, 1e-9 * rmax)
        elif k == "logdet":
            close(k, 1e-10, 0.0)
        elif k in ("mean", "cov"):
            close(k, 1e-8, 1e-10)
        elif k == "dev":
            close(k, 1e-7, 1e-10)
        elif k in ("ei", "ei_grad", "ucb", "ucb_grad", "dmean", "ddev"):    # UCB's gradient is dmean + h ddev: its tolerance
            close(k, 1e-6, 1e-9 * max(rmax, 1e-30))
        elif k == "map_value":
            close(k, 0.0, 1e-8 * max(1.0, rmax))
        elif k == "map_grad":
            close(k, 1e-6, 1e-8 * max(1.0, rmax))
        else:
            raise KeyError(k)


def quantities(r):
    """The comparable quantities of a reference() record, under the keys of check()."""
    out = dict(K=r["fit"]["K"], Ks=r["Ks"], alpha=r["fit"]["alpha"], Kinv=r["fit"]["Kinv"], logdet=r["fit"]["logdet"],
               mean=r["pred"]["mean"], dev=r["pred"]["dev"], cov=r["pred"]["cov"], ei=r["ei"][0], ei_grad=r["ei"][1],
               ucb=r["ucb"][0], ucb_grad=r["ucb"][1], dmean=r["pred"]["dmean"], ddev=r["pred"]["ddev"])
    if "map" in r:
        out.update(map_value=r["map"][0], map_grad=r["map"][1])
    return out
