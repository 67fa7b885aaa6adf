"""numpy restatement of qLogNEI, log-space noisy expected improvement of q points on posterior draws, as include/sls_hip.h states it
("log-space noisy expected improvement on posterior draws"), on the draws of path_ref.PathRef: every draw at every option
(eval_all), log softplus in its three branches, the temperature log-sum-exp over the options, the log-sum-exp over the draws, the
weights c = d value / d v, and qeubo_ref's gradient by linearity on the aggregated weights -- with no division by S.  The sum over
the options is the header's order-free fixed-point sum, so permuting the options permutes the weights and gradient blocks exactly;
the log-sum-exp over the draws is formed from the maximum (not online, as the device does): the difference is rounding."""
import numpy as np

import qeubo_ref as qr

CUT = -36.0
FIX = 2.0 ** 58


def terms(a):
    """(L, R) = (log softplus(a), dL/da), elementwise, in the header's three branches."""
    a = np.asarray(a, float)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(a))
        lp = np.log1p(e)
        pos = a >= 0.0
        sp = np.where(pos, a + lp, lp)
        L = np.where(a < CUT, a, np.log(sp))
        R = np.where(a < CUT, 1.0, np.where(pos, 1.0, e) / ((1.0 + e) * sp))
    return L, R


def weights(V, t, tau_relu, tau_max):
    """V (q, M, S) the values, t (S,).  Returns (value (M,), c (q, M, S), rho_max (M,), log c (q, M, S)): log c is the sum of the three
    factors' logarithms, finite where c itself has underflowed to 0."""
    q, M, S = V.shape
    L, R = terms((V - t[None, None, :]) / tau_relu)
    l = np.log(tau_relu) + L
    rho = R / tau_relu
    Mq = l.max(axis=0)                                                           # M x S
    E = np.exp((l - Mq[None]) / tau_max)
    # the header's order-free sum over the options: the terms, all in [0, 1], rounded to multiples of 2^-58 and added as integers
    Zq = np.rint(np.nan_to_num(E) * FIX).astype(np.int64).sum(axis=0).astype(float) / FIX
    pi = E / Zq[None]
    m = Mq + tau_max * np.log(Zq)
    Mx = m.max(axis=1)                                                           # M
    Ex = np.exp(m - Mx[:, None])
    Z = np.zeros(M)
    for s in range(S):
        Z = Z + Ex[:, s]
    value = Mx + np.log(Z) - np.log(float(S))
    omega = Ex / Z[:, None]
    log_c = ((m - Mx[:, None]) - np.log(Z)[:, None])[None] + ((l - Mq[None]) / tau_max - np.log(Zq)[None]) + np.log(rho)
    return value, omega[None] * pi * rho, rho.max(axis=(0, 2)), log_c


def hard_wins(V, t):
    """sls_qnei_eval's scan: best = t_s, strictly greater, increasing i.  (q, M) int."""
    q, M, S = V.shape
    best = np.broadcast_to(t, (M, S)).copy()
    arg = np.full((M, S), -1)
    for i in range(q):
        up = V[i] > best
        best = np.where(up, V[i], best)
        arg = np.where(up, i, arg)
    return np.stack([(arg == i).sum(axis=1) for i in range(q)]).astype(np.int64)


def qlognei(ref, sets, q, t, tau_relu, tau_max, want_G=True):
    """sets (qD, M), rows iD..iD+D-1 = point i; t (S,) the per-draw baseline.  Returns a dict: val (M,), grad (qD, M), wins (q, M) int
    (hard), c (q, M, S), A (M,) = sum_{i,s} c, G (M,) = sum_{i,s} c max_d |d f_s / d x_d (x_i)| (want_G; else None), rho_max (M,),
    log_c (q, M, S)."""
    sets, t = np.asarray(sets, float), np.asarray(t, float)
    D, S = ref.D, ref.n_draws
    M = sets.shape[1]
    assert sets.shape[0] == q * D and t.shape == (S,)
    V = np.stack([ref.eval_all(sets[i * D:(i + 1) * D]) for i in range(q)])     # q x M x S
    with np.errstate(all="ignore"):
        val, c, rho_max, log_c = weights(V, t, tau_relu, tau_max)
    grad = np.empty((q * D, M))
    for i in range(q):
        grad[i * D:(i + 1) * D] = qr.grad_with_weights(ref, sets[i * D:(i + 1) * D], ref.W @ c[i].T, ref.v @ c[i].T)
    G = None
    if want_G:
        G = np.zeros(M)
        for i in range(q):
            for s in range(S):
                g = ref.eval(sets[i * D:(i + 1) * D], np.full(M, s))[1]         # D x M
                G = G + c[i, :, s] * np.abs(g).max(axis=0)
    bad = np.isnan(V).any(axis=(0, 2)) | np.isnan(val) | np.isnan(grad).any(axis=0)
    return dict(val=np.where(bad, -1.0e300, val), grad=np.where(bad[None, :], 0.0, grad), wins=hard_wins(V, t), c=c,
                A=c.sum(axis=(0, 2)), G=G, rho_max=rho_max, log_c=log_c)
