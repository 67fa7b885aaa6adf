"""numpy restatement of qEUBO, the expected utility of the best of q options on posterior draws, as include/sls_hip.h states it
("expected utility of the best of q options"), on the draws of path_ref.PathRef: every draw at every option (eval_all), the first
option winning ties, the sum over the draws in increasing order with one division, and the gradient by linearity on the aggregated
weights (the sums of the columns of W and v over the draws an option wins)."""
import numpy as np

import path_ref as ph

FLOOR = -1.0e300


def grad_with_weights(ref, Xs, Wb, Vb):
    """Gradient (D x M) at Xs[:, m] of the path function with weights (Wb[:, m] (2F), Vb[:, m] (N)): PathRef.eval's formulas, or the
    reference's own where it has them (path_short_ref: raw coordinate differences, in its own number type)."""
    if hasattr(ref, "grad_with_weights"):
        return ref.grad_with_weights(Xs, Wb, Vb)
    Xs = np.asarray(Xs, float)
    T = ref.om @ ((Xs - 0.5) / ref.ell[:, None])                    # F x M
    wc, ws = Wb[:ref.F], Wb[ref.F:]
    g = ws * np.cos(T) - wc * np.sin(T)
    grad = (ref.om.T @ g) / ref.ell[:, None]
    _, c = ph.kernel_c(Xs, ref.X, ref.theta, ref.kernel)            # M x N
    cv = c * Vb.T
    l2 = (ref.ell ** 2)[:, None]
    return grad - (Xs * cv.sum(axis=1)[None, :] - ref.X @ cv.T) / l2


def qeubo(ref, sets, q):
    """ref: a PathRef; sets (qD, M), rows iD..iD+D-1 = option i.  Returns (val (M,), grad (qD, M), wins (q, M) int, gap (M,)): gap
    is, per set, the smallest difference between the best and the second-best option over the draws (inf for q = 1) -- how far the
    values may move before a winner changes."""
    sets = np.asarray(sets, float)
    D, S = ref.D, ref.n_draws
    M = sets.shape[1]
    assert sets.shape[0] == q * D
    V = np.stack([ref.eval_all(sets[i * D:(i + 1) * D]) for i in range(q)])     # q x M x S
    arg = np.argmax(V, axis=0)                                                  # the first maximum: the lowest i wins ties
    best = np.take_along_axis(V, arg[None], axis=0)[0]                          # M x S
    total = np.zeros(M)
    for s in range(S):
        total = total + best[:, s]
    val = total / S
    wins = np.stack([(arg == i).sum(axis=1) for i in range(q)]).astype(np.int64)
    if q > 1:
        top = np.sort(V, axis=0)
        gap = (top[-1] - top[-2]).min(axis=1)
    else:
        gap = np.full(M, np.inf)
    grad = np.empty((q * D, M))
    for i in range(q):
        mask = (arg == i).astype(float)                                         # M x S
        grad[i * D:(i + 1) * D] = grad_with_weights(ref, sets[i * D:(i + 1) * D], ref.W @ mask.T, ref.v @ mask.T) / S
    bad = np.isnan(V).any(axis=(0, 2)) | np.isnan(val) | np.isnan(grad).any(axis=0)
    return np.where(bad, FLOOR, val), np.where(bad[None, :], 0.0, grad), wins, gap


def pair_variance(ref, Xa, Xb):
    """Var[f_s(x) - f_s(x')] over the draws of THIS frequency set for the pairs (Xa[:, m], Xb[:, m]): path_ref.pathwise_cov at the
    2M points, cov00 + cov11 - 2 cov01.  With it the closed form of eubo_ref is the exact expectation of the q = 2 estimator."""
    import posterior_ref as pr
    M = Xa.shape[1]
    P = np.concatenate([Xa, Xb], axis=1)
    Ps, PX = ph.features(ref.om, ref.a, P, ref.ell), ph.features(ref.om, ref.a, ref.X, ref.ell)
    KsX = pr.ard_kernel(P, ref.X, ref.theta, ref.kernel)
    cov = ph.pathwise_cov(Ps.T @ Ps, Ps.T @ PX, PX.T @ PX, KsX.T, ref.Ky, ref.b)
    i, j = np.arange(M), M + np.arange(M)
    return cov[i, i] + cov[j, j] - 2.0 * cov[i, j]
