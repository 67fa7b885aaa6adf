"""numpy restatement of qNEI, noisy expected improvement of q points on posterior draws, as include/sls_hip.h states it ("noisy
expected improvement on posterior draws"), on the draws of path_ref.PathRef: the per-draw incumbent as a column maximum with the
lowest index winning ties, every draw at every option (eval_all), the scan against the draw's baseline with a strictly-greater test,
the sum over the draws in increasing order with one division, and qeubo_ref's gradient by linearity on the aggregated weights."""
import numpy as np

import qeubo_ref as qr


def max_over_points(ref, Xb):
    """ref: a PathRef; Xb (D, Mb).  Returns (t (S,), arg (S,) int, gap (S,)): the per-draw maximum over the points, the lowest index
    that attains it (NaN and -1 where a draw has a NaN), and the difference between the two largest values (inf for Mb = 1) -- how
    far the values may move before the argmax changes."""
    V = ref.eval_all(np.asarray(Xb, float))                                    # Mb x S
    arg = np.argmax(V, axis=0)                                                  # the first maximum
    t = V.max(axis=0)
    bad = np.isnan(V).any(axis=0)
    if V.shape[0] > 1:
        top = np.sort(V, axis=0)
        gap = top[-1] - top[-2]
    else:
        gap = np.full(V.shape[1], np.inf)
    return np.where(bad, np.nan, t), np.where(bad, -1, arg).astype(np.int64), gap


def qnei(ref, sets, q, t):
    """sets (qD, M), rows iD..iD+D-1 = option i; t (S,) the per-draw baseline.  Returns (val (M,), grad (qD, M), wins (q, M) int,
    gap (M,)): gap is, per set, the smallest of the best-versus-second-best option difference over the draws (inf for q = 1) and
    min |v_{i,s} - t_s| -- how far the values may move before a winner, or whether there is one, changes."""
    sets, t = np.asarray(sets, float), np.asarray(t, float)
    D, S = ref.D, ref.n_draws
    M = sets.shape[1]
    assert sets.shape[0] == q * D and t.shape == (S,)
    V = np.stack([ref.eval_all(sets[i * D:(i + 1) * D]) for i in range(q)])     # q x M x S
    best = np.broadcast_to(t, (M, S)).copy()
    arg = np.full((M, S), -1)
    for i in range(q):                                                          # strictly greater: the lowest option wins ties
        up = V[i] > best
        best = np.where(up, V[i], best)
        arg = np.where(up, i, arg)
    total = np.zeros(M)
    for s in range(S):
        total = total + (best[:, s] - t[s])
    val = total / S
    wins = np.stack([(arg == i).sum(axis=1) for i in range(q)]).astype(np.int64)
    gap = np.abs(V - t[None, None, :]).min(axis=(0, 2))
    if q > 1:
        top = np.sort(V, axis=0)
        gap = np.minimum(gap, (top[-1] - top[-2]).min(axis=1))
    grad = np.empty((q * D, M))
    for i in range(q):
        mask = (arg == i).astype(float)                                         # M x S; all zero in a draw nobody improves
        grad[i * D:(i + 1) * D] = qr.grad_with_weights(ref, sets[i * D:(i + 1) * D], ref.W @ mask.T, ref.v @ mask.T) / S
    bad = np.isnan(V).any(axis=(0, 2)) | np.isnan(val) | np.isnan(grad).any(axis=0)
    return np.where(bad, 0.0, val), np.where(bad[None, :], 0.0, grad), wins, gap
