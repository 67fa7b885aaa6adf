"""numpy restatement of qBALD, the information gain of a q-option choice query on posterior draws, as include/sls_hip.h states it
("information gain of a choice query on posterior draws"), on the draws of path_ref.PathRef: every draw at every option
(eval_all), the BTL probabilities with the maximum subtracted before the division by the scale, the header's order-free fixed-point
sum over the options, the predicted choice probabilities (from zero, s increasing, one division), KL_s as a signed sum in index
order, the weights c = d value / d v, and qeubo_ref's gradient by linearity on the aggregated weights -- with no further division."""
import numpy as np

import qeubo_ref as qr

FIX = 2.0 ** 58
FLOOR = -1.0e300


def weights(V, tau):
    """V (q, M, S) the values.  Returns (value (M,), c (q, M, S), p (q, M, S), pbar (q, M))."""
    q, M, S = V.shape
    with np.errstate(all="ignore"):
        z = (V - V.max(axis=0)[None]) / tau
        E = np.exp(z)
        Z = np.rint(np.nan_to_num(E) * FIX).astype(np.int64).sum(axis=0).astype(float) / FIX
        p = E / Z[None]
        tot = np.zeros((q, M))
        for s in range(S):
            tot = tot + p[:, :, s]
        pbar = tot / S
        l = np.where(p > 0.0, np.log(p) - np.log(pbar)[:, :, None], 0.0)
        KL = np.zeros((M, S))
        for i in range(q):
            KL = KL + p[i] * l[i]
        total = np.zeros(M)
        for s in range(S):
            total = total + KL[:, s]
        c = p * (l - KL[None]) / (S * tau)
    return total / S, c, p, pbar


def hard_wins(V):
    """sls_qeubo_eval's scan: the lowest index wins a tie.  (q, M) int."""
    arg = np.argmax(V, axis=0)
    return np.stack([(arg == i).sum(axis=1) for i in range(V.shape[0])]).astype(np.int64)


def draw_gradient_norms(ref, sets, q):
    """(q, M, S): |grad f_s(x_i)|_inf of every draw at every option (it does not depend on the scale: form it once per case)."""
    D, S, M = ref.D, ref.n_draws, sets.shape[1]
    g = np.empty((q, M, S))
    for i in range(q):
        for s in range(S):
            g[i, :, s] = np.abs(ref.eval(sets[i * D:(i + 1) * D], np.full(M, s))[1]).max(axis=0)
    return g


def qbald(ref, sets, q, tau, want_G=True, gabs=None):
    """sets (qD, M), rows iD..iD+D-1 = option i; tau the BTL scale.  Returns a dict: val (M,), grad (qD, M), prob (q, M), wins (q, M)
    int (hard), c (q, M, S), p (q, M, S), A (M,) = sum |c|, and with want_G (else None) G (M,) = sum |c| |grad f_s(x_i)|_inf and
    P (M,) = sum p |grad f_s(x_i)|_inf / (S tau) (gabs: draw_gradient_norms, formed here when None), and gap (M,): the smallest
    difference over the draws between the two largest values (inf for q = 1)."""
    sets = np.asarray(sets, float)
    D, S = ref.D, ref.n_draws
    M = sets.shape[1]
    assert sets.shape[0] == q * D
    V = np.stack([ref.eval_all(sets[i * D:(i + 1) * D]) for i in range(q)])     # q x M x S
    val, c, p, pbar = weights(V, tau)
    grad = np.empty((q * D, M))
    for i in range(q):
        grad[i * D:(i + 1) * D] = qr.grad_with_weights(ref, sets[i * D:(i + 1) * D], ref.W @ c[i].T, ref.v @ c[i].T)
    G = P = None
    if want_G:
        if gabs is None:
            gabs = draw_gradient_norms(ref, sets, q)
        G, P = np.zeros(M), np.zeros(M)
        for i in range(q):
            for s in range(S):
                G = G + np.abs(c[i, :, s]) * gabs[i, :, s]
                P = P + p[i, :, s] * gabs[i, :, s] / (S * tau)
    if q > 1:
        top = np.sort(V, axis=0)
        gap = (top[-1] - top[-2]).min(axis=1)
    else:
        gap = np.full(M, np.inf)
    bad = np.isnan(V).any(axis=(0, 2)) | np.isnan(val) | np.isnan(grad).any(axis=0)
    return dict(val=np.where(bad, FLOOR, val), grad=np.where(bad[None, :], 0.0, grad), prob=np.where(bad[None, :], 0.0, pbar),
                wins=hard_wins(V), c=c, p=p, A=np.abs(c).sum(axis=(0, 2)), G=G, P=P, gap=gap)
