"""numpy restatement of line EUBO, the expected utility of the best of q grid positions on a slider, as include/sls_hip.h states it
("expected utility of the best slider position"): the expansion of a line into the set of its positions exactly as stated
(u_i a + t_i b with u_i = (q-1-i)/(q-1), t_i = i/(q-1); numpy does not fuse the products into the sum), tests/qeubo_ref.py or
tests/qnei_ref.py at that set, and the fold of the set gradient onto the ends as a sequential loop over i (increasing for the first end, decreasing for the
second)."""
import numpy as np

import qeubo_ref as qr
import qnei_ref as nr


def weights(q):
    """(u (q,), t (q,)): one double division of two exact integers each, so u[i] == t[q-1-i] to the bit."""
    i = np.arange(q, dtype=np.float64)
    den = np.float64(q - 1)
    return (den - i) / den, i / den


def split(lines, D, anchor=None):
    """(a, b), each D x M, of a line block: 2D x M (free form), or D x M = b with a = anchor for every line."""
    lines = np.asarray(lines, float)
    if anchor is None:
        assert lines.shape[0] == 2 * D
        return lines[:D], lines[D:]
    assert lines.shape[0] == D
    return np.repeat(np.asarray(anchor, float)[:, None], lines.shape[1], axis=1), lines


def expand(lines, q, D, anchor=None):
    """The sets (qD x M) of the lines: rows iD..iD+D-1 = x_i = u_i a + t_i b, two products and one sum, no clamp."""
    a, b = split(lines, D, anchor)
    u, t = weights(q)
    sets = np.empty((q * D, a.shape[1]))
    for i in range(q):
        ua = u[i] * a
        tb = t[i] * b
        sets[i * D:(i + 1) * D] = ua + tb
    return sets


def fold(set_grad, q, D, anchored=False):
    """The line gradient of a set gradient (qD x M): grad_a = sum_i u_i g_i from zero in increasing i, grad_b = sum_i t_i g_i from zero
    in DECREASING i (the mirror image of grad_a's order), product and sum as separate roundings.  2D x M (rows 0..D-1 = grad_a), or
    D x M = grad_b alone when anchored."""
    u, t = weights(q)
    M = set_grad.shape[1]
    ga, gb = np.zeros((D, M)), np.zeros((D, M))
    for i in range(q):
        j = q - 1 - i
        ug = u[i] * set_grad[i * D:(i + 1) * D]
        tg = t[j] * set_grad[j * D:(j + 1) * D]
        ga = ga + ug
        gb = gb + tg
    return gb if anchored else np.concatenate([ga, gb], axis=0)


def unfolded(ref, lines, q, anchor=None, baseline=None):
    """The set gradient (qD x M) behind line()."""
    sets = expand(lines, q, ref.D, anchor)
    return (qr.qeubo(ref, sets, q) if baseline is None else nr.qnei(ref, sets, q, baseline))[1]


def line(ref, lines, q, anchor=None, baseline=None):
    """ref: a PathRef.  Returns (val (M,), grad (2D or D, M), wins (q, M) int, gap (M,)) -- qeubo_ref.qeubo (baseline None) or
    qnei_ref.qnei at the expanded sets, the gradient folded; gap is theirs.  A guarded set (floor / 0 and a zero set gradient) folds to
    an exactly zero line gradient."""
    D = ref.D
    sets = expand(lines, q, D, anchor)
    if baseline is None:
        val, sg, wins, gap = qr.qeubo(ref, sets, q)
    else:
        val, sg, wins, gap = nr.qnei(ref, sets, q, baseline)
    return val, fold(sg, q, D, anchored=anchor is not None), wins, gap
