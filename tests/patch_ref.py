"""numpy restatement of gallery EUBO, the expected utility of the best cell of a qs x qt grid on the bilinear patch spanned by four
corners, as include/sls_hip.h states it ("expected utility of the best gallery cell"): the expansion of a patch into the set of its
cells exactly as stated (option k = i + qs j: lo = u_i c00 + s_i c10, hi = u_i c01 + s_i c11, x_k = v_j lo + t_j hi, the weights of
tests/line_ref.py along each axis; numpy does not fuse the products into the sums), tests/qeubo_ref.py or tests/qnei_ref.py at that
set, and the fold of the set gradient onto the corners as sequential loops in the stated orders."""
import numpy as np

import line_ref as lr
import qeubo_ref as qr
import qnei_ref as nr


def split(patches, D, anchor=None):
    """(c00, c10, c01, c11), each D x M, of a patch block: 4D x M (free form), or 3D x M = (c10, c01, c11) with c00 = anchor."""
    patches = np.asarray(patches, float)
    if anchor is None:
        assert patches.shape[0] == 4 * D
        return tuple(patches[c * D:(c + 1) * D] for c in range(4))
    assert patches.shape[0] == 3 * D
    c00 = np.repeat(np.asarray(anchor, float)[:, None], patches.shape[1], axis=1)
    return (c00,) + tuple(patches[c * D:(c + 1) * D] for c in range(3))


def expand(patches, qs, qt, D, anchor=None):
    """The sets (qs qt D x M) of the patches: rows kD..kD+D-1 = x_k, k = i + qs j; three sums of two products each, no clamp."""
    c00, c10, c01, c11 = split(patches, D, anchor)
    u, s = lr.weights(qs)
    v, t = lr.weights(qt)
    sets = np.empty((qs * qt * D, c00.shape[1]))
    for j in range(qt):
        for i in range(qs):
            a = u[i] * c00
            b = s[i] * c10
            lo = a + b
            a = u[i] * c01
            b = s[i] * c11
            hi = a + b
            a = v[j] * lo
            b = t[j] * hi
            k = i + qs * j
            sets[k * D:(k + 1) * D] = a + b
    return sets


def fold(set_grad, qs, qt, D, anchored=False):
    """The patch gradient of a set gradient (qs qt D x M).  Per row j: A_j = sum_i u_i g_{i + qs j} from zero in increasing i, B_j =
    sum_i s_i g_{i + qs j} from zero in DECREASING i.  grad_c00 = sum_j v_j A_j and grad_c10 = sum_j v_j B_j from zero in increasing j,
    grad_c01 = sum_j t_j A_j and grad_c11 = sum_j t_j B_j from zero in DECREASING j; product and sum as separate roundings.  4D x M
    (blocks c00, c10, c01, c11), or 3D x M without c00 when anchored."""
    u, s = lr.weights(qs)
    v, t = lr.weights(qt)
    M = set_grad.shape[1]
    g = lambda i, j: set_grad[(i + qs * j) * D:(i + qs * j + 1) * D]
    A, B = [], []
    for j in range(qt):
        a, b = np.zeros((D, M)), np.zeros((D, M))
        for i in range(qs):
            r = qs - 1 - i
            ug = u[i] * g(i, j)
            sg = s[r] * g(r, j)
            a = a + ug
            b = b + sg
        A.append(a)
        B.append(b)
    g00, g10, g01, g11 = (np.zeros((D, M)) for _ in range(4))
    for j in range(qt):
        r = qt - 1 - j
        p00 = v[j] * A[j]
        p10 = v[j] * B[j]
        p01 = t[r] * A[r]
        p11 = t[r] * B[r]
        g00 = g00 + p00
        g10 = g10 + p10
        g01 = g01 + p01
        g11 = g11 + p11
    return np.concatenate(([] if anchored else [g00]) + [g10, g01, g11], axis=0)


def patch(ref, patches, qs, qt, anchor=None, baseline=None):
    """ref: a PathRef.  Returns (val (M,), grad (4D or 3D, M), wins (qs qt, M) int, gap (M,)) -- qeubo_ref.qeubo (baseline None) or
    qnei_ref.qnei at the expanded sets, the gradient folded; gap is theirs.  A guarded set (floor / 0 and a zero set gradient) folds to
    an exactly zero patch gradient."""
    D, q = ref.D, qs * qt
    sets = expand(patches, qs, qt, D, anchor)
    if baseline is None:
        val, sg, wins, gap = qr.qeubo(ref, sets, q)
    else:
        val, sg, wins, gap = nr.qnei(ref, sets, q, baseline)
    return val, fold(sg, qs, qt, D, anchored=anchor is not None), wins, gap


# ---- the symmetries of the contract, as index maps shared by the tests ---------------------------------------------------------------
def mirror(patches, D, axis):
    """The free-form block with c00 <-> c10, c01 <-> c11 (axis "s") or c00 <-> c01, c10 <-> c11 (axis "t")."""
    order = (1, 0, 3, 2) if axis == "s" else (2, 3, 0, 1)
    return np.concatenate([patches[c * D:(c + 1) * D] for c in order], axis=0)


def mirror_cells(qs, qt, axis):
    """perm with: cell k of the mirrored patch is cell perm[k] of the patch."""
    return np.array([(qs - 1 - i if axis == "s" else i) + qs * (qt - 1 - j if axis == "t" else j) for j in range(qt) for i in range(qs)])
