"""Restatement of the two kernels of the *_sub entry points (csrc/kernels_sub.hip; include/sls_hip.h "maximisation over affine
subspaces") in numpy, with the contract's loop orders: every product is rounded before it is added (numpy never fuses), so the
results are the device's to the bit.  A is (n_maps, D, d), c is (n_maps, D), map_of_column one map per column."""
import numpy as np


def _maps(A, c, map_of_column, M):
    A, c = np.asarray(A, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if A.ndim == 2:
        A, c = A[None], c.reshape(1, -1)
    k = np.zeros(M, dtype=np.int64) if map_of_column is None else np.asarray(map_of_column, dtype=np.int64)
    assert k.shape == (M,) and k.min() >= 0 and k.max() < A.shape[0]
    return A[k], c[k]                                       # (M, D, d), (M, D)


def expand(A, c, map_of_column, Z):
    """x_r = c_r, then x_r = x_r + (A_rj z_j) for j = 0..d-1 in increasing order.  Z is d x M; returns D x M.  No clamp."""
    Z = np.asarray(Z, dtype=np.float64)
    Ak, ck = _maps(A, c, map_of_column, Z.shape[1])
    x = ck.T.copy()
    for j in range(Ak.shape[2]):
        x = x + Ak[:, :, j].T * Z[j][None, :]
    return np.asfortranarray(x)


def fold(A, c, map_of_column, GX):
    """gz_j = 0, then gz_j = gz_j + (A_rj gx_r) for r = 0..D-1 in increasing order.  GX is D x M; returns d x M."""
    GX = np.asarray(GX, dtype=np.float64)
    Ak, _ = _maps(A, c, map_of_column, GX.shape[1])
    gz = np.zeros((Ak.shape[2], GX.shape[1]))
    for r in range(Ak.shape[1]):
        gz = gz + Ak[:, r, :].T * GX[r][None, :]
    return np.asfortranarray(gz)


def composed(evaluate_x, A, c, map_of_start):
    """The objective of lbfgs_ref.run(..., with_live=True) in the variables z: evaluate_x(X) -> (val, grad_x) at x = c + A z."""
    map_of_start = np.asarray(map_of_start)

    def evaluate(T, live):
        k = map_of_start[live]
        val, gx = evaluate_x(expand(A, c, k, T))
        return val, fold(A, c, k, gx)
    return evaluate
