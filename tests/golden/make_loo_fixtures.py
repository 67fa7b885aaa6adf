"""Generates tests/golden/loo_terms.npz: 50-digit mpmath values of the leave-one-out quantities of tests/loo_ref.py -- mu_-i, var_-i,
logp_i, L and all D + 2 derivatives of L (a, r_1..r_D, b), the derivatives in GPML's per-parameter form (eq. 5.13) -- for both kernels
on loo_ref.FIXTURE_CASES, and tests/golden/loo_illcond.npz: the same quantities plus cond(K_y) on the conditioning ladder loo_ref.RUNGS,
the derivatives there in the weight form (one product M = K_y^-1 diag(c) K_y^-1 for all parameters, every step at 50 digits; minutes
at N = 130).  A file whose regenerated values equal the committed ones is left as it is.  Needs mpmath (1.3.0 when the committed
files were made); run from the repository root:

    python tests/golden/make_loo_fixtures.py
"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import loo_ref  # noqa: E402

mp.mp.dps = 50


def kernel_and_derivatives(kernel, X, theta):
    D, N = X.shape
    a = mp.mpf(float(theta[0]))
    ell = [mp.mpf(float(v)) for v in theta[1:]]
    Xm = [[mp.mpf(float(X[d, i])) for i in range(N)] for d in range(D)]
    K = mp.zeros(N, N)
    dK = [mp.zeros(N, N) for _ in range(D + 1)]
    for i in range(N):
        for j in range(N):
            diffs = [Xm[d][i] - Xm[d][j] for d in range(D)]
            q = sum((diffs[d] / ell[d]) ** 2 for d in range(D))
            if kernel == 0:
                k = a * mp.exp(-q / 2)
                c = k
            else:
                s = mp.sqrt(5 * q)
                k = a * (1 + s + mp.mpf(5) / 3 * q) * mp.exp(-s)
                c = a * mp.mpf(5) / 3 * (1 + s) * mp.exp(-s)
            K[i, j] = k
            dK[0][i, j] = k / a
            for d in range(D):
                dK[1 + d][i, j] = c * diffs[d] ** 2 / ell[d] ** 3
    return K, dK


def cholesky_inverse(Ky, N):
    """K_y^-1 of a positive definite K_y as rows of mpf, from its Cholesky factor; raises where a pivot is not positive."""
    L = [[mp.mpf(0)] * N for _ in range(N)]
    for j in range(N):
        piv = Ky[j, j] - mp.fsum(L[j][k] ** 2 for k in range(j))
        if piv <= 0:
            raise ArithmeticError("K_y is not positive definite at 50 digits")
        L[j][j] = mp.sqrt(piv)
        for i in range(j + 1, N):
            L[i][j] = (Ky[i, j] - mp.fdot(L[i][:j], L[j][:j])) / L[j][j]
    T = [[mp.mpf(0)] * N for _ in range(N)]                    # T = L^-1, lower triangular
    for j in range(N):
        T[j][j] = 1 / L[j][j]
        for i in range(j + 1, N):
            T[i][j] = -mp.fdot(L[i][j:i], [T[k][j] for k in range(j, i)]) / L[i][i]
    Tc = [[T[k][i] for k in range(N)] for i in range(N)]       # columns of T
    inv = [[None] * N for _ in range(N)]
    for i in range(N):
        for j in range(i + 1):
            inv[i][j] = inv[j][i] = mp.fdot(Tc[i][i:], Tc[j][i:])
    return inv


def cond_2(Ky):
    """cond_2(K_y) = lambda_max / lambda_min of the symmetric matrix, at 50 digits."""
    ev = mp.eigsy(Ky, eigvals_only=True)
    return max(ev) / min(ev)


def rung(kernel, D, N, s, b):
    """One rung of the conditioning ladder: the derivatives as sum_ij W_ij dK_ij/dtheta_p with W = 1/2 (u alpha^T + alpha u^T) - M."""
    X, y, theta = loo_ref.scaled_problem(D, N, s)
    K, dK = kernel_and_derivatives(kernel, X, theta)
    Ky = K + mp.mpf(float(b)) * mp.eye(N)
    Kinv = cholesky_inverse(Ky, N)
    ym = [mp.mpf(float(v)) for v in y]
    alpha = [mp.fdot(Kinv[i], ym) for i in range(N)]
    d = [Kinv[i][i] for i in range(N)]
    mu = [ym[i] - alpha[i] / d[i] for i in range(N)]
    var = [1 / d[i] for i in range(N)]
    logp = [mp.log(d[i]) / 2 - alpha[i] ** 2 / (2 * d[i]) - mp.log(2 * mp.pi) / 2 for i in range(N)]
    u = [mp.fdot(Kinv[i], [alpha[k] / d[k] for k in range(N)]) for i in range(N)]
    c = [(1 + alpha[i] ** 2 / d[i]) / (2 * d[i]) for i in range(N)]
    scaled = [[Kinv[i][k] * c[k] for k in range(N)] for i in range(N)]
    grads = [mp.mpf(0)] * (D + 2)
    for i in range(N):
        for j in range(i + 1):
            w = (u[i] * alpha[j] + alpha[i] * u[j]) / 2 - mp.fdot(scaled[i], Kinv[j])
            if i == j:
                grads[D + 1] += w
            else:
                w = 2 * w                                       # W and every dK_p are symmetric
            for p in range(D + 1):
                grads[p] += w * dK[p][i, j]
    f = lambda v: np.array([float(t) for t in v])
    return dict(X=X, y=y, theta=theta, b=float(b), mu=f(mu), var=f(var), logp=f(logp), L=float(mp.fsum(logp)),
                grad_theta=f(grads[:-1]), grad_b=float(grads[-1]), cond=float(cond_2(Ky)))


def case(kernel, D, N, b):
    X, y, theta = loo_ref.problem(D, N)
    K, dK = kernel_and_derivatives(kernel, X, theta)
    Ky = K + mp.mpf(float(b)) * mp.eye(N)
    Kinv = mp.inverse(Ky)
    ym = mp.matrix([mp.mpf(float(v)) for v in y])
    alpha = Kinv * ym
    d = [Kinv[i, i] for i in range(N)]
    mu = [ym[i] - alpha[i] / d[i] for i in range(N)]
    var = [1 / d[i] for i in range(N)]
    logp = [mp.log(d[i]) / 2 - alpha[i] ** 2 / (2 * d[i]) - mp.log(2 * mp.pi) / 2 for i in range(N)]
    grads = []
    for dKp in dK + [mp.eye(N)]:
        Z = Kinv * dKp
        Za = Z * alpha
        ZK = Z * Kinv
        grads.append(sum((alpha[i] * Za[i] - (1 + alpha[i] ** 2 / d[i]) * ZK[i, i] / 2) / d[i] for i in range(N)))
    f = lambda v: np.array([float(t) for t in v])
    return dict(X=X, y=y, theta=theta, b=float(b), mu=f(mu), var=f(var), logp=f(logp), L=float(sum(logp)),
                grad_theta=f(grads[:-1]), grad_b=float(grads[-1]))


def save_if_changed(name, out):
    """Writes tests/golden/<name> unless the committed file already holds exactly these arrays."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    if os.path.exists(path):
        old = np.load(path)
        if sorted(old.files) == sorted(out) and all(np.array_equal(old[k], np.asarray(out[k])) for k in out):
            print(name, "unchanged")
            return
    np.savez(path, **out)
    print(name, "written")


def main():
    out = {}
    names = []
    for kernel in (0, 1):
        for (D, N, b) in loo_ref.FIXTURE_CASES:
            name = f"k{kernel}_D{D}_N{N}_b{b:g}"
            names.append(name)
            for key, val in case(kernel, D, N, b).items():
                out[f"{name}/{key}"] = val
            print(name, "L =", out[f"{name}/L"])
    out["cases"] = np.array(names)
    save_if_changed("loo_terms.npz", out)
    out = {}
    names = []
    for r in loo_ref.RUNGS:
        name = loo_ref.rung_name(*r)
        names.append(name)
        for key, val in rung(*r).items():
            out[f"{name}/{key}"] = val
        print(name, "L =", out[f"{name}/L"], "cond = %.3g" % out[f"{name}/cond"], flush=True)
    out["cases"] = np.array(names)
    save_if_changed("loo_illcond.npz", out)


if __name__ == "__main__":
    main()
