"""Generates tests/golden/loo_terms.npz: 50-digit mpmath values of the leave-one-out quantities of tests/loo_ref.py -- mu_-i, var_-i,
logp_i, L and all D + 2 derivatives of L (a, r_1..r_D, b), the derivatives in GPML's per-parameter form (eq. 5.13) -- for both kernels
on loo_ref.FIXTURE_CASES.  Needs mpmath (1.3.0 when the committed file was made); run from the repository root:

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
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "loo_terms.npz"), **out)


if __name__ == "__main__":
    main()
