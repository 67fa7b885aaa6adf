"""Generates cov_fixtures.npz: the joint posterior of two small GP problems as scikit-learn computes it
(GaussianProcessRegressor.predict(return_cov=True) with fixed hyper-parameters), a third opinion for tests/test_gpu_posterior.py
that shares no code with this project.  Run once; the .npz is committed.

    python tests/golden/make_cov_fixtures.py
"""
import os

import numpy as np
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern


def case(name, kernel_id, N=30, M=40, D=4, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    Xs = rng.uniform(0.0, 1.0, (D, M))
    y = np.sin(3.0 * X.sum(axis=0)) + 0.05 * rng.standard_normal(N)
    a, b = 0.7, 0.01
    ell = rng.uniform(0.3, 0.8, D)
    base = RBF(ell, "fixed") if kernel_id == 0 else Matern(ell, "fixed", nu=2.5)
    gp = GaussianProcessRegressor(ConstantKernel(a, "fixed") * base, alpha=b, optimizer=None).fit(X.T, y)
    mu, cov = gp.predict(Xs.T, return_cov=True)
    return {f"{name}_X": X, f"{name}_y": y, f"{name}_Xs": Xs, f"{name}_theta": np.concatenate([[a], ell]),
            f"{name}_b": np.array(b), f"{name}_kernel": np.array(kernel_id), f"{name}_mu": mu, f"{name}_cov": cov}


if __name__ == "__main__":
    out = {}
    out.update(case("se", 0, seed=7))
    out.update(case("matern", 1, seed=11))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "cov_fixtures.npz"), **out)
