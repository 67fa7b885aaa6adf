"""Joint entropy search without a GPU: the numpy restatement (tests/jes_ref.py) against central differences, against a from-scratch
GP on the data plus one optimum, against a Monte-Carlo truncated normal, its degenerate rules, and its own float64 error against the
60-digit fixtures (the yardstick of the device tests in tests/test_gpu_jes.py)."""
import os

import numpy as np
import pytest

import gram_ref
import jes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SE, MATERN52 = 0, 1


def small_problem(kernel, D=3, N=12, K=5, seed=0, b=0.01):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (D, N))
    y = np.sin(3.0 * X.sum(axis=0)) + 0.05 * rng.standard_normal(N)
    ell = 0.4 * rng.uniform(0.8, 1.25, D)
    f = gram_ref.fit(X, y, ell, 0.7, b, kernel)
    x_star = rng.uniform(0, 1, (D, K))
    f_star = y.max() + 0.2 * np.abs(rng.standard_normal(K))
    f_star[1] = y.mean() - 0.3                     # an optimum value below the posterior mean: gamma < 0
    return f, x_star, f_star, rng


@pytest.mark.parametrize("kernel", [SE, MATERN52])
def test_gradient_against_central_differences(kernel):
    f, x_star, f_star, rng = small_problem(kernel)
    o = jes_ref.condition(f, x_star, f_star, 1e-6)
    Xs = rng.uniform(0.05, 0.95, (3, 9))
    val, grad, info = jes_ref.evaluate(f, o, Xs, noise_var=0.01)
    assert not info["bad"].any() and (info["gamma"] < 0).any() and (info["gamma"] > 0).any()
    h = 1e-6
    for d in range(3):
        E = np.zeros_like(Xs)
        E[d] = h
        fd = (jes_ref.evaluate(f, o, Xs + E, 0.01, False)[0] - jes_ref.evaluate(f, o, Xs - E, 0.01, False)[0]) / (2 * h)
        err = np.abs(fd - grad[d]).max()
        print(f"kernel {kernel} d {d}: central differences {err:.3g} (|grad| max {np.abs(grad).max():.3g})")
        # truncation h^2 |f'''| / 6 ~ 1e-12 x 1e3 and rounding eps |f| / h ~ 1e-10
        assert err <= 1e-7 * (1.0 + np.abs(grad).max())


@pytest.mark.parametrize("kernel", [SE, MATERN52])
def test_rank_one_conditioning_is_a_gp_on_the_data_plus_the_optimum(kernel):
    b = 0.01
    f, x_star, f_star, rng = small_problem(kernel, b=b)
    o = jes_ref.condition(f, x_star, f_star, star_noise=b)
    Xs = rng.uniform(0, 1, (3, 7))
    p = gram_ref.predict(f, Xs)
    cov = jes_ref.covariances(f, o, Xs)
    for k in range(f_star.size):
        X2 = np.concatenate([f["X"], o["xs"][:, k:k + 1]], axis=1)
        y2 = np.concatenate([f["y"], [f_star[k]]])
        p2 = gram_ref.predict(gram_ref.fit(X2, y2, f["ell"], f["a"], b, kernel), Xs)
        m_k = p["mean"] + cov[:, k] / o["v"][k] * o["d"][k]
        s2_k = p["dev"] ** 2 - cov[:, k] ** 2 / o["v"][k]
        cond = np.linalg.cond(f["K"])
        tol = 64 * cond * EPS * (1.0 + np.abs(f["alpha"]).max())
        assert np.abs(m_k - p2["mean"]).max() <= tol and np.abs(s2_k - p2["dev"] ** 2).max() <= tol, (k, cond)


def test_tau_is_the_variance_of_a_truncated_normal():
    rng = np.random.default_rng(5)
    n = 4_000_000
    z = rng.standard_normal(n)
    for t in (-1.0, 0.3, 2.0):
        s = z[z < t]
        # the sample variance of m draws of a distribution with variance tau <= 1 and fourth central moment <= 3 has standard
        # deviation <= sqrt(3 / m); 5 of them
        bound = 5.0 * np.sqrt(3.0 / s.size)
        tau = float(jes_ref.terms(t)[0])
        print(f"t {t}: tau {tau:.6f}, Monte Carlo {s.var():.6f} on {s.size} draws, bound {bound:.2g}")
        assert abs(s.var() - tau) <= bound
        assert abs(tau - float(jes_ref.terms_mp(t)[0])) <= 8 * EPS


def test_degenerate_rules():
    f, x_star, f_star, rng = small_problem(SE, b=1e-6)
    Xs = rng.uniform(0, 1, (3, 4))
    p = gram_ref.predict(f, Xs, want_grad=True)
    # an uninformative optimum (v below the floor): c / v counts as 0, so the term is that of an unconditioned posterior
    o = jes_ref.condition(f, x_star, f_star, 0.0)
    cov, dcov = jes_ref.covariances(f, o, Xs, True)
    v = o["v"].copy()
    v[2] = 1e-21
    val, grad, info = jes_ref.alpha(p["mean"], p["dev"], cov, f_star, o["d"], v, 0.01, p["dmean"], p["ddev"], dcov)
    c0 = cov.copy()
    c0[:, 2] = 0.0
    v1 = v.copy()
    v1[2] = 1.0
    val0, grad0, _ = jes_ref.alpha(p["mean"], p["dev"], c0, f_star, o["d"], v1, 0.01, p["dmean"], p["ddev"], dcov)
    assert np.array_equal(val, val0) and np.all(info["H"][2] == 0.0) and np.all(np.isfinite(grad))
    assert np.allclose(info["s2"][2], p["dev"] ** 2, rtol=0, atol=0)
    # a candidate on an optimum with star_noise = 0: c = v = sigma^2 there, s_k^2 = 0 < floor: the term is log noise_var
    Xo = np.concatenate([o["xs"][:, :1], Xs], axis=1)
    val, grad, info = jes_ref.evaluate(f, o, Xo, 0.01)
    assert abs(info["s2"][0, 0]) < 1e-12 and info["q"][0, 0] == 0.01 and info["H"][0, 0] == 0.0
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    # sigma below the guard: value 0, gradient 0
    sg = p["dev"].copy()
    sg[1] = 5e-11
    val, grad, info = jes_ref.alpha(p["mean"], sg, cov, f_star, o["d"], o["v"], 0.01, p["dmean"], p["ddev"], dcov)
    assert info["bad"][1] and val[1] == 0.0 and np.all(grad[:, 1] == 0.0) and not info["bad"][0]


def test_float64_error_of_the_restatement_against_the_fixtures():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jes_terms.npz"))
    t = z["t"]
    assert 190 <= t.size <= 210 and t.min() == -1e4 and abs(t.max() - 38) < 1e-9
    assert ((t > -30.5) & (t < -29.5)).sum() >= 30 and (np.abs(t) < 0.1).sum() >= 30
    tau, dtau = jes_ref.terms(t)
    e_tau = np.abs(tau - z["tau"]) / (EPS * np.maximum(1.0, t * t))
    e_d = np.abs(dtau - z["dtau"]) / np.abs(z["dtau"])
    print(f"float64 restatement: tau {e_tau.max():.3f} eps max(1, t^2) at t = {t[e_tau.argmax()]:.5g}; "
          f"tau' {e_d.max():.3g} relative at t = {t[e_d.argmax()]:.5g}")
    # the forms of the contract: tau to a few eps max(1, t^2); tau' loses t^6 eps / 2 just above the switch at -30 (1e-7)
    assert e_tau.max() <= 16 and e_d.max() <= 1e-6
    assert np.all((z["tau"] > 0) & (z["tau"] <= 1) & (z["dtau"] > 0))
