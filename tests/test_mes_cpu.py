"""CPU-side checks of max-value entropy search: the numpy restatement (tests/mes_ref.py) against 60-digit values
(tests/golden/mes_terms.npz, make_mes_fixtures.py), its gradient against central differences on a 2-D toy posterior, the guard, and
the package's bindings of the three entry points."""
import os
import re

import numpy as np

import mes_ref
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def test_restatement_agrees_with_60_digit_values():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mes_terms.npz"))
    t, g, dg = z["t"], z["g"], z["dg"]
    assert t.size == 222 and t.min() == -1e4 and abs(t.max() - 38.0) < 1e-12 and (t == 0).sum() == 1
    gv, dv = mes_ref.terms(t)
    err_g = np.abs(gv - g) / (EPS * np.maximum(1.0, t * t))
    err_d = np.abs(dv - dg) / (np.abs(dg) + 1e-300)
    msg = f"largest value error {err_g.max():.2f} eps max(1, t^2) at t = {t[err_g.argmax()]:.4g}; largest g' error {err_d.max():.3g} at t = {t[err_d.argmax()]:.4g}"
    assert np.all(np.abs(gv - g) <= 16 * EPS * np.maximum(1.0, t * t)), msg
    # 1e-9: ten times the t^4 eps / 2 that the direct form of 1 + t (t + r) has lost at the switch to the series, t = -30
    assert np.all(np.abs(dv - dg) <= 1e-9 * np.abs(dg) + 1e-300), msg


def toy_posterior(X):
    """A smooth 2-D stand-in for (mu, sigma, dmu, dsigma): X is (2, M)."""
    x, y = X
    mu = np.sin(3.0 * x) * np.cos(2.0 * y) + 0.3 * x
    dmu = np.stack([3.0 * np.cos(3.0 * x) * np.cos(2.0 * y) + 0.3, -2.0 * np.sin(3.0 * x) * np.sin(2.0 * y)])
    sigma = 0.2 + 0.15 * np.sin(2.0 * x + y) ** 2
    ds = 0.3 * np.sin(2.0 * x + y) * np.cos(2.0 * x + y)
    dsigma = np.stack([2.0 * ds, ds])
    return mu, sigma, dmu, dsigma


def test_gradient_against_central_differences():
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (2, 40))
    y_star = np.concatenate([1.3 + 0.2 * rng.standard_normal(12), [-0.4, 0.1]])   # some below mu: gamma < 0 occurs
    mu, sigma, dmu, dsigma = toy_posterior(X)
    val, grad, info = mes_ref.alpha(mu, sigma, y_star, dmu, dsigma)
    assert (info["gamma"] < 0).any() and (info["gamma"] > 0).any() and not info["bad"].any()
    h = 1e-6
    for d in range(2):
        E = np.zeros((2, 1))
        E[d] = h
        vp = mes_ref.alpha(*toy_posterior(X + E)[:2], y_star)[0]
        vm = mes_ref.alpha(*toy_posterior(X - E)[:2], y_star)[0]
        fd = (vp - vm) / (2 * h)
        assert np.abs(fd - grad[d]).max() <= 1e-6 * (1.0 + np.abs(grad).max())


def test_guard():
    y_star = np.array([1.0, 1.5])
    mu = np.array([0.2, 0.2, 0.2, np.nan])
    sigma = np.array([0.3, 5e-11, 0.3, 0.3])
    dmu = np.ones((3, 4))
    dsigma = np.ones((3, 4))
    dsigma[1, 2] = np.nan
    val, grad, info = mes_ref.alpha(mu, sigma, y_star, dmu, dsigma)
    assert val[0] > 0 and np.all(grad[:, 0] != 0)
    assert np.array_equal(val[1:], np.zeros(3)) and np.array_equal(grad[:, 1:], np.zeros((3, 3)))
    # without a gradient only the value decides
    val2 = mes_ref.alpha(mu, sigma, y_star)[0]
    assert val2[0] == val[0] and val2[1] == 0 and val2[2] == val[0] and val2[3] == 0


def test_package_binds_the_three_entry_points():
    m = sls()
    names = ("sls_mes_terms", "sls_mes_eval", "sls_mes_maximize")
    hdr = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    for n in names:
        assert n in m.EXPORTS and re.search(r"\bint " + n + r"\(", hdr)
    assert re.search(r"#define SLS_MES_MAX_SAMPLES 4096\b", hdr)
    assert callable(m.GP.mes_eval) and callable(m.GP.mes_maximize) and callable(m.mes_terms) and callable(m.Context.mes_terms)
