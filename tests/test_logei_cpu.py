"""CPU-side checks of log expected improvement: the numpy restatement (tests/logei_ref.py) against 60-digit values
(tests/golden/logei_terms.npz, make_logei_fixtures.py), its agreement with expected improvement where that is sound, its gradient
against central differences on a 2-D toy posterior, the guard, and the package's bindings."""
import ctypes as C
import os
import re

import numpy as np
from scipy.special import erfc

import logei_ref
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def terms_errors(u, got, want):
    """Largest error / bound of (log h, B1, B2) against the fixtures, with the bounds of the device test: log h within
    16 eps max(1, u^2); B1, B2 within 1e-12 relative + 1e-300 absolute (phi underflows for u > 38: B2 is 0 there against a true value
    that no double holds)."""
    ratios = [np.abs(got[0] - want[0]) / (16 * EPS * np.maximum(1.0, u * u))]
    ratios += [np.abs(g - w) / (1e-12 * np.abs(w) + 1e-300) for g, w in zip(got[1:], want[1:])]
    msg = "; ".join(f"{name}: {r.max():.3g} of its bound at u = {u[r.argmax()]:.6g}" for name, r in zip(("log h", "B1", "B2"), ratios))
    return ratios, msg


def load_fixtures():
    z = np.load(os.path.join(ROOT, "tests", "golden", "logei_terms.npz"))
    return z["u"], (z["log_h"], z["b1"], z["b2"])


def test_restatement_agrees_with_60_digit_values():
    u, want = load_fixtures()
    assert u.size == 1130 and u.min() == -1e12 and u.max() == 1e10 and (u == 0).sum() >= 1 and (u == -38.6).sum() == 1
    assert (u == -30.0).sum() >= 1 and (u == np.nextafter(-30.0, -np.inf)).sum() == 1 and (u == np.nextafter(-30.0, 0.0)).sum() == 1
    assert all(np.all(np.isfinite(w)) for w in want)
    ratios, msg = terms_errors(u, logei_ref.terms(u), want)
    print(msg)
    for r in ratios:
        assert np.all(r <= 1.0), msg


def test_direct_expected_improvement_is_dead_where_logei_is_not():
    """The point of the feature: the direct form underflows to exactly 0 below u ~ -38.6 and has lost log EI = -730.2 to -722.9 at
    u = -38; the log-space form has neither problem."""
    u, want = load_fixtures()
    with np.errstate(all="ignore"):
        direct = u * 0.5 * erfc(-u / np.sqrt(2.0)) + np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)
    dead = u < -39.0
    assert dead.sum() > 100 and np.all(direct[dead] == 0.0) and np.all(np.isfinite(logei_ref.terms(u[dead])[0]))
    at = np.array([-38.0])
    with np.errstate(all="ignore"):
        d38 = np.log(at * 0.5 * erfc(-at / np.sqrt(2.0)) + np.exp(-0.5 * at * at) / np.sqrt(2.0 * np.pi))[0]
    assert abs(logei_ref.terms(at)[0][0] - (-730.2)) < 0.05 and abs(d38 - logei_ref.terms(at)[0][0]) > 1.0
    # where the direct form is sound the two agree: its cancellation is ~u^2 eps
    ok = (u >= -20.0) & (u <= 30.0)
    np.testing.assert_allclose(np.exp(logei_ref.terms(u[ok])[0]), direct[ok], rtol=1e-10)


def toy_posterior(X):
    """A smooth 2-D stand-in for (mu, sigma, dmu, dsigma): X is (2, M)."""
    x, y = X
    mu = np.sin(3.0 * x) * np.cos(2.0 * y) + 0.3 * x
    dmu = np.stack([3.0 * np.cos(3.0 * x) * np.cos(2.0 * y) + 0.3, -2.0 * np.sin(3.0 * x) * np.sin(2.0 * y)])
    sigma = 0.02 + 0.015 * np.sin(2.0 * x + y) ** 2
    ds = 0.03 * np.sin(2.0 * x + y) * np.cos(2.0 * x + y)
    dsigma = np.stack([2.0 * ds, ds])
    return mu, sigma, dmu, dsigma


def test_gradient_against_central_differences():
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (2, 60))
    mu_best = 0.9
    mu, sigma, dmu, dsigma = toy_posterior(X)
    val, grad, info = logei_ref.logei(mu, sigma, mu_best, dmu, dsigma)
    assert (info["u"] < -30).any() and (info["u"] > 0).any() and ((info["u"] < 0) & (info["u"] > -30)).any() and not info["bad"].any()
    h = 1e-6
    for d in range(2):
        E = np.zeros((2, 1))
        E[d] = h
        vp = logei_ref.logei(*toy_posterior(X + E)[:2], mu_best)[0]
        vm = logei_ref.logei(*toy_posterior(X - E)[:2], mu_best)[0]
        fd = (vp - vm) / (2 * h)
        # second differences of a value ~u^2 / 2 over h: the rounding of the values, |val| eps / h, on top of the h^2 term
        assert np.all(np.abs(fd - grad[d]) <= 1e-6 * (1.0 + np.abs(grad).max()) + 4 * EPS * np.abs(val) / h)


def test_guard():
    mu = np.array([0.2, 0.2, 0.2, np.nan])
    sigma = np.array([0.3, 5e-11, 0.3, 0.3])
    dmu = np.ones((3, 4))
    dsigma = np.ones((3, 4))
    dsigma[1, 2] = np.nan
    val, grad, info = logei_ref.logei(mu, sigma, 0.5, dmu, dsigma)
    assert np.isfinite(val[0]) and val[0] > logei_ref.FLOOR and np.all(grad[:, 0] != 0)
    assert np.array_equal(val[1:], np.full(3, -1.0e300)) and np.array_equal(grad[:, 1:], np.zeros((3, 3)))
    # without a gradient only the value decides
    val2 = logei_ref.logei(mu, sigma, 0.5)[0]
    assert val2[0] == val[0] and val2[1] == -1.0e300 and val2[2] == val[0] and val2[3] == -1.0e300


def test_package_binds_the_acquisition_type_and_the_hook():
    m = sls()
    assert m.ACQ_LOG_EI == 2 and (m.ACQ_EI, m.ACQ_UCB) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    assert "sls_logei_terms" in m.EXPORTS and re.search(r"\bint sls_logei_terms\(", hdr)
    assert re.search(r"#define SLS_ACQ_LOG_EXPECTED_IMPROVEMENT 2\b", hdr) and re.search(r"#define SLS_LOG_EI_FLOOR \(-1\.0e300\)", hdr)
    assert callable(m.Context.logei_terms)
    assert hasattr(m.lib(), "sls_logei_terms")                        # the symbol is exported


def test_null_handle_is_refused_without_a_gpu():
    lib = sls().lib()
    lib.sls_last_error.restype = C.c_char_p
    u = np.zeros(3)
    out = np.empty(3)
    dp = C.POINTER(C.c_double)
    assert lib.sls_logei_terms(None, u.ctypes.data_as(dp), C.c_long(3), out.ctypes.data_as(dp), None, None) == -1
    assert b"ctx is NULL" in lib.sls_last_error()
    for acq in (2, 3):
        assert lib.sls_acq_eval(None, acq, C.c_double(1.0), u.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), None) == -1
