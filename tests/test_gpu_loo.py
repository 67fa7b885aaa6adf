"""Leave-one-out cross-validation on the device (sls_nll_loo, sls_gp_loo_grad, sls_gp_loo; kernels_loo.hip) against tests/loo_ref.py
and, where it has the case, the 50-digit fixture tests/golden/loo_terms.npz.  Shapes: where the kernels can go wrong (loo_ref.SHAPES),
both kernels, b = 0.005 and 1e-6; tests/test_loo_cpu.py holds every problem to cond(K_y) <= 1e6, where numpy itself is within 3e-12 of
mpmath.  Tolerances: those of tests/test_gpu_parity.py for the same quantities -- value rtol 1e-9; mu, var, logp rtol 1e-7 with atol
1e-9 max|.|; gradients rtol 1e-6 with atol 1e-6 max|g|.  The scale of mu's absolute tolerance is max(|mu|, |y|): mu_-i = y_i - alpha_i /
d_i is a difference of two numbers of the size of y_i (at N = 1 it is exactly 0 and both sides return a last-place residue of y_1)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import loo_ref
from util import env_switch, sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, D, N, b) for k in (0, 1) for (D, N) in loo_ref.SHAPES for b in loo_ref.NOISES]


@pytest.fixture(scope="module")
def ctx():
    c = sls().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "loo_terms.npz"))
    return {str(n): {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(str(n) + "/")} for n in z["cases"]}


_ref_cache = {}


def reference(kernel, D, N, b):
    """loo_ref's values of one case, computed once and shared."""
    key = (kernel, D, N, b)
    if key not in _ref_cache:
        X, y, theta = loo_ref.problem(D, N)
        mu, var, logp, L = loo_ref.loo_terms(kernel, X, y, theta, b)
        gth, gb = loo_ref.loo_grad_weight(kernel, X, y, theta, b)
        for a in (mu, var, logp, gth):
            a.setflags(write=False)
        _ref_cache[key] = dict(X=X, y=y, theta=theta, mu=mu, var=var, logp=logp, L=L, grad_theta=gth, grad_b=gb)
    return _ref_cache[key]


def check_vectors(r, mu, var, logp, y):
    for got, want, scale in ((r["mu"], mu, max(np.abs(mu).max(), np.abs(y).max())), (r["var"], var, np.abs(var).max()),
                             (r["logp"], logp, np.abs(logp).max())):
        np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-9 * scale)


def check_gradient(gth, gb, want_th, want_b):
    got, want = np.concatenate([gth, [gb]]), np.concatenate([want_th, [want_b]])
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())


def same_bits(r1, r2, grad=True):
    keys = ("mu", "var", "logp") + (("grad_theta",) if grad else ())
    return all(np.array_equal(r1[k], r2[k]) for k in keys) and r1["value"] == r2["value"] and (not grad or r1["grad_b"] == r2["grad_b"])


@pytest.mark.parametrize("kernel,D,N,b", CASES)
def test_loo_matches_reference(ctx, fixture, kernel, D, N, b):
    ref = reference(kernel, D, N, b)
    X, y, theta = ref["X"], ref["y"], ref["theta"]
    h = sls().Nll(ctx, X, kernel)
    try:
        before = h.eval(y, theta, b)
        r = h.loo(y, theta, b)                        # a fresh factor for N <= 128 (sls_nll_eval ran in one workgroup), cached beyond
        r2 = h.loo(y, theta, b)                       # the cached factor
        rv = h.loo(y, theta, b, want_grad=False)
        after = h.eval(y, theta, b)
        h2 = sls().Nll(ctx, X, kernel)
        rf = h2.loo(y, theta, b)                      # a fresh factor on a new handle
        h2.close()
    finally:
        h.close()
    assert abs(r["value"] - ref["L"]) <= 1e-9 * abs(ref["L"])
    check_vectors(r, ref["mu"], ref["var"], ref["logp"], y)
    check_gradient(r["grad_theta"], r["grad_b"], ref["grad_theta"], ref["grad_b"])
    name = f"k{kernel}_D{D}_N{N}_b{b:g}"
    if name in fixture:
        f = fixture[name]
        assert abs(r["value"] - float(f["L"])) <= 1e-9 * abs(float(f["L"]))
        check_vectors(r, f["mu"], f["var"], f["logp"], y)
        check_gradient(r["grad_theta"], r["grad_b"], f["grad_theta"], float(f["grad_b"]))
    # bits: repeated call, cached against fresh factor, value-only against gradient call, the fixed-order sum, sls_nll_eval untouched
    assert same_bits(r, r2) and same_bits(r, rf)
    assert same_bits(r, rv, grad=False)
    assert abs(r["value"] - math.fsum(r["logp"])) <= N * 2.3e-16 * np.sum(np.abs(r["logp"]))
    for k in ("quad", "logdet", "grad_b"):
        assert before[k] == after[k]
    assert np.array_equal(before["alpha"], after["alpha"]) and np.array_equal(before["grad_theta"], after["grad_theta"])
    if N == 1:
        assert abs(r["mu"][0]) <= 1e-9 * abs(y[0]) and abs(r["var"][0] - (theta[0] + b)) <= 1e-7 * (theta[0] + b)


def test_fixture_cases_on_the_device(ctx, fixture):
    """The (8, 40) cases of the fixture, which loo_ref.SHAPES does not hold."""
    for kernel in (0, 1):
        for (D, N, b) in loo_ref.FIXTURE_CASES:
            f = fixture[f"k{kernel}_D{D}_N{N}_b{b:g}"]
            h = sls().Nll(ctx, f["X"], kernel)
            r = h.loo(f["y"], f["theta"], float(f["b"]))
            h.close()
            assert abs(r["value"] - float(f["L"])) <= 1e-9 * abs(float(f["L"]))
            check_vectors(r, f["mu"], f["var"], f["logp"], f["y"])
            check_gradient(r["grad_theta"], r["grad_b"], f["grad_theta"], float(f["grad_b"]))


@pytest.mark.parametrize("kernel", (0, 1))
def test_direct_form(ctx, kernel):
    """One length scale of 0.01 and a near-duplicate pair: the call goes through gram_direct_form (with the guard switched off the
    same call takes the norm expansion and gives other bits)."""
    X, y, theta, b = loo_ref.direct_form_problem()
    mu, var, logp, L = loo_ref.loo_terms(kernel, X, y, theta, b)
    gth, gb = loo_ref.loo_grad_weight(kernel, X, y, theta, b)
    h = sls().Nll(ctx, X, kernel)
    r = h.loo(y, theta, b)
    h.close()
    with env_switch("SLS_GRAM_GUARD", 0):
        h = sls().Nll(ctx, X, kernel)
        r0 = h.loo(y, theta, b)
        h.close()
    assert abs(r["value"] - L) <= 1e-9 * abs(L)
    check_vectors(r, mu, var, logp, y)
    check_gradient(r["grad_theta"], r["grad_b"], gth, gb)
    assert not same_bits(r, r0)


@pytest.mark.parametrize("kernel", (0, 1))
@pytest.mark.parametrize("D,N", [(3, 37), (5, 257)])
def test_gp_loo_both_sigma_modes_and_append(ctx, kernel, D, N):
    """sls_gp_loo on a fitted handle = sls_nll_loo at the same hyper-parameters (rtol 1e-7): explicit inverse, Cholesky solve, and
    after one appended point against a fresh fit of N + 1 points."""
    b = 0.005
    X, y, theta = loo_ref.problem(D, N + 1)
    h = sls().Nll(ctx, X[:, :N], kernel)
    want = h.loo(y[:N], theta, b, want_grad=False)
    h.close()
    h = sls().Nll(ctx, X, kernel)
    want1 = h.loo(y, theta, b, want_grad=False)
    h.close()
    for mode in (sls().SIGMA_EXPLICIT_INVERSE, sls().SIGMA_CHOLESKY_SOLVE):
        gp = sls().GP(ctx, X[:, :N], y[:N], theta, b, kernel)
        gp.set_sigma_mode(mode)
        got = gp.loo()
        gp.append_point(X[:, N], y[N])
        got1 = gp.loo()
        gp.close()
        fresh = sls().GP(ctx, X, y, theta, b, kernel)
        fresh.set_sigma_mode(mode)
        gotf = fresh.loo()
        fresh.close()
        for g, w in ((got, want), (got1, want1), (gotf, want1)):
            for a, k in zip(g, ("mu", "var", "logp")):
                np.testing.assert_allclose(a, w[k], rtol=1e-7, atol=1e-9 * max(np.abs(w[k]).max(), np.abs(y).max() if k == "mu" else 0.0))


@pytest.mark.parametrize("kernel", (0, 1))
def test_outlier_has_the_largest_standardised_residual(ctx, kernel):
    X, y, theta = loo_ref.problem(3, 37)
    b, i = 0.005, 11
    y = y.copy()
    y[i] += 20.0 * math.sqrt(b)
    mu, var, _, _ = loo_ref.loo_terms(kernel, X, y, theta, b)
    assert int(np.argmax(np.abs(y - mu) / np.sqrt(var))) == i
    h = sls().Nll(ctx, X, kernel)
    r = h.loo(y, theta, b, want_grad=False)
    h.close()
    assert int(np.argmax(np.abs(y - r["mu"]) / np.sqrt(r["var"]))) == i
    gp = sls().GP(ctx, X, y, theta, b, kernel)
    m, v, _ = gp.loo()
    gp.close()
    assert int(np.argmax(np.abs(y - m) / np.sqrt(v))) == i


@pytest.mark.parametrize("kernel", (0, 1))
@pytest.mark.parametrize("D,N", [(3, 37), (17, 129)])
def test_gp_loo_objective(ctx, kernel, D, N):
    """sls_gp_loo_grad: L plus the log-normal priors and its gradient in x = (a, b, r_1..r_D); NULL grad; an invalid x is refused."""
    X, y, theta = loo_ref.problem(D, N)
    x = np.concatenate([[theta[0], 0.005], theta[1:]])
    val, g = loo_ref.gp_loo_objective(kernel, X, y, x)
    h = sls().Nll(ctx, X, kernel)
    try:
        v1, g1 = h.gp_loo_objective(y, x)
        v0 = h.gp_loo_objective(y, x, want_grad=False)
        assert abs(v1 - val) <= 1e-9 * abs(val) and v0 == v1
        np.testing.assert_allclose(g1, g, rtol=1e-6, atol=1e-6 * np.abs(g).max())
        for p, bad in ((0, 0.0), (0, -1.0), (1, -1e-3), (2, 0.0), (1 + D, -0.5)):
            xb = x.copy()
            xb[p] = bad
            with pytest.raises(sls().SlsError):
                h.gp_loo_objective(y, xb)
        yb = C.c_double()
        assert sls().lib().sls_gp_loo_grad(h.h, None, x.ctypes.data_as(C.POINTER(C.c_double)), C.byref(yb), None) != 0
        assert h.gp_loo_objective(y, x, want_grad=False) == v1          # the handle is still good
    finally:
        h.close()


def test_not_positive_definite_is_reported(ctx):
    """Duplicate points without noise: SLS_ERR_NOT_SPD as from sls_nll_eval, and the handle keeps working."""
    X, y, theta = loo_ref.problem(3, 37)
    X = X.copy(order="F")
    X[:, 20:28] = X[:, 4:12]
    h = sls().Nll(ctx, X, 0)
    try:
        with pytest.raises(sls().SlsError, match="positive definite"):
            h.loo(y, theta, 0.0)
        r = h.loo(y, theta, 0.005)
        assert np.all(np.isfinite(r["logp"])) and np.all(np.isfinite(r["grad_theta"]))
    finally:
        h.close()


def test_profiler_scopes(ctx):
    """A value-only call launches neither the symmetric product nor the weight kernel."""
    X, y, theta = loo_ref.problem(17, 129)
    h = sls().Nll(ctx, X, 1)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        h.loo(y, theta, 0.005, want_grad=False)
        assert ctx.prof_get("loo_terms")[1] == 1 and ctx.prof_get("loo_syrk")[1] == 0 and ctx.prof_get("loo_weight")[1] == 0
        h.loo(y, theta, 0.005)
        assert ctx.prof_get("loo_terms")[1] == 2 and ctx.prof_get("loo_syrk")[1] == 1 and ctx.prof_get("loo_weight")[1] == 1
    finally:
        ctx.prof_enable(False)
        h.close()
