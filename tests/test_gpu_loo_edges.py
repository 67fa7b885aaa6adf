"""Leave-one-out cross-validation on the device where its first suite (tests/test_gpu_loo.py) does not reach, at that suite's
tolerances and against the same reference (tests/loo_ref.py):

  * the direct Gram form on several tiles (loo_weight_direct_kernel reads M(j, i) for every tile above the diagonal, which
    loo_syrk_kernel never writes), with near-duplicate pairs across every off-diagonal tile;
  * partial outputs: every output pointer of sls_nll_loo alone, none at all, and mixtures -- each a branch of its own in the
    pipeline -- to the bits of the full call, on a fresh and on a cached factor;
  * the cached factor under new targets, a new noise level, new length scales, and sls_nll_eval / sls_pref_objective calls at other
    hyper-parameters in between (they share G, the partial sums, Y and the row sums with LOO): every step to the bits of a fresh handle;
  * SLS_LOO_SYRK=0 (the full product by the generic GEMM); nt = 4 (ten product tiles, the last tile one point); b = 0 where K_f
    alone is positive definite; sls_gp_loo while a handle grows across the 128-point padding, with NULL output pointers and under
    sigma-mode switches."""
import ctypes as C

import numpy as np
import pytest

import loo_ref
from test_gpu_loo import check_gradient, check_vectors, reference, same_bits
from test_gpu_short_length_scales import random_prefs
from util import env_switch, sls

pytestmark = pytest.mark.gpu
OUTPUTS = ("mu", "var", "logp", "value", "grad_theta", "grad_b")


@pytest.fixture(scope="module")
def ctx():
    c = sls().Context(0)
    yield c
    c.close()


def check_against(r, want, y):
    assert abs(r["value"] - want["L"]) <= 1e-9 * abs(want["L"])
    check_vectors(r, want["mu"], want["var"], want["logp"], y)
    check_gradient(r["grad_theta"], r["grad_b"], want["grad_theta"], want["grad_b"])


def loo_once(ctx, X, kernel, y, theta, b, **kw):
    h = sls().Nll(ctx, X, kernel)
    try:
        return h.loo(y, theta, b, **kw)
    finally:
        h.close()


# ---- the direct form on several tiles -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", (0, 1))
@pytest.mark.parametrize("N", (130, 257))
def test_direct_form_on_several_tiles(ctx, kernel, N):
    X, y, theta, b = loo_ref.direct_form_problem_tiled(N)
    mu, var, logp, L = loo_ref.loo_terms(kernel, X, y, theta, b)
    gth, gb = loo_ref.loo_grad_weight(kernel, X, y, theta, b)
    want = dict(mu=mu, var=var, logp=logp, L=L, grad_theta=gth, grad_b=gb)
    r = loo_once(ctx, X, kernel, y, theta, b)
    with env_switch("SLS_GRAM_GUARD", 0):
        r0 = loo_once(ctx, X, kernel, y, theta, b)                       # the norm expansion: other bits, the same tolerances
    check_against(r, want, y)
    check_against(r0, want, y)
    assert not same_bits(r, r0)
    check_gradient(r["grad_theta"], r["grad_b"], *loo_ref.loo_grad_gpml(kernel, X, y, theta, b))   # the algebraically independent form


# ---- partial outputs and the cached factor --------------------------------------------------------------------------------------
HANDLE_CASES = [(0, 17, 129), (1, 17, 129), (0, 5, 257), (1, 5, 257), (1, "direct", 130)]


def handle_problem(D, N):
    if D == "direct":
        return loo_ref.direct_form_problem_tiled(N)
    return loo_ref.problem(D, N) + (0.005,)


def wants(names):
    return {"want_" + k: k in names for k in OUTPUTS}


def same_returned_bits(part, full, names):
    for k in OUTPUTS:
        if k not in names:
            if part[k] is not None:
                return False
        elif not np.array_equal(np.asarray(part[k]), np.asarray(full[k])):
            return False
    return True


# every output alone (grad_b alone, grad_theta alone and the value alone among them), none at all, and mixtures of vectors and gradient
COMBOS = [(k,) for k in OUTPUTS] + [(), ("mu", "grad_b"), ("value", "grad_theta"), ("var", "logp"), ("mu", "var", "logp", "grad_theta", "grad_b"),
                                    ("grad_theta", "grad_b")]


@pytest.mark.parametrize("kernel,D,N", HANDLE_CASES)
def test_partial_outputs_to_the_bit(ctx, kernel, D, N):
    X, y, theta, b = handle_problem(D, N)
    h = sls().Nll(ctx, X, kernel)
    try:
        full = h.loo(y, theta, b)
        for names in COMBOS:
            part = h.loo(y, theta, b, **wants(names))                   # the cached factor
            assert same_returned_bits(part, full, names), names
            assert same_bits(h.loo(y, theta, b), full), names           # the handle repeats the full call
            h2 = sls().Nll(ctx, X, kernel)
            try:
                part2 = h2.loo(y, theta, b, **wants(names))             # a fresh factor behind the same outputs
                assert same_returned_bits(part2, full, names), names
                assert same_bits(h2.loo(y, theta, b), full), names
            finally:
                h2.close()
    finally:
        h.close()


@pytest.mark.parametrize("kernel,D,N", HANDLE_CASES)
def test_cached_factor_against_fresh_handles(ctx, kernel, D, N):
    X, y1, theta, b = handle_problem(D, N)
    rng = np.random.default_rng(7 * N + kernel)
    y2 = y1[::-1].copy() + 0.1 * rng.standard_normal(N)
    theta_new = theta * (1.0 + 0.1 * np.cos(np.arange(theta.size)))
    theta_eval, b_eval = theta * 1.3, 0.02
    prefs = random_prefs(rng, N, 40)
    dims = theta.size - 1
    x_pref = np.concatenate([y2, [0.4, 0.008], np.full(dims, 0.45)])

    def fresh(fn):
        h2 = sls().Nll(ctx, X, kernel)
        try:
            return fn(h2)
        finally:
            h2.close()

    def same_eval(e1, e2):
        return (all(e1[k] == e2[k] for k in ("quad", "logdet", "grad_b")) and np.array_equal(e1["alpha"], e2["alpha"])
                and np.array_equal(e1["grad_theta"], e2["grad_theta"]))

    h = sls().Nll(ctx, X, kernel)
    try:
        steps = [("first", y1, theta, b), ("new y, the factor kept", y2, theta, b), ("the first y again", y1, theta, b), "eval",
                 ("new b", y1, theta, 2.0 * b), "pref", ("new theta", y1, theta_new, b), "eval", ("back to the first", y1, theta, b)]
        for step in steps:
            if step == "eval":
                assert same_eval(h.eval(y2, theta_eval, b_eval), fresh(lambda g: g.eval(y2, theta_eval, b_eval)))
            elif step == "pref":
                v, g = h.pref_objective(prefs, x_pref, use_map=True)
                vf, gf = fresh(lambda g2: g2.pref_objective(prefs, x_pref, use_map=True))
                assert v == vf and np.array_equal(g, gf)
            else:
                what, yy, th, bb = step
                assert same_bits(h.loo(yy, th, bb), fresh(lambda g: g.loo(yy, th, bb))), what
    finally:
        h.close()


# ---- the rest -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", (0, 1))
@pytest.mark.parametrize("D,N", [(5, 257), (17, 129)])
def test_full_product_route(ctx, kernel, D, N):
    """SLS_LOO_SYRK=0: M by the generic GEMM, every tile.  The same tolerances, still one loo_syrk scope, and the terms -- which do
    not pass through M -- to the bit."""
    b = 0.005
    ref = reference(kernel, D, N, b)
    X, y, theta = ref["X"], ref["y"], ref["theta"]
    r = loo_once(ctx, X, kernel, y, theta, b)
    with env_switch("SLS_LOO_SYRK", 0):
        h = sls().Nll(ctx, X, kernel)
        ctx.prof_enable(True)
        try:
            ctx.prof_reset()
            r0 = h.loo(y, theta, b)
            assert ctx.prof_get("loo_syrk")[1] == 1 and ctx.prof_get("loo_weight")[1] == 1 and ctx.prof_get("loo_terms")[1] == 1
        finally:
            ctx.prof_enable(False)
            h.close()
    check_against(r, ref, y)
    check_against(r0, ref, y)
    assert same_bits(r, r0, grad=False)


@pytest.mark.parametrize("kernel", (0, 1))
def test_four_tiles(ctx, kernel):
    """problem(5, 385): nt = 4, ten product tiles in loo_syrk_kernel's triangular decode, the last tile holds one point."""
    b = 0.005
    ref = reference(kernel, 5, 385, b)
    r = loo_once(ctx, ref["X"], kernel, ref["y"], ref["theta"], b)
    check_against(r, ref, ref["y"])


def test_without_noise(ctx):
    """b = 0 where K_f alone is positive definite (Matern 5/2 at (3, 37), cond about 4e2): sls_nll_loo and sls_gp_loo_grad succeed.
    sls_nll_loo is compared in full.  The log-normal prior's density at b = 0 is zero, so the objective's value and its derivative
    in b are no numbers to compare there: the derivatives in a and the length scales are."""
    kernel, b = 1, 0.0
    X, y, theta = loo_ref.problem(3, 37)
    mu, var, logp, L = loo_ref.loo_terms(kernel, X, y, theta, b)
    gth, gb = loo_ref.loo_grad_weight(kernel, X, y, theta, b)
    h = sls().Nll(ctx, X, kernel)
    try:
        r = h.loo(y, theta, b)
        _, g = h.gp_loo_objective(y, np.concatenate([[theta[0], b], theta[1:]]))
    finally:
        h.close()
    check_against(r, dict(mu=mu, var=var, logp=logp, L=L, grad_theta=gth, grad_b=gb), y)
    want = gth + np.array([loo_ref.log_lognormal_d(theta[0], loo_ref.PRIOR_MU["a"], loo_ref.PRIOR_S2)] +
                          [loo_ref.log_lognormal_d(v, loo_ref.PRIOR_MU["r"], loo_ref.PRIOR_S2) for v in theta[1:]])
    np.testing.assert_allclose(np.concatenate([g[:1], g[2:]]), want, rtol=1e-6, atol=1e-6 * max(np.abs(want).max(), abs(gb)))


@pytest.mark.parametrize("kernel", (0, 1))
def test_gp_loo_grows_across_the_padding(ctx, kernel):
    """A handle fitted on 126 points and grown to 130: after every appended point (at 128 -> 129 the handle is rebuilt on the device)
    sls_gp_loo equals a fresh fit's and sls_nll_loo's, in both sigma modes, at the tolerances of
    test_gp_loo_both_sigma_modes_and_append."""
    b = 0.005
    X, y, theta = loo_ref.problem(5, 130)
    want = {}
    for n in range(126, 131):
        want[n] = loo_once(ctx, X[:, :n], kernel, y[:n], theta, b, want_grad=False)

    def close_to(g, w, n):
        for a, k in zip(g, ("mu", "var", "logp")):
            np.testing.assert_allclose(a, w[k], rtol=1e-7, atol=1e-9 * max(np.abs(w[k]).max(), np.abs(y[:n]).max() if k == "mu" else 0.0))

    for mode in (sls().SIGMA_EXPLICIT_INVERSE, sls().SIGMA_CHOLESKY_SOLVE):
        gp = sls().GP(ctx, X[:, :126], y[:126], theta, b, kernel)
        try:
            gp.set_sigma_mode(mode)
            close_to(gp.loo(), want[126], 126)
            for n in range(127, 131):
                gp.append_point(X[:, n - 1], y[n - 1])
                close_to(gp.loo(), want[n], n)
                fresh = sls().GP(ctx, X[:, :n], y[:n], theta, b, kernel)
                try:
                    fresh.set_sigma_mode(mode)
                    close_to(fresh.loo(), want[n], n)
                finally:
                    fresh.close()
        finally:
            gp.close()


@pytest.mark.parametrize("kernel", (0, 1))
def test_gp_loo_null_pointers_and_sigma_mode_switches(ctx, kernel):
    """Any of sls_gp_loo's three pointers may be NULL; switching the sigma mode back and forth reproduces each mode's bits."""
    X, y, theta = loo_ref.problem(5, 130)
    N = X.shape[1]
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    gp = sls().GP(ctx, X, y, theta, 0.005, kernel)
    try:
        bits = {}
        for mode in (sls().SIGMA_EXPLICIT_INVERSE, sls().SIGMA_CHOLESKY_SOLVE, sls().SIGMA_EXPLICIT_INVERSE, sls().SIGMA_CHOLESKY_SOLVE):
            gp.set_sigma_mode(mode)
            full = gp.loo()
            if mode in bits:
                assert all(np.array_equal(a, w) for a, w in zip(full, bits[mode]))
            bits[mode] = full
            for mask in range(7):                                        # every subset of the pointers but the full one
                out = [np.full(N, np.nan) for _ in range(3)]
                args = [ptr(out[k]) if mask >> k & 1 else None for k in range(3)]
                assert sls().lib().sls_gp_loo(gp.h, *args) == 0
                for k in range(3):
                    assert np.array_equal(out[k], full[k]) if mask >> k & 1 else np.all(np.isnan(out[k]))
    finally:
        gp.close()
