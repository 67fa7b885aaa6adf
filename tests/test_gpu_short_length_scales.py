"""Every Gram route at short length scales with near-duplicate points, against the direct-difference reference of gram_ref.py.

The matrix-core Gram kernels take q_ij from the norm expansion |x~_i|^2 + |x~_j|^2 - 2 x~_i . x~_j, x~ = (x - 0.5) / l, whose
cancellation error is eps D / (2 l^2) ABSOLUTE in q: nothing at l = 0.3, O(1) at the l = 1e-8 the DIRECT phase of the GP MAP fit
visits -- exactly where a near-duplicate pair (normal late in a line search) has a small TRUE q, so that its kernel value is neither
0 nor a.  The cases here put twenty such pairs among uniform points, candidates against training points and outside the unit box,
and walk l over {0.3, 3e-2, 3e-3, 1e-5, 1e-8} plus one ARD case, at sizes on both sides of every switch (N = 128: one-workgroup
kernels / tiles; D = 32, 64: the staging limits; D = 65: a second dimension chunk).  tests/test_gram_ref_cpu.py shows that the
reference is good to 1e-13 on these cases and that the expansion, emulated in fp64, fails them at l <= 1e-5.

The same bodies run gram_ref.WIDE_CASES: D = 129, 192 and 257 at l = 0.3 sqrt(D) (dense: every gradient row is live) and two cases
beyond the guard.  Above D = 128 the gradient contraction has a second and a third 128-column tile, no handle takes the one-wavefront
kernels, and N <= 128 runs the tiled fit and the tiled MAP objective (the single-launch forms stop at D = 128).

Tolerances (gram_ref.check): Gram entries 4 (D + 8) eps a, derived from the direct form; everything else the suite's own
(test_append_point_equals_refit, test_matrix_core_form_and_direct_difference_form_agree, the short-l MAP test).  Every case leaves
its measured errors in the session's evidence file (kind "short_length_scales")."""
import numpy as np
import pytest

import gram_ref as gr
from util import env_switch, record, sls

pytestmark = pytest.mark.gpu

CASES = [(N, D, case) for (N, D) in gr.SIZES for case in gr.ELL_CASES] + list(gr.WIDE_CASES)
EI, UCB = 0, 1


@pytest.fixture(scope="module")
def ctx():
    c = sls().Context(0)
    yield c
    c.close()


def hold(route, got, ref, y_max, **where):
    """Record the measured errors of `got`, then hold them to the tolerances."""
    record("short_length_scales", route=route, errors=gr.errors(got, {k: ref[k] for k in got}),
           gram_tolerance=gr.gram_tolerance(where["D"]), **{k: (v if isinstance(v, (int, float, str)) else str(v)) for k, v in where.items()})
    gr.check(got, ref, where["D"], y_max)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case", CASES)
def test_gram_and_cross_gram_entries(ctx, N, D, case, kernel):
    """sls_gram and sls_gram_cross entry by entry; twelve of the candidates lie outside the unit box (norms beyond the box bound)."""
    r = gr.reference(N, D, case, kernel)
    got = dict(K=ctx.gram(r["X"], r["theta"], r["b"], kernel), Ks=ctx.gram_cross(r["X"], r["Xs"], r["theta"], kernel))
    hold("gram", got, gr.quantities(r), 1.0, N=N, D=D, ell=case, kernel=kernel)


@pytest.mark.parametrize("wave", [0, 1])
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case", CASES)
def test_fit_predict_and_acquisition(ctx, N, D, case, kernel, wave):
    """sls_gp_create (alpha, K_y^-1, log|K_y|), sls_gp_predict and sls_acq_eval (EI and UCB, values and gradients) in both sigma
    modes, on the per-point wavefront kernels and on the tiled pipeline.  Ten candidates sit at q ~ 0.5 from a training point.

    Beyond the guard a handle takes the tiled pipeline whatever SLS_WAVE_PATH says, with the gradient's two contractions over raw
    coordinate differences: formed from scaled coordinates (a GEMM over x~_i minus x~* times the sum of the weights) they carry
    eps |x~| / l ~ 0.5 absolute at l = 1e-8, which missed the 1e-6 of small entries of the EI gradient at D = 33, 64, 65."""
    m = sls()
    r = gr.reference(N, D, case, kernel)
    ref, y_max = gr.quantities(r), float(np.abs(r["y"]).max())
    with env_switch("SLS_WAVE_PATH", wave):
        for sigma_mode in (0, 1):
            gp = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], kernel)
            if sigma_mode:
                gp.set_sigma_mode(sigma_mode)
            got = dict(alpha=gp.matrix(m.GP_ALPHA), Kinv=gp.matrix(m.GP_K_Y_INV), logdet=gp.summary()["logdet"])
            got["mean"], got["dev"] = gp.predict(r["Xs"])
            got["ei"], got["ei_grad"] = gp.acq_eval(r["Xs"], EI)
            got["ucb"], got["ucb_grad"] = gp.acq_eval(r["Xs"], UCB, 2.0)
            gp.close()
            hold("gp", got, ref, y_max, N=N, D=D, ell=case, kernel=kernel, wave=wave, sigma_mode=sigma_mode)


@pytest.mark.parametrize("wave", [0, 1])
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case", gr.WIDE_CASES)
def test_predict_grad_above_128_dimensions(ctx, N, D, case, kernel, wave):
    """sls_gp_predict_grad in both sigma modes: the gradients of mean and deviation at the tolerance of UCB's gradient, which is
    their sum with h = 2.  Rows 128 and up come from the second and third column tile of the contraction."""
    m = sls()
    r = gr.reference(N, D, case, kernel)
    ref = gr.quantities(r)
    with env_switch("SLS_WAVE_PATH", wave):
        for sigma_mode in (0, 1):
            gp = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], kernel)
            if sigma_mode:
                gp.set_sigma_mode(sigma_mode)
            got = {}
            got["dmean"], got["ddev"] = gp.predict_grad(r["Xs"])
            gp.close()
            hold("predict_grad", got, ref, 1.0, N=N, D=D, ell=case, kernel=kernel, wave=wave, sigma_mode=sigma_mode)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("D", [6, 64])
@pytest.mark.parametrize("case", gr.ELL_CASES)
def test_append_near_duplicates_equals_refit(ctx, case, D, kernel):
    """sls_gp_append_point of near-duplicates of existing points (N0 = 126 -> 130: across the 128 padding) against a fresh fit on the
    extended data (the tolerances of test_append_point_equals_refit) and against the reference."""
    m = sls()
    N0, N = 126, 130
    r = gr.reference(N, D, case, kernel)
    rng = np.random.default_rng(5)
    X, y = np.array(r["X"], order="F"), r["y"].copy()
    for k, i in enumerate(range(N0, N)):
        X[:, i] = X[:, 50 + 7 * k] + gr._offset(rng, r["ell"], 0.7, D)     # q ~ 0.5 from point 50 + 7 k
    f = gr.fit(X, y, r["ell"], gr.A, gr.B, kernel)
    gp = m.GP(ctx, X[:, :N0], y[:N0], r["theta"], r["b"], kernel)
    for i in range(N0, N):
        gp.append_point(X[:, i], y[i])
    fresh = m.GP(ctx, X, y, r["theta"], r["b"], kernel)
    Ki, Kr = gp.matrix(m.GP_K_Y_INV), fresh.matrix(m.GP_K_Y_INV)
    al, alr = gp.matrix(m.GP_ALPHA), fresh.matrix(m.GP_ALPHA)
    ld, ldr = gp.summary()["logdet"], fresh.summary()["logdet"]
    acq = [gp.acq_eval(r["Xs"]), fresh.acq_eval(r["Xs"])]
    gp.close(); fresh.close()
    y_max = float(np.abs(y).max())
    refq = dict(alpha=f["alpha"], Kinv=f["Kinv"], logdet=f["logdet"])
    hold("append", dict(alpha=al, Kinv=Ki, logdet=ld), refq, y_max, N=N, D=D, ell=case, kernel=kernel)
    hold("append_fresh", dict(alpha=alr, Kinv=Kr, logdet=ldr), refq, y_max, N=N, D=D, ell=case, kernel=kernel)
    assert np.abs(Ki - Kr).max() < 1e-9 * np.abs(Kr).max()
    np.testing.assert_allclose(al, alr, rtol=1e-6, atol=1e-7 * y_max)
    np.testing.assert_allclose(ld, ldr, rtol=1e-10)
    for a_, b_ in zip(*acq):
        np.testing.assert_allclose(a_, b_, rtol=1e-6, atol=1e-9 * max(np.abs(b_).max(), 1e-30))


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case", CASES)
def test_joint_posterior_of_a_near_duplicate_candidate_pair(ctx, N, D, case, kernel):
    """sls_gp_predict_cov: mean, diagonal, and the covariance of the near-duplicate candidate pair (its prior covariance is
    k(q ~ 0.5), neither 0 nor a).  The deviation's tolerance (rtol 1e-7, atol 1e-10) carried over to variances: an entry of the
    covariance is a product of two deviations times a correlation <= 1, so |d cov_ij| <= 2e-7 s_i s_j + 1e-10 (s_i + s_j)."""
    r = gr.reference(N, D, case, kernel)
    ref = gr.quantities(r)
    gp = sls().GP(ctx, r["X"], r["y"], r["theta"], r["b"], kernel)
    mu, cov = gp.predict_cov(r["Xs"])
    gp.close()
    i, j = gr.CAND_PAIR
    s = ref["dev"]
    err = np.abs(cov - ref["cov"])
    record("short_length_scales", route="predict_cov", N=N, D=D, ell=str(case), kernel=kernel,
           errors=dict(gr.errors(dict(mean=mu), ref), diag=float(np.diag(err).max()), pair=float(err[i, j]), pair_cov=float(ref["cov"][i, j])))
    gr.check(dict(mean=mu), ref, D, 1.0)
    bound = 2e-7 * np.outer(s, s) + 1e-10 * (s[:, None] + s[None, :])
    assert (np.diag(err) <= np.diag(bound)).all(), (np.diag(err).max(), np.diag(bound).min())
    assert err[i, j] <= bound[i, j] and err[j, i] <= bound[j, i], (err[i, j], bound[i, j])


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case", CASES)
def test_gp_map_objective_and_gradient(ctx, oracle, N, D, case, kernel):
    """Nll.gp_objective (sls_gp_nll_grad) value and gradient against the reference and against the oracle (both form differences)."""
    r = gr.reference(N, D, case, kernel)
    h = sls().Nll(ctx, r["X"], kernel)
    v, g = h.gp_objective(r["y"], r["hyp"])
    h.close()
    vo, go = oracle.gp_map_objective(kernel, r["X"], r["y"], r["hyp"])
    hold("map", dict(map_value=v, map_grad=g), gr.quantities(r), 1.0, N=N, D=D, ell=case, kernel=kernel)
    gr.check(dict(map_value=v, map_grad=g), dict(map_value=vo, map_grad=go), D, 1.0)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D", gr.SIZES + gr.WIDE_SIZES)
def test_gp_map_objective_batch_mixing_ordinary_and_short_length_scales(ctx, N, D, kernel):
    """sls_gp_nll_batch over rows that alternate l = 0.3 and l = 1e-8 (and one ARD row) on data whose near-duplicates are O(1) apart
    at 1e-8: equal to the single evaluations the way test_gp_map_objective_batch_matches_single_evaluations asserts it, and every
    row within 1e-8 max(1, |v|) of the reference."""
    r = gr.reference(N, D, 1e-8, kernel)
    rows = [np.concatenate([[gr.A, gr.B], gr.ell_vector(c, D)]) for c in (0.3, 1e-8, 0.3, 1e-8, "ard", 1e-8, 0.3, 1e-8, 1e-8, 0.3, 0.3)]
    rows[2][0], rows[3][1], rows[5][0] = 0.4, 2e-3, 1.1
    xs = np.array(rows)
    ref = np.array([float(gr.gp_map_objective(r["X"], r["y"], x, kernel)[0]) for x in xs])
    h = sls().Nll(ctx, r["X"], kernel)
    vb = h.gp_objective_batch(r["y"], xs)
    single = np.array([h.gp_objective(r["y"], x, want_grad=False) for x in xs])
    one = np.array([h.gp_objective_batch(r["y"], xs[k:k + 1])[0] for k in range(len(xs))])
    h.close()
    record("short_length_scales", route="map_batch", N=N, D=D, kernel=kernel,
           errors=dict(batch=[float(e) for e in np.abs(vb - ref)], single=[float(e) for e in np.abs(single - ref)]), values=[float(v) for v in ref])
    if N <= 128 and D <= 128:                            # the single-launch objective: one route for batch and single
        np.testing.assert_array_equal(vb, single)
    else:
        np.testing.assert_array_equal(vb, one)
        assert (np.abs(vb - single) <= 1e-9 * np.maximum(1.0, np.abs(single))).all(), (vb, single)
    for got in (vb, single):
        assert (np.abs(got - ref) <= 1e-8 * np.maximum(1.0, np.abs(ref))).all(), (got, ref)


def random_prefs(rng, M, n_prefs, sizes=(2, 3, 4, 5)):
    return [[int(i) for i in rng.choice(M, size=int(rng.choice(sizes)), replace=False)] for _ in range(n_prefs)]


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case", CASES)
def test_preference_objective_with_hyperparameters(ctx, oracle, N, D, case, kernel):
    """pref_objective(use_map=True) against oracle.pref_objective, and the GP objective on the same handle against
    oracle.gp_map_objective (the oracle forms differences)."""
    r = gr.reference(N, D, case, kernel)
    rng = np.random.default_rng(N + D)
    prefs = random_prefs(rng, N, max(3, N // 2))
    x = np.concatenate([r["y"], r["hyp"]])
    h = sls().Nll(ctx, r["X"], kernel)
    v, g = h.pref_objective(prefs, x, use_map=True)
    vg, gg = h.gp_objective(r["y"], r["hyp"])
    h.close()
    vo, go = oracle.pref_objective(kernel, r["X"], prefs, x, use_map=True)
    vgo, ggo = oracle.gp_map_objective(kernel, r["X"], r["y"], r["hyp"])
    got, ref = dict(map_value=v, map_grad=g), dict(map_value=vo, map_grad=go)
    hold("pref", got, ref, 1.0, N=N, D=D, ell=case, kernel=kernel)
    gr.check(dict(map_value=vg, map_grad=gg), dict(map_value=vgo, map_grad=ggo), D, 1.0)
