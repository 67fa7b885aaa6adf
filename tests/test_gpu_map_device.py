"""The device-resident MAP fits (map_opt_kernel; sls_pref_map_fit / sls_gp_map_fit) and the device-side Bradley-Terry-Luce terms.

Reference: PreferenceRegressor::PerformMapEstimation + objective (src/preference-regressor.cpp:129-259,332-403), BTL
(include/sequential-line-search/utils.hpp:25-52, no max-subtraction), GaussianProcessRegressor::PerformMapEstimation's local
phase (src/gaussian-process-regressor.cpp:141-193,295).

Checked here:
  * objective + gradient with the BTL terms on the device vs the oracle (slso_pref_objective) at 1e-9: tuple sizes 2-5, goodness
    values up to the exp() overflow edge |f| / s -> 709, both kernels, with and without hyper-parameters, and vs the host-BTL path;
  * one launch == one launch per evaluation (continued from device-resident state), BIT for bit;
  * the device optimiser vs the same optimiser driven from the host with one objective call per evaluation (same optimum);
  * scipy's optima (tests/golden/map_optima.npz) through the C ABI directly.
"""
import os

import numpy as np
import pytest

from util import env_switch, sls, synth_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = sls().Context(0)
    yield c
    c.close()


def random_prefs(rng, M, n_prefs, sizes=(2, 3, 4, 5)):
    prefs = []
    for _ in range(n_prefs):
        m = int(rng.choice(sizes))
        prefs.append([int(i) for i in rng.choice(M, size=min(m, M), replace=False)])
    return prefs


def host_path(fn):
    """Run fn with SLS_MAP_DEVICE=0: BTL terms on the host, optimiser on the host (the pre-round-4 path)."""
    with env_switch("SLS_MAP_DEVICE", 0):
        return fn()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("use_map", [False, True])
@pytest.mark.parametrize("M,D,n_prefs", [(5, 1, 3), (40, 8, 30), (91, 16, 60), (128, 3, 300), (128, 32, 100), (91, 32, 30), (17, 33, 9),
                                         (70, 64, 40), (64, 65, 40), (100, 100, 60), (128, 128, 100)])
def test_device_btl_objective_and_gradient_vs_oracle(ctx, oracle, kernel, use_map, M, D, n_prefs):
    """Round 5: the hyper-parameter gradient runs on the device for every D <= 128 (C3 as the reference runs it: M = 91, D = 32,
    use_MAP_hyperparams = true); (64, 65), (100, 100) and (128, 128) have more than 192 variables (five per lane), D > 64 takes two
    dimensions per lane in the length-scale contraction."""
    rng = np.random.default_rng(100 * M + D + 7 * kernel)
    X = rng.uniform(0, 1, (D, M))
    prefs = random_prefs(rng, M, n_prefs)
    h = sls().Nll(ctx, X, kernel)
    for trial, (yscale, btl_scale) in enumerate([(1.0, 0.01), (0.05, 0.01), (3.0, 1.0), (7.0, 0.01)]):
        y = rng.normal(size=M) * yscale
        if trial == 3:
            # |f| / s up to 709, right below the exp() overflow edge of CalcBtl (709.78), differences within a tuple below it too
            # (CalcBtlDerivative forms exp((f_i - f_0) / s)): the sum of a tuple's exponentials stays finite (8.2e307 + a few 1e299)
            y = np.clip(np.abs(y), 0.0, 6.9)
            y[prefs[0][0]] = 7.09
        hyp = np.concatenate([[rng.uniform(0.2, 1.0), rng.uniform(1e-3, 1e-2)], rng.uniform(0.2, 1.0, D)])
        x = np.concatenate([y, hyp]) if use_map else y
        vo, go = oracle.pref_objective(kernel, X, prefs, x, use_map=use_map, btl_scale=btl_scale)
        v, g = h.pref_objective(prefs, x, use_map=use_map, btl_scale=btl_scale)
        assert np.isfinite(vo) and np.isfinite(go).all()
        scale = max(1.0, abs(vo))
        assert abs(v - vo) <= 1e-9 * scale, (trial, v, vo)
        np.testing.assert_allclose(g, go, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(go).max()))
        vh, gh = host_path(lambda: h.pref_objective(prefs, x, use_map=use_map, btl_scale=btl_scale))
        assert abs(v - vh) <= 1e-11 * scale
        np.testing.assert_allclose(g, gh, rtol=1e-10, atol=1e-10 * max(1.0, np.abs(gh).max()))
        v_only = h.pref_objective(prefs, x, use_map=use_map, btl_scale=btl_scale, want_grad=False)
        assert v_only == v
    h.close()


@pytest.mark.parametrize("kernel", [0, 1])
# (63 .. 65, 128: the element slots of the kernel-function / gradient-weight passes fill the eight register slots exactly, spill one
# element into the pair scratch, and (N = 128) fill the whole LDS image so that the pair scratch is global memory; odd N: the middle
# column of the folded triangle pairs with itself; 1, 2: degenerate triangles)
@pytest.mark.parametrize("M,D", [(30, 4), (60, 32), (91, 32), (64, 100), (112, 5), (100, 16), (16, 128), (33, 1), (63, 7), (64, 32), (65, 32),
                                 (128, 4), (127, 16), (2, 3), (1, 2)])
def test_matrix_core_form_and_direct_difference_form_agree(ctx, oracle, kernel, M, D):
    """Round 5: when the centred design matrix fits beside the N x N image in LDS, the one-workgroup kernels build the Gram matrix
    and the length-scale gradient on the matrix cores (norm expansion, Y = G X); otherwise -- and with SLS_SMALL_XLDS=0 -- they form
    the coordinate differences directly from global memory.  Both against the oracle (1e-9) and against each other (1e-10): the
    preference objective with hyper-parameters, the GP marginal likelihood, and the fitted predictor of a GP handle."""
    rng = np.random.default_rng(7 * M + D + kernel)
    X = rng.uniform(0, 1, (D, M))
    prefs = random_prefs(rng, M, max(3, M // 2))
    y = rng.normal(size=M) * 0.3
    hyp = np.concatenate([[rng.uniform(0.2, 1.0), rng.uniform(1e-3, 1e-2)], rng.uniform(0.3, 1.5, D)])
    x = np.concatenate([y, hyp])
    Q = rng.uniform(0, 1, (D, 17))
    theta = np.concatenate([[hyp[0]], hyp[2:]])

    def run():
        h = sls().Nll(ctx, X, kernel)
        v, g = h.pref_objective(prefs, x, use_map=True)
        vg, gg = h.gp_objective(y, hyp)
        h.close()
        gp = sls().GP(ctx, X, y, theta, hyp[1], kernel)
        mu, sg = gp.predict(Q)
        gp.close()
        return v, g, vg, gg, mu, sg
    fast = run()
    with env_switch("SLS_SMALL_XLDS", 0):
        direct = run()
    vo, go = oracle.pref_objective(kernel, X, prefs, x, use_map=True)
    vgo, ggo = oracle.gp_map_objective(kernel, X, y, hyp)
    ref = oracle.Regressor(X, y, theta, hyp[1], kernel=kernel)
    mu_o, sg_o = ref.predict_batch(Q)
    for (v, g, vg, gg, mu, sg), tol in ((fast, 1e-9), (direct, 1e-9)):
        assert abs(v - vo) <= tol * max(1.0, abs(vo)) and abs(vg - vgo) <= tol * max(1.0, abs(vgo))
        np.testing.assert_allclose(g, go, rtol=tol, atol=tol * max(1.0, np.abs(go).max()))
        np.testing.assert_allclose(gg, ggo, rtol=tol, atol=tol * max(1.0, np.abs(ggo).max()))
        np.testing.assert_allclose(mu, mu_o, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(sg, sg_o, rtol=1e-7, atol=1e-10)
    assert abs(fast[0] - direct[0]) <= 1e-10 * max(1.0, abs(vo)) and abs(fast[2] - direct[2]) <= 1e-10 * max(1.0, abs(vgo))
    np.testing.assert_allclose(fast[1], direct[1], rtol=1e-10, atol=1e-10 * max(1.0, np.abs(go).max()))
    np.testing.assert_allclose(fast[3], direct[3], rtol=1e-10, atol=1e-10 * max(1.0, np.abs(ggo).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("ell", [3e-3, 1e-5, 1e-8])
@pytest.mark.parametrize("M,D", [(40, 6), (200, 6), (300, 64)])
def test_small_length_scales_with_near_duplicates_take_the_direct_form(ctx, oracle, kernel, ell, M, D):
    """ADVICE (round 5): the matrix-core Gram pass expands q_ij = |x~_i|^2 + |x~_j|^2 - 2 x~_i . x~_j, whose cancellation error is
    eps D / (2 l^2) absolute -- O(1) at the l = 1e-8 the DIRECT phase of the GP MAP fit visits, exactly where near-duplicate points
    (late in a line search) have a small TRUE q.  Such evaluations must take the direct differences: the marginal likelihood and its
    gradient with near-duplicates at small l agree with the oracle (which forms differences) and with SLS_SMALL_XLDS=0.
    M = 200 and 300 take the tiled route (N > 128), which carries the same guard; SLS_SMALL_XLDS belongs to the one-workgroup
    kernels, so the bit comparison with it applies at M = 40 only."""
    rng = np.random.default_rng(11 + kernel)
    X = rng.uniform(0, 1, (D, M))
    X[:, 1] = X[:, 0] + ell * 0.3 * rng.normal(size=D)        # q ~ 0.5 at this length scale: the kernel value is O(1), not 0 or 1
    X[:, 7] = X[:, 6] + ell * 1.0 * rng.normal(size=D)
    y = rng.normal(size=M) * 0.3
    hyp = np.concatenate([[0.7, 5e-3], np.full(D, ell)])

    def run():
        h = sls().Nll(ctx, X, kernel)
        vg, gg = h.gp_objective(y, hyp)
        h.close()
        return vg, gg
    fast = run()
    with env_switch("SLS_SMALL_XLDS", 0):
        direct = run()
    vgo, ggo = oracle.gp_map_objective(kernel, X, y, hyp)
    for vg, gg in (fast, direct):
        assert abs(vg - vgo) <= 1e-8 * max(1.0, abs(vgo)), (vg, vgo)
        np.testing.assert_allclose(gg, ggo, rtol=1e-6, atol=1e-8 * max(1.0, np.abs(ggo).max()))
    if M <= 128:
        assert fast[0] == direct[0]                            # the same arithmetic: the guard sent both down the direct path
        np.testing.assert_array_equal(fast[1], direct[1])


def test_device_btl_overflows_like_the_reference(ctx, oracle):
    """utils.hpp:25-29 has no max-subtraction: f / s > 709.78 makes exp() infinite and the likelihood inf / inf = NaN.  The device
    terms must do the same (not silently stabilise), like the oracle's restatement."""
    rng = np.random.default_rng(5)
    M, D = 12, 2
    X = rng.uniform(0, 1, (D, M))
    prefs = [[0, 1, 2], [3, 4], [5, 6, 7, 8]]
    y = rng.normal(size=M)
    y[0] = 7.2                                   # 720 > 709.78
    h = sls().Nll(ctx, X, 1)
    v, g = h.pref_objective(prefs, y, btl_scale=0.01)
    vo, go = oracle.pref_objective(1, X, prefs, y, btl_scale=0.01)
    assert np.isnan(vo) and np.isnan(v)
    assert np.isnan(g[[0, 1, 2]]).all() and np.isfinite(g[3:]).all()
    assert np.array_equal(np.isnan(g), np.isnan(go))
    h.close()


def pref_setup(rng, M, D, use_map):
    X = rng.uniform(0, 1, (D, M))
    prefs = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(M // 3)] + random_prefs(rng, M, 5)
    n = M + (D + 2 if use_map else 0)
    z0 = np.zeros(n)
    lo, hi = np.full(n, -10.0), np.full(n, 10.0)
    if use_map:
        lo[M:], hi[M:] = np.log(1e-8), np.log(10.0)
        z0[M], z0[M + 1], z0[M + 2:] = np.log(0.5), np.log(0.005), np.log(0.5)
    return X, prefs, z0, lo, hi


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("use_map,M,D", [(False, 30, 4), (False, 91, 32), (True, 30, 4), (True, 61, 16), (True, 91, 32), (True, 48, 32),
                                         (True, 90, 101)])
def test_pref_fit_one_launch_equals_one_launch_per_evaluation(ctx, kernel, use_map, M, D):
    rng = np.random.default_rng(31 * M + D)
    X, prefs, z0, lo, hi = pref_setup(rng, M, D, use_map)
    h = sls().Nll(ctx, X, kernel)
    one = h.pref_map_fit(prefs, z0, lo, hi, 100, 0, use_map=use_map)
    per = h.pref_map_fit(prefs, z0, lo, hi, 100, 1, use_map=use_map)
    few = h.pref_map_fit(prefs, z0, lo, hi, 100, 7, use_map=use_map)
    assert one["evals"] == per["evals"] == few["evals"] and 1 < one["evals"] <= 100
    assert one["value"] == per["value"] == few["value"]
    assert np.array_equal(one["z"], per["z"]) and np.array_equal(one["z"], few["z"])
    # the reported value is the objective at the returned point
    x = one["z"].copy()
    if use_map:
        x[M:] = np.exp(x[M:])
    v = h.pref_objective(prefs, x, use_map=use_map, want_grad=False)
    assert abs(v - one["value"]) <= 1e-12 * max(1.0, abs(v))
    assert one["value"] > h.pref_objective(prefs, np.concatenate([z0[:M], np.exp(z0[M:])]), use_map=use_map, want_grad=False)
    h.close()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D", [(20, 1), (90, 8), (128, 16), (60, 32), (100, 128)])
def test_gp_fit_one_launch_equals_one_launch_per_evaluation(ctx, oracle, kernel, N, D):
    X, y, _, _ = synth_problem(oracle, D, N, seed=77 + N)
    z0 = np.log(np.concatenate([[0.5, 1e-4], np.full(D, 0.5)]))
    lo, hi = np.full(D + 2, np.log(1e-8)), np.full(D + 2, np.log(50.0))
    h = sls().Nll(ctx, X, kernel)
    one = h.gp_map_fit(y, z0, lo, hi, 1000, 0)
    per = h.gp_map_fit(y, z0, lo, hi, 1000, 1)
    assert one["evals"] == per["evals"] and one["value"] == per["value"] and np.array_equal(one["z"], per["z"])
    v, g = h.gp_objective(y, np.exp(one["z"]))
    vo, go = oracle.gp_map_objective(kernel, X, y, np.exp(one["z"]))
    assert abs(v - one["value"]) <= 1e-12 * max(1.0, abs(v)) and abs(vo - one["value"]) <= 1e-9 * max(1.0, abs(vo))
    assert one["value"] >= h.gp_objective(y, np.exp(z0), want_grad=False)
    # bounded stationary point in the log-parameters (or the evaluation cap was reached)
    gz = go * np.exp(one["z"])
    gz[(one["z"] <= lo + 1e-12) & (gz < 0)] = 0.0
    gz[(one["z"] >= hi - 1e-12) & (gz > 0)] = 0.0
    assert one["evals"] == 1000 or np.max(np.abs(gz)) <= 1e-4 * max(1.0, abs(vo)), (one["evals"], np.max(np.abs(gz)))
    h.close()


def host_driven_maximise(f, z0, lo, hi, max_evals, ftol_rel=0.0, xtol_rel=0.0):
    """optim::MaximizeBounded (host/device.cpp) restated in numpy: the optimiser the device kernel implements, driven with one
    objective call per evaluation."""
    x = np.clip(z0, lo, hi)
    v, g = f(x)
    fx, g, evals = -v, -g, 1
    S, Y, rho = [], [], []
    stalled = False
    while evals < max_evals and not stalled:
        pg = g.copy()
        pg[((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))] = 0.0
        if not np.abs(pg).max() > 0:
            break
        d = pg.copy()
        al = [0.0] * len(S)
        for k in range(len(S) - 1, -1, -1):
            al[k] = rho[k] * S[k].dot(d)
            d -= al[k] * Y[k]
        gamma = S[-1].dot(Y[-1]) / Y[-1].dot(Y[-1]) if S else 1.0 / max(1.0, np.sqrt(pg.dot(pg)))
        d *= gamma
        for k in range(len(S)):
            d += S[k] * (al[k] - rho[k] * Y[k].dot(d))
        d = np.where(pg == 0.0, 0.0, -d)
        if not pg.dot(d) < 0:
            S, Y, rho = [], [], []
            d = -pg / max(1.0, np.sqrt(pg.dot(pg)))
            if not pg.dot(d) < 0:
                break
        t, accepted, bt = 1.0, False, 0
        while bt <= 30 and evals < max_evals:
            xt = np.clip(x + t * d, lo, hi)
            if (xt - x).dot(xt - x) == 0.0:
                break
            vt, gt = f(xt)
            ft, gt, evals = -vt, -gt, evals + 1
            if np.isfinite(ft) and ft <= fx + 1e-4 * g.dot(xt - x):
                s, yv = xt - x, gt - g
                if s.dot(yv) > 1e-10 * yv.dot(yv) and s.dot(yv) > 0:
                    S, Y, rho = (S + [s])[-8:], (Y + [yv])[-8:], (rho + [1.0 / s.dot(yv)])[-8:]
                # NLopt's relative stopping tests on the accepted step (sls_nll_set_tolerances)
                if ftol_rel > 0 and (abs(ft - fx) < ftol_rel * 0.5 * (abs(ft) + abs(fx)) or ft == fx):
                    stalled = True
                if xtol_rel > 0 and np.all((np.abs(xt - x) < xtol_rel * 0.5 * (np.abs(xt) + np.abs(x))) | (xt == x)):
                    stalled = True
                x, g, fx, accepted = xt, gt, ft, True
                break
            t *= 0.5
            bt += 1
        if not accepted:
            break
    return x, -fx, evals


@pytest.mark.parametrize("use_map,M,D", [(False, 40, 6), (True, 40, 6)])
def test_device_optimiser_reaches_the_host_driven_optimum(ctx, use_map, M, D):
    rng = np.random.default_rng(9 + M)
    X, prefs, z0, lo, hi = pref_setup(rng, M, D, use_map)
    h = sls().Nll(ctx, X, 1)

    def f(z):
        x = z.copy()
        if use_map:
            x[M:] = np.exp(x[M:])
        v, g = h.pref_objective(prefs, x, use_map=use_map)
        if use_map:
            g = g.copy()
            g[M:] *= x[M:]
        return v, g
    dev = h.pref_map_fit(prefs, z0, lo, hi, 5000, 0, use_map=use_map)
    xh, vh, eh = host_driven_maximise(f, z0, lo, hi, 5000)
    assert dev["evals"] < 5000 and eh < 5000                       # both converged
    assert abs(dev["value"] - vh) <= 1e-8 * max(1.0, abs(vh)), (dev["value"], vh)
    np.testing.assert_allclose(dev["z"], xh, atol=2e-4 * max(1.0, np.abs(xh).max()))
    # the first iterations follow the same trajectory to rounding (the optimiser IS the same statement sequence)
    dev5 = h.pref_map_fit(prefs, z0, lo, hi, 5, 0, use_map=use_map)
    x5, v5, _ = host_driven_maximise(f, z0, lo, hi, 5)
    assert abs(dev5["value"] - v5) <= 1e-9 * max(1.0, abs(v5))
    np.testing.assert_allclose(dev5["z"], x5, rtol=1e-8, atol=1e-9)
    h.close()


@pytest.mark.parametrize("use_map,M,D", [(False, 40, 6), (True, 40, 6), (True, 61, 32)])
def test_relative_stopping_tests_of_nlopt_end_the_map_fits(ctx, oracle, use_map, M, D):
    """sls_nll_set_tolerances (round 5): NLopt's relative tests on every accepted step of the device-resident MAP fits -- what
    nloptutil::solve's defaults (1e-6 / 1e-6) do to the reference's fits and what the host layer sets.  The
    device fit must stop where the host-driven optimiser with the same tests stops (to within the steps that hover around the
    threshold), end within the tolerance's reach of the converged optimum, use far fewer
    evaluations than the run to convergence, and tolerances of 0 must restore that run.  Likewise the GP marginal-likelihood fit."""
    rng = np.random.default_rng(19 + M)
    X, prefs, z0, lo, hi = pref_setup(rng, M, D, use_map)
    h = sls().Nll(ctx, X, 1)

    def f(z):
        x = z.copy()
        if use_map:
            x[M:] = np.exp(x[M:])
        v, g = h.pref_objective(prefs, x, use_map=use_map)
        if use_map:
            g = g.copy()
            g[M:] *= x[M:]
        return v, g
    full = h.pref_map_fit(prefs, z0, lo, hi, 5000, 0, use_map=use_map)
    h.set_tolerances(1e-6, 1e-6)
    dev = h.pref_map_fit(prefs, z0, lo, hi, 5000, 0, use_map=use_map)
    xh, vh, eh = host_driven_maximise(f, z0, lo, hi, 5000, 1e-6, 1e-6)
    # (on the slow tail successive steps hover around the threshold: which of them is the first below it may differ between two
    # implementations that round differently -- by a dozen evaluations and as many times 1e-6 of the value, measured)
    assert abs(dev["evals"] - eh) <= max(5, 0.15 * eh) and dev["evals"] < 0.7 * full["evals"], (dev["evals"], eh, full["evals"])
    scale = max(1.0, abs(full["value"]))
    # (the tests look at ONE step: on the slow tail of the joint fit a step below 1e-6 still leaves 4e-4 of the objective on the table
    # -- measured here; the reference's fits, which run with the same tests, stop there as well)
    assert abs(dev["value"] - vh) <= 5e-5 * scale and full["value"] - dev["value"] <= 2e-3 * scale and dev["value"] <= full["value"] + 1e-9 * scale
    stepwise = h.pref_map_fit(prefs, z0, lo, hi, 5000, 1, use_map=use_map)          # one launch per evaluation: the same machine
    assert stepwise["evals"] == dev["evals"] and stepwise["value"] == dev["value"]
    h.set_tolerances(0.0, 0.0)
    again = h.pref_map_fit(prefs, z0, lo, hi, 5000, 0, use_map=use_map)
    assert again["evals"] == full["evals"] and again["value"] == full["value"]
    # GP marginal likelihood on the same points
    y = np.sin(3.0 * X.sum(axis=0)) + 0.05 * rng.normal(size=M)
    zg = np.log(np.concatenate([[0.5, 0.01], np.full(D, 0.5)]))
    lg, hg = np.full(D + 2, np.log(1e-8)), np.full(D + 2, np.log(10.0))
    gfull = h.gp_map_fit(y, zg, lg, hg, 1000)
    h.set_tolerances(1e-6, 1e-6)
    gtol = h.gp_map_fit(y, zg, lg, hg, 1000)
    assert gtol["evals"] < 0.7 * gfull["evals"] and abs(gtol["value"] - gfull["value"]) <= 1e-5 * max(1.0, abs(gfull["value"])), (gtol, gfull)
    h.close()


@pytest.mark.parametrize("fixture", ["map_optima.npz", "map_optima_c3.npz"])
def test_pref_fit_matches_scipy_optima_through_the_c_abi(ctx, fixture):
    """tests/golden/map_optima.npz (scipy TNC / L-BFGS-B on a numpy objective) against sls_pref_map_fit directly; map_optima_c3.npz
    holds config 3's own shape (D = 32, M = 91 and 40), with and without the joint hyper-parameter estimation."""
    z = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    for name in [str(n) for n in z["pref_cases"]]:
        c = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
        X, kind, use_map = c["X"], int(c["kernel"]), bool(int(c["use_map"]))
        D, M = X.shape
        offs = c["offsets"]
        prefs = [[int(i) for i in c["prefs_flat"][offs[p]:offs[p + 1]]] for p in range(len(offs) - 1)]
        n = M + (D + 2 if use_map else 0)
        z0, lo, hi = np.zeros(n), np.full(n, -10.0), np.full(n, 10.0)
        if use_map:
            lo[M:], hi[M:] = np.log(1e-8), np.log(10.0)
            z0[M], z0[M + 1], z0[M + 2:] = np.log(0.5), np.log(0.005), np.log(0.5)
        h = sls().Nll(ctx, X, kind)
        r = h.pref_map_fit(prefs, z0, lo, hi, 20000, 0, use_map=use_map)
        h.close()
        scale = max(1.0, abs(float(c["value"])))
        assert r["value"] >= float(c["value"]) - 1e-6 * scale, (name, r["value"], float(c["value"]))
        if abs(r["value"] - float(c["value"])) <= 1e-6 * scale:
            np.testing.assert_allclose(r["z"][:M], c["x_opt"][:M], atol=1e-3 * max(1.0, float(np.max(np.abs(c["x_opt"][:M])))))


def test_unsupported_sizes_are_reported_not_computed(ctx):
    rng = np.random.default_rng(1)
    X = rng.uniform(0, 1, (3, 130))
    h = sls().Nll(ctx, X, 1)
    with pytest.raises(sls().Unsupported):
        h.pref_map_fit([[0, 1]], np.zeros(130), np.full(130, -10.0), np.full(130, 10.0), 10)
    h.close()
    X = rng.uniform(0, 1, (130, 30))
    h = sls().Nll(ctx, X, 1)
    with pytest.raises(sls().Unsupported):
        h.gp_map_fit(np.zeros(30), np.zeros(132), np.full(132, -18.0), np.full(132, 3.9), 10)
    h.close()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D", [(300, 5), (1000, 8), (1024, 3), (1537, 16)])
def test_value_only_batch_runs_concurrent_bordered_factorisations(ctx, oracle, kernel, N, D):
    """sls_gp_nll_batch for N > 128: the B independent points of a DIRECT iteration (src/gaussian-process-regressor.cpp:294) are
    factored several at a time in ONE persistent launch, each on its own share of the chip, with y as a border row of K_y so that
    y^T K^-1 y and log|K_y| come from the factor alone.  Values: bit-identical to the same call with one point at a time (how many
    workgroups share a factorisation never changes a tile's arithmetic), equal to the full evaluation (explicit inverse) and to the
    oracle to rounding; N = 1024 has no padding row (an extra 128-block carries the border)."""
    X, y, _, _ = synth_problem(oracle, D, N, seed=500 + N)
    rng = np.random.default_rng(N + kernel)
    B = 7
    xs = np.column_stack([rng.uniform(0.2, 1.5, B), 10.0 ** rng.uniform(-4, -1, B), rng.uniform(0.3, 1.5, (B, D))])
    h = sls().Nll(ctx, X, kernel)
    vals = h.gp_objective_batch(y, xs)
    single = np.array([h.gp_objective_batch(y, xs[k:k + 1])[0] for k in range(B)])
    assert np.array_equal(vals, single)
    with env_switch("SLS_NLL_BATCH", 0):
        full = h.gp_objective_batch(y, xs)                   # one full evaluation (K^-1, alpha) after the other
    orc = np.array([oracle.gp_map_objective(kernel, X, y, xs[k], want_grad=False) for k in range(B)])
    scale = np.maximum(1.0, np.abs(orc))
    assert np.max(np.abs(vals - full) / scale) <= 1e-10, np.max(np.abs(vals - full) / scale)
    assert np.max(np.abs(vals - orc) / scale) <= 1e-9, np.max(np.abs(vals - orc) / scale)
    h.close()
