"""The Laplace posterior through the host classes and the pybind11 module: PreferenceRegressor.use_laplace_posterior against the
ctypes handle (sls_gp_set_laplace) on the same fitted values, the refusal of Schonlau's trick, and the optimisers' switch."""
import os
import sys

import numpy as np
import pytest

import laplace_ref as lr
from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pysls():
    sys.path.insert(0, os.path.join(ROOT, "sequential-line-search_amd"))
    import pySequentialLineSearch
    return pySequentialLineSearch


@pytest.fixture(scope="module")
def case():
    N, D = 40, 3
    rng = np.random.default_rng(1000 + N + D)
    X = np.asfortranarray(rng.uniform(0, 1, (D, N)))
    prefs = lr.example_prefs(N, rng)
    Xs = np.asfortranarray(np.random.default_rng(57).uniform(0.02, 0.98, (D, 50)))
    return X, prefs, Xs


def test_regressor_predicts_the_sigma_of_the_ctypes_handle(pysls, case):
    X, prefs, Xs = case
    m = sls()
    reg = pysls.PreferenceRegressor(X, [list(p) for p in prefs])
    assert not reg.uses_laplace_posterior()
    mu0, sg0 = reg.predict(Xs)
    with pytest.raises(Exception):
        reg.laplace_log_evidence()
    reg.use_laplace_posterior()
    assert reg.uses_laplace_posterior()
    mu, sg = reg.predict(Xs)
    y, theta, b = reg.goodness_values(), reg.kernel_hyperparams(), reg.noise_hyperparam()
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
    gp.set_sigma_mode(m.SIGMA_CHOLESKY_SOLVE)
    gp.set_laplace(prefs, 0.01)
    mu_c, sg_c = gp.predict(Xs)
    np.testing.assert_allclose(sg, sg_c, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(mu, mu_c, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(mu, mu0, rtol=1e-9, atol=1e-12)                 # the mean does not change
    assert np.all(sg >= sg0 - 1e-8) and np.median(sg) > 1.5 * np.median(sg0)
    assert reg.laplace_log_evidence() == pytest.approx(gp.laplace_summary()["log_evidence"], rel=1e-9, abs=1e-9)
    S = reg.goodness_covariance()
    np.testing.assert_allclose(S, gp.laplace_matrix(m.LAPLACE_COV), rtol=1e-9, atol=1e-12)
    # ... and both are the restatement's, at the regressor's own fitted values
    ref = lr.LaplaceRef(X, y, theta, b, lr.MATERN52, prefs, 0.01)
    np.testing.assert_allclose(sg, ref.predict(Xs)[1], rtol=1e-6, atol=1e-8)
    assert reg.laplace_log_evidence() == pytest.approx(ref.log_evidence, rel=1e-6, abs=1e-8)
    # Schonlau's trick appends pseudo-observations: refused with a pointer to the draw-based batch criteria; one point is a search
    with pytest.raises(RuntimeError) as e:
        pysls.find_next_points(reg, 2, 16, 5)
    assert "FindNextQueryByExpectedUtility" in str(e.value) and "Laplace" in str(e.value)
    one = pysls.find_next_points(reg, 1, 16, 5)
    assert len(one) == 1 and np.all((one[0] >= 0) & (one[0] <= 1))
    reg.use_laplace_posterior(False)
    assert not reg.uses_laplace_posterior()
    assert np.array_equal(reg.predict(Xs)[1], sg0)
    assert len(pysls.find_next_points(reg, 2, 16, 5)) == 2
    gp.close()
    ctx.close()


def test_an_empty_regressor_ignores_the_call(pysls):
    reg = pysls.PreferenceRegressor(np.zeros((3, 0), order="F"), [])
    reg.use_laplace_posterior()
    assert not reg.uses_laplace_posterior()


def utility(x):
    return -np.linalg.norm(x - 0.3)


def run_optimizer(pysls, laplace):
    """Three plain steps and three expected-utility steps of a 2-D line search with a simulated user; the trajectory of slider ends."""
    pysls.set_random_seed(12)
    # without slider enlargement (it stretches a short slider past the unit box, src/slider.cpp:104-118) every step stays in the box
    opt = pysls.SequentialLineSearchOptimizer(num_dims=2, use_slider_enlargement=False, use_map_hyperparams=False)
    if laplace is not None:
        opt.set_use_laplace_posterior(laplace)
    assert opt.get_use_laplace_posterior() == bool(laplace)
    traj = []
    for it in range(6):
        pos = float(max(np.linspace(0, 1, 11), key=lambda t: utility(opt.calc_point_from_slider_position(t))))
        if it < 3:
            opt.submit_feedback_data(pos)
        else:
            opt.submit_feedback_data_by_expected_utility(pos, num_draws=32, num_global_search_iters=16, num_local_search_iters=10, seed=it,
                                                         num_frequencies=128)
        e0, e1 = opt.get_slider_ends()
        assert np.all((e0 >= 0) & (e0 <= 1)) and np.all((e1 >= 0) & (e1 <= 1))
        x = opt.get_maximizer()
        assert x.shape == (2,) and np.all(x >= 0) and np.all(x <= 1)
        traj.append(np.concatenate([e0, e1, x, [opt.get_preference_value_stdev(np.full(2, 0.5))]]))
    return np.array(traj)


def test_optimizer_switch(pysls):
    off_default = run_optimizer(pysls, None)
    off = run_optimizer(pysls, False)
    on = run_optimizer(pysls, True)
    assert np.array_equal(off, off_default)               # switch off: today's trajectory, bit for bit
    assert np.all(np.isfinite(on))
    assert not np.array_equal(on, off)
    assert on[0, -1] > off[0, -1]                         # after the first (common) step the Laplace deviation at the centre is the larger


@pytest.mark.parametrize("cls", ["SequentialGallerySearchOptimizer", "PreferentialBayesianOptimizer"])
def test_the_other_optimizers_carry_the_switch(pysls, cls):
    pysls.set_random_seed(13)
    opt = getattr(pysls, cls)(num_dims=2, use_map_hyperparams=False)
    opt.set_use_laplace_posterior(True)
    assert opt.get_use_laplace_posterior()
    for on in (True, False):
        opt.set_use_laplace_posterior(on)
        if cls == "SequentialGallerySearchOptimizer":
            opt.submit_feedback_data(0.3, 0.6)
        else:
            opt.submit_feedback_data(0)
            opt.determine_next_query(16, 5)
        here = opt.get_preference_value_stdev(np.full(2, 0.5))
        opt.set_use_laplace_posterior(not on)             # the current regressor follows the switch at once
        there = opt.get_preference_value_stdev(np.full(2, 0.5))
        lap, plain = (here, there) if on else (there, here)
        assert np.isfinite(lap) and lap > plain > 0.0, (on, lap, plain)
