"""The expected utility of the best gallery cell through the C++ host layer, by way of the pybind11 module:
PosteriorFunctionSamples::CalcExpectedUtilitiesOfBestGalleryCell / MaximizeExpectedUtilityOfBestGalleryCell and
acquisition_func::FindNextGalleryByExpectedUtility[FromStarts] against the ctypes path (PathSamples.patch_*) on the same data, seed
and starts, to the bit, and SequentialGallerySearchOptimizer in a simulated-user loop."""
import os
import sys

import numpy as np
import pytest

from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")
D, N, M, S, QS, QT, ND, NF = 3, 25, 7, 48, 3, 4, 24, 128
OD, STEPS = 4, 5                                    # the optimiser loop


@pytest.fixture(scope="module")
def pysls():
    sys.path.insert(0, PKG)
    import pySequentialLineSearch
    return pySequentialLineSearch


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    theta = np.array([0.5] + [0.3] * D)
    return dict(X=X, y=y, theta=theta, P=rng.uniform(0, 1, (4 * D, M)), starts=rng.uniform(0, 1, (4 * D, S)),
                anchor=X[:, int(np.argmax(y))])


def test_calc_and_find_are_the_ctypes_path_to_the_bit(pysls, data):
    X, y, theta, P, starts, anchor = (data[k] for k in ("X", "y", "theta", "P", "starts", "anchor"))
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    draws = pysls.sample_posterior_functions(reg, ND, 5, NF)
    corners = [P[c * D:(c + 1) * D] for c in range(4)]
    pv, pg, pw = draws.calc_expected_utilities_of_best_gallery_cell(*corners, QS, QT)
    fv, fg, fw = pysls.calc_expected_utilities_of_best_gallery_cell(reg, *corners, QS, QT, ND, 5, NF)
    m = sls()
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    ps = m.PathSamples(gp, ND, NF, seed=5)
    v, g, w = ps.patch_eval(P, QS, QT, want_wins=True)
    assert np.array_equal(pv, v) and np.array_equal(pw, w) and np.array_equal(np.concatenate(pg, axis=0), g)
    assert np.array_equal(fv, v) and np.array_equal(fw, w) and np.array_equal(np.concatenate(fg, axis=0), g)
    assert w.shape == (QS * QT, M) and np.array_equal(w.sum(axis=0), np.full(M, ND)) and np.any(g != 0.0)
    tol = m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6)                                # GetLocalSearchTolerances' defaults
    # anchored and free, from explicit starts
    ac, avalue = pysls.find_next_gallery_by_expected_utility_from_starts(reg, anchor, starts[D:], QS, QT, ND, 20, 5, NF)
    ra = ps.patch_maximize(starts[D:], QS, QT, 20, anchor=anchor, opts=tol)
    assert len(ac) == 4 and np.array_equal(ac[0], anchor) and np.array_equal(np.concatenate(ac[1:]), ra["x"]) and avalue == ra["value"]
    fc, fvalue = draws.maximize_expected_utility_of_best_gallery_cell(QS, QT, starts, 20)
    rf = ps.patch_maximize(starts, QS, QT, 20, opts=tol)
    assert len(fc) == 4 and np.array_equal(np.concatenate(fc), rf["x"]) and fvalue == rf["value"]
    ec, evalue = pysls.find_next_gallery_by_expected_utility_from_starts(reg, np.zeros(0), starts, QS, QT, ND, 20, 5, NF)
    assert np.array_equal(np.concatenate(ec), rf["x"]) and evalue == rf["value"]
    ps.close()
    gp.close()
    ctx.close()


def test_seeded_find_reproduces_its_from_starts_form(pysls, data):
    X, y, theta, anchor = (data[k] for k in ("X", "y", "theta", "anchor"))
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    for a, nvar in ((anchor, 3 * D), (np.zeros(0), 4 * D)):
        c7, v7 = pysls.find_next_gallery_by_expected_utility(reg, a, QS, QT, ND, 32, 20, 7, NF)
        c7b, v7b = pysls.find_next_gallery_by_expected_utility(reg, a, QS, QT, ND, 32, 20, 7, NF)
        c8, v8 = pysls.find_next_gallery_by_expected_utility(reg, a, QS, QT, ND, 32, 20, 8, NF)
        cs, vs = pysls.find_next_gallery_by_expected_utility_from_starts(reg, a, pysls.seeded_uniform_starts(nvar, 32, 7), QS, QT, ND, 20,
                                                                         7, NF)
        x7 = np.concatenate(c7)
        assert np.array_equal(x7, np.concatenate(c7b)) and v7 == v7b                 # the same seed, the same gallery
        assert np.array_equal(x7, np.concatenate(cs)) and v7 == vs                   # and that of its starts
        assert not np.array_equal(x7, np.concatenate(c8))
        assert x7.shape == (4 * D,) and np.all((x7 >= 0) & (x7 <= 1)) and np.isfinite(v7)
        if a.size:
            assert np.array_equal(c7[0], anchor)
    for grid in ((1, 4), (4, 1), (5, 4), (0, 2)):
        with pytest.raises(ValueError):
            pysls.find_next_gallery_by_expected_utility(reg, anchor, *grid)


def target(x):
    return -float(np.sum((np.asarray(x) - 0.3) ** 2))


def fixed_corners(d):
    return [np.array([0.9 - 0.1 * i for i in range(d)]), np.array([0.15 + 0.2 * i for i in range(d)]),
            np.array([0.5 + 0.1 * i for i in range(d)]), np.array([0.8 - 0.2 * i for i in range(d)])]


def gallery_run(pysls):
    """STEPS steps of a user who picks the best cell of the 4 x 4 grid: per step the corners, the maximiser and the number of points."""
    pysls.set_random_seed(11)
    opt = pysls.SequentialGallerySearchOptimizer(OD, use_map_hyperparams=False, initial_query_generator=fixed_corners)
    assert np.array_equal(np.concatenate(opt.get_gallery_corners()), np.concatenate(fixed_corners(OD)))
    log, n_before = [], 0
    for it in range(STEPS):
        pts = opt.get_gallery_points(4, 4)
        assert pts.shape == (OD, 16)
        k = int(np.argmax([target(pts[:, c]) for c in range(16)]))
        s, t = (k % 4) / 3.0, (k // 4) / 3.0
        chosen = opt.calc_point_from_gallery_position(s, t)
        assert np.abs(chosen - pts[:, k]).max() <= 2e-15                          # the cell, up to the roundings of 1 - s and 1 - t
        opt.submit_feedback_data(s, t, 4, 4, 32, 100, 24, 20, 100 + it, 128)
        corners, xm, n = opt.get_gallery_corners(), opt.get_maximizer(), opt.get_raw_data_points().shape[1]
        log.append(np.concatenate(corners + [xm, [n]]))
        assert len(corners) == 4 and all(c.shape == (OD,) and np.all((c >= 0.0) & (c <= 1.0)) for c in corners)
        assert np.array_equal(corners[0], xm)                                     # the gallery hangs on the current best point
        X = opt.get_raw_data_points()
        assert any(np.array_equal(X[:, j], xm) for j in range(n))                 # which is one of the data points
        assert n_before < n <= n_before + 5                                       # the chosen point and the four corners at most
        n_before = n
        assert np.isfinite(opt.get_preference_value_mean(xm)) and opt.get_preference_value_stdev(xm) >= 0.0
        assert opt.get_preference_value_means(pts).shape == (16,) and opt.get_preference_value_stdevs(pts).shape == (16,)
    return np.array(log)


def test_gallery_optimizer_loop(pysls):
    a = gallery_run(pysls)
    b = gallery_run(pysls)
    assert np.array_equal(a, b)                                                   # the same seeds, the same run, bit for bit
    assert not np.array_equal(a[0, :4 * OD], a[-1, :4 * OD])                      # the gallery does move
