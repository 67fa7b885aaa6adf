"""The helpers and inputs of tests/test_gpu_subspace.py, checked without a GPU.

tests/subspace_ref.py restates the expand and fold kernels of the *_sub entry points with the contract's loop orders; here it is held
to einsum, and the gradient in z of the composed objective (the oracle's acquisition at x = c + A z, folded) to central differences.
Then the condition on the INPUTS that tests/test_maximize_restated_seeds_cpu.py sets for the other routes: every case of
tests/subspace_cases.py runs tests/lbfgs_ref.py on that objective once per summation order, and at most 2 % of the starts may end more
than 1e-6 of the largest value apart.  The same runs show that the cases reach the branches they are there for."""
import numpy as np
import pytest

import maximize_cases as mc
import subspace_cases as sc
import subspace_ref as sr


def oracle_objective(case, oracle):
    ref = oracle.Regressor(case.X, case.y, case.theta, case.b, kernel=case.kernel)
    return lambda X: ref.acq_eval_batch(X, case.acq, mc.UCB_H)


@pytest.mark.parametrize("i", range(len(sc.SHAPES)), ids=sc.shape_name)
def test_expand_and_fold_agree_with_einsum(i):
    case = sc.SubCase(i)
    Z, k = case.eval_points(300, 40 + i)
    Z = 1.4 * Z - 0.2                                        # no clamp: points outside [0,1]^d too
    X = sr.expand(case.A, case.c, k, Z)
    want = case.c[k].T + np.einsum("mrj,jm->rm", case.A[k], Z)
    assert X.shape == (case.D, 300)
    assert np.abs(X - want).max() <= 1e-14 * max(1.0, np.abs(want).max())
    GX = np.random.default_rng(50 + i).standard_normal((case.D, 300))
    gz = sr.fold(case.A, case.c, k, GX)
    want = np.einsum("mrj,rm->jm", case.A[k], GX)
    assert gz.shape == (case.d, 300)
    assert np.abs(gz - want).max() <= 1e-14 * max(1.0, np.abs(want).max())
    if case.kind != "segment":                               # the constructors keep the image of [0,1]^d inside the cube
        Xin = sr.expand(case.A, case.c, k, np.clip(Z, 0.0, 1.0))
        assert Xin.min() >= -1e-15 and Xin.max() <= 1.0 + 1e-15


def test_identity_map_expands_to_the_variables_themselves():
    Z = np.random.default_rng(3).uniform(0.0, 1.0, (5, 17))
    X = sr.expand(np.eye(5), np.zeros(5), None, Z)
    assert np.array_equal(X, Z)
    assert np.array_equal(sr.fold(np.eye(5), np.zeros(5), None, Z - 0.5), Z - 0.5)


@pytest.mark.parametrize("i", range(len(sc.SHAPES)), ids=sc.shape_name)
def test_gradient_in_z_agrees_with_central_differences(oracle, i):
    """The error of the folded gradient against central differences in z, measured against the error of the oracle's own gradient in
    x against central differences at the same points: the fold may cost a factor 10 over it (both are printed)."""
    case = sc.SubCase(i)
    f = oracle_objective(case, oracle)
    M, h = 12, 1e-5
    Z, k = case.eval_points(M, 60 + i)
    Z = 0.1 + 0.8 * Z
    X = sr.expand(case.A, case.c, k, Z)
    val, gx = f(X)
    gz = sr.fold(case.A, case.c, k, gx)
    fd_z = np.zeros_like(gz)
    for j in range(case.d):
        E = np.zeros_like(Z)
        E[j] = h
        fd_z[j] = (f(sr.expand(case.A, case.c, k, Z + E))[0] - f(sr.expand(case.A, case.c, k, Z - E))[0]) / (2 * h)
    fd_x = np.zeros_like(gx)
    for r in range(case.D):
        E = np.zeros_like(X)
        E[r] = h
        fd_x[r] = (f(X + E)[0] - f(X - E)[0]) / (2 * h)
    err_x = np.abs(fd_x - gx).max() / max(np.abs(gx).max(), 1e-300)
    err_z = np.abs(fd_z - gz).max() / max(np.abs(gz).max(), 1e-300)
    print(f"{sc.shape_name(i)}: folded gradient vs central differences {err_z:.3e}, the oracle's own x-gradient {err_x:.3e}")
    assert err_z <= 10.0 * err_x


@pytest.fixture(scope="module")
def runs(oracle):
    """(shape, variant) -> (case, lanes run, sequential run); each computed once."""
    out = {}
    for i in range(len(sc.SHAPES)):
        case = sc.SubCase(i)
        evaluate = sr.composed(oracle_objective(case, oracle), case.A, case.c, case.map_of_start)
        for v in mc.VARIANTS:
            out[i, v] = (case,) + tuple(mc.restated(evaluate, case, mc.VARIANTS[v], order=o, with_live=True)
                                        for o in ("lanes", "sequential"))
    return out


@pytest.mark.parametrize("c", sc.case_ids(), ids=sc.case_name)
def test_at_most_two_percent_of_the_starts_depend_on_the_summation_order(runs, c):
    case, a, b = runs[c]
    scale = np.abs(b["y_stars"]).max()
    apart = np.abs(a["y_stars"] - b["y_stars"]) > 1e-6 * scale
    print(f"{sc.case_name(c)}: {apart.sum()} of {case.S} starts ({apart.mean():.2%}) end more than 1e-6 apart between the two orders; "
          f"evaluations {a['evals_issued']}, live at the end {a['live_at_end']}, ring {a['ring_max'].max()}, "
          f"smallest Armijo margin {a['armijo_margin'].min():.2e}")
    assert apart.mean() <= 0.02


WRAPS_AND_REJECTS = (0, 1, 7)      # the shapes that reach a rejected trial and a history-3 ring that wraps
ALL_ON_FACES = (2,)                # every end point of this shape lies on faces of [0,1]^2


def test_cases_reach_the_branches_they_are_there_for(runs):
    for i in range(len(sc.SHAPES)):
        case, a, _ = runs[i, "default"]
        st = case.starts
        assert (st < 0.0).any() and (st > 1.0).any(), "the clamp"
        on_face = (a["x_stars"] == 0.0) | (a["x_stars"] == 1.0)
        assert on_face.any(), "the projected gradient: coordinates on a face"
        if i not in ALL_ON_FACES:
            assert not on_face.all(), "... and coordinates inside"
        assert a["accepted"].max() >= 4, "steps"
        if i in WRAPS_AND_REJECTS:
            assert (a["evals"] - 1 - a["accepted"]).max() >= 1, "a rejected trial"
            h3 = runs[i, "history3"][1]
            assert h3["ring_max"].max() == 3 and h3["accepted"].max() > 3, "history 3: the ring wraps"
        assert runs[i, "tol1e-2"][1]["evals_issued"] < a["evals_issued"], "the relative tolerances end starts early"
        assert len(set(case.map_of_start[:case.n_maps])) == case.n_maps, "every map is searched"
