"""The inputs of tests/test_gpu_maximize_restated.py are not sensitive to the summation order -- shown without a GPU.

util.assert_starts_agree lets 5 % of the starts end elsewhere when one of their Armijo tests sat at rounding level of its threshold.
That share is a condition on the INPUTS.  Here every case of tests/maximize_cases.py runs tests/lbfgs_ref.py on the CPU restatement
of its objective (the oracle's posterior for the handle routes, tests/logei_ref.py, mes_ref.py, eubo_ref.py, qeubo_ref.py, qnei_ref.py,
path_ref.py), once per summation order: at most 2 % of the starts may end more than 1e-6 of the largest value apart.  The same runs
show that each case reaches the branches it is there for."""
import numpy as np
import pytest
from scipy.special import erfc

import eubo_ref
import lbfgs_ref
import logei_ref
import maximize_cases as mc
import mes_ref
import path_ref
import qeubo_ref
import qnei_ref


def cpu_objective(case, oracle):
    """(evaluate, with_live) of the case's objective on the CPU."""
    route, sh = case.route, case.shape
    if route in ("harness", "logei", "mes"):
        ref = oracle.Regressor(case.X, case.y, case.theta, case.b, kernel=case.kernel)
        if route == "harness":
            return (lambda T: ref.acq_eval_batch(T, sh["acq"], mc.UCB_H)), False
        mu_best = ref.mu_best()

        def post(T):
            mu, sg = ref.predict_batch(T)
            dmu, dsg = ref.predict_grad_batch(T)
            return mu, sg, dmu, dsg
        if route == "logei":
            return (lambda T: logei_ref.logei(*post(T)[:2], mu_best, *post(T)[2:])[:2]), False
        return (lambda T: mes_ref.alpha(*post(T)[:2], case.y_star, *post(T)[2:])[:2]), False
    if route == "pair":
        r1 = oracle.Regressor(case.X, case.y, case.theta, case.b, kernel=case.kernel)
        X2, y2 = case.X, case.y
        for k in range(case.grow.shape[1]):                  # FindNextPoints: the point enters with its own predicted mean
            x_new = case.grow[:, k]
            r2 = oracle.Regressor(X2, y2, case.theta, case.b, kernel=case.kernel)
            X2 = np.concatenate([X2, x_new[:, None]], axis=1)
            y2 = np.concatenate([y2, [r2.predict_batch(x_new[:, None])[0][0]]])
        r2 = oracle.Regressor(X2, y2, case.theta, case.b, kernel=case.kernel)
        mu_best = r1.mu_best()

        def pair(T):
            mu, dmu = r1.predict_batch(T)[0], r1.predict_grad_batch(T)[0]
            sg, dsg = r2.predict_batch(T)[1], r2.predict_grad_batch(T)[1]
            if sh["acq"] == mc.EI:
                u = (mu - mu_best) / sg
                Phi, phi = 0.5 * erfc(-u / np.sqrt(2.0)), np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)
                return (mu - mu_best) * Phi + sg * phi, Phi * dmu + phi * dsg
            if sh["acq"] == mc.UCB:
                return mu + mc.UCB_H * sg, dmu + mc.UCB_H * dsg
            return logei_ref.logei(mu, sg, mu_best, dmu, dsg)[:2]
        return pair, False
    if route == "eubo":
        return (lambda T: eubo_ref.eubo(case.X, case.y, case.theta, case.b, case.kernel, T)[:2]), False
    ref = path_ref.PathRef(case.X, case.y, case.theta, case.b, case.kernel, case.n_draws, case.F, case.path_seed)
    if route == "qeubo":
        return (lambda T: qeubo_ref.qeubo(ref, T, sh["q"])[:2]), False
    if route == "qnei":
        t = qnei_ref.max_over_points(ref, case.X)[0]
        return (lambda T: qnei_ref.qnei(ref, T, sh["q"], t)[:2]), False
    return (lambda T, live: ref.eval(T, live // case.per_draw)), True


ALL = [c for route in mc.ROUTES for c in mc.case_ids(route, mc.PAIR_VARIANTS if route == "pair" else None)]


@pytest.fixture(scope="module")
def runs(oracle):
    """(route, shape, variant) -> (case, lanes run, sequential run); each computed once."""
    out = {}
    for route in mc.ROUTES:
        for i in range(len(mc.ROUTES[route])):
            case = mc.Case(route, i)
            evaluate, with_live = cpu_objective(case, oracle)
            for v in (mc.PAIR_VARIANTS if route == "pair" else mc.VARIANTS):
                out[route, i, v] = (case,) + tuple(mc.restated(evaluate, case, mc.VARIANTS[v], order=o, with_live=with_live)
                                                   for o in ("lanes", "sequential"))
    return out


@pytest.mark.parametrize("c", ALL, ids=mc.case_name)
def test_at_most_two_percent_of_the_starts_depend_on_the_summation_order(runs, c):
    case, a, b = runs[c]
    keep = b["y_stars"] > 0.1 * mc.FLOOR
    assert np.array_equal(a["y_stars"] > 0.1 * mc.FLOOR, keep)
    scale = np.abs(b["y_stars"][keep]).max()
    apart = np.abs(a["y_stars"][keep] - b["y_stars"][keep]) > 1e-6 * scale
    print(f"{mc.case_name(c)}: {apart.sum()} of {case.S} starts ({apart.mean():.2%}) end more than 1e-6 apart between the two orders; "
          f"evaluations {a['evals_issued']}, live at the end {a['live_at_end']}, ring {a['ring_max'].max()}, "
          f"smallest Armijo margin {a['armijo_margin'].min():.2e}")
    assert apart.mean() <= 0.02


@pytest.mark.parametrize("i", range(len(mc.EUBO)), ids=lambda i: "D%d" % mc.EUBO[i]["D"])
def test_inputs_of_the_eubo_switch_point_test(oracle, i):
    """tests/test_gpu_eubo.py::test_maximiser_at_the_switch_points_of_the_step_kernel holds its own inputs (the data of the eubo cases
    here, 128 uniform starts of seed 2, 12 evaluations) to the restatement as well."""
    case = mc.Case("eubo", i)
    starts = np.random.default_rng(2).uniform(0, 1, (case.nvar, 128))
    evaluate, _ = cpu_objective(case, oracle)
    a, b = (lbfgs_ref.run(evaluate, starts, 12, order=o) for o in ("lanes", "sequential"))
    apart = np.abs(a["y_stars"] - b["y_stars"]) > 1e-6 * np.abs(b["y_stars"]).max()
    print(f"eubo switch points D = {case.D}: {apart.sum()} of 128 starts end more than 1e-6 apart between the two orders")
    assert apart.mean() <= 0.02


@pytest.mark.parametrize("route", list(mc.ROUTES))
def test_cases_reach_the_branches_they_are_there_for(runs, route):
    for i in range(len(mc.ROUTES[route])):
        case, a, _ = runs[route, i, "default"]
        st = case.starts
        assert (st < 0.0).any() and (st > 1.0).any(), "the clamp"
        on_face = (a["x_stars"] == 0.0) | (a["x_stars"] == 1.0)
        assert on_face.any() and not on_face.all(), "the projected gradient: coordinates on a face and coordinates inside"
        assert (a["evals"] - 1 - a["accepted"]).max() >= 1, "a rejected trial"
        assert a["accepted"].max() >= 4, "steps"
        if route != "pair":
            h3 = runs[route, i, "history3"][1]
            assert h3["ring_max"].max() == 3 and h3["accepted"].max() > 3, "history 3: the ring wraps"
        if route == "qnei":
            assert (a["evals"][case.dead] == 1).all() and (a["y_stars"][case.dead] == 0.0).all(), "no draw improves: leave at once"
            assert np.array_equal(a["x_stars"][:, case.dead], case.starts[:, case.dead])
    if route != "pair":
        tol = [runs[route, i, "tol1e-6"][1]["evals_issued"] < runs[route, i, "default"][1]["evals_issued"] for i in range(len(mc.ROUTES[route]))]
        print(f"{route}: the relative tolerances end starts early in {sum(tol)} of {len(tol)} shapes")
