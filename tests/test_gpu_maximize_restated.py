"""Every *_maximize route of the device, start by start, against an independent run of the same bounded L-BFGS.

All routes share one body (csrc/lbfgs_driver.hpp: maximize_begin, lockstep_rounds with the objective as a callback, maximize_finish;
lbfgs_step_kernel / lbfgs_step_reg_kernel<4|16> in csrc/kernels_acq.hip).  tests/lbfgs_ref.py restates the step in numpy with the
objective as a callable; here the callable is the device's own *_eval entry point on the same handle, so the evaluations are the
ones the maximiser sees (each route documents that a point's bits depend on neither its column nor the rest of the call) and only
the optimiser arithmetic is restated.  A gradient block in the wrong rows, a wrong leading dimension of a trial block, options that
do not reach the kernel or a history ring that never fills change a start's trajectory and show here; "no worse than at the
start" and SLS_COMPACT=0/1 bit identity do not see them.

Compared through util.assert_starts_agree, unchanged: end values to 1e-6 on at least 95 % of the starts, every other start with a
restated Armijo margin below 1e-6.  The cases, their seeds and the CPU check that the inputs themselves stay within that share are in
tests/maximize_cases.py.  Every case leaves a "maximize_restated" record in the evidence file (largest end-value gap, bit-equal
starts, largest |x - x_ref|): nothing is asserted on those.

The harness check runs expected improvement and GP-UCB, which are ALSO held to the oracle's C implementation as before: if a route
disagrees with the restatement while the harness check agrees with both, the route is wrong, not the harness."""
import numpy as np
import pytest

import maximize_cases as mc
from util import assert_starts_agree, sls

pytestmark = pytest.mark.gpu
N_LOCAL = mc.N_LOCAL


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def opts_of(m, variant):
    kw = mc.VARIANTS[variant]
    return m.LbfgsOpts(**kw) if kw else None


def run_all_starts(m, label, case, variant, gp, maximize, evaluate):
    """A route that returns every start's end point: device call, restated run on the device's evaluations, comparison."""
    rg = maximize(opts_of(m, variant))
    st = gp.last_stats()
    rr = mc.restated(evaluate, case, mc.VARIANTS[variant])
    mc.hold_to_restatement(rg, rr, label, stats=st)
    return rg, rr


def ids(route, variants=None):
    return dict(argvalues=mc.case_ids(route, variants), ids=mc.case_name)


@pytest.mark.parametrize("c", **ids("harness"))
def test_harness_expected_improvement_and_ucb_also_against_the_oracle(m, ctx, oracle, monkeypatch, c):
    _, i, variant = c
    case = mc.Case("harness", i)
    acq = case.shape["acq"]
    monkeypatch.setenv("SLS_WAVE_PATH", "0")             # N = 600 takes the tiled evaluation in sls_acq_eval; so must the maximiser
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ctx.prof_enable(True)
    ctx.prof_reset()
    rg, rr = run_all_starts(m, mc.case_name(c), case, variant, gp,
                            lambda o: gp.acq_maximize(case.starts, N_LOCAL, acq, mc.UCB_H, opts=o), lambda T: gp.acq_eval(T, acq, mc.UCB_H))
    wave = ctx.prof_get("acq_wave")[1]
    ctx.prof_enable(False)
    assert wave == 0
    if "history" not in mc.VARIANTS[variant]:            # the oracle's wrapper has no history argument
        ro = oracle.Regressor(case.X, case.y, case.theta, case.b, kernel=case.kernel).acq_maximize(
            case.starts, N_LOCAL, acq, mc.UCB_H, diag=True, **mc.VARIANTS[variant])
        assert_starts_agree(rg, ro, label=mc.case_name(c) + " (oracle)")
        assert_starts_agree(rr, ro, label=mc.case_name(c) + " (restated on device evaluations vs oracle)")
    gp.close()


@pytest.mark.parametrize("c", **ids("logei"))
def test_logei(m, ctx, c):
    _, i, variant = c
    case = mc.Case("logei", i)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    v0 = gp.acq_eval(case.starts, mc.LOG_EI)[0]
    floored = v0 <= 0.1 * mc.FLOOR
    print(f"{mc.case_name(c)}: {floored.sum()} starts at the floor, {floored[case.at_data].sum()} of the {case.at_data.size} on data points")
    if case.b == 0.0:
        assert floored[case.at_data].any() and not floored[case.at_data].all(), "premise: sigma < 1e-10 at some of the data points"
    else:
        assert not floored.any(), "premise: sigma = sqrt(b) = 1e-4 at the data points, nowhere near the guard"
    rg, rr = run_all_starts(m, mc.case_name(c), case, variant, gp,
                            lambda o: gp.acq_maximize(case.starts, N_LOCAL, mc.LOG_EI, opts=o), lambda T: gp.acq_eval(T, mc.LOG_EI))
    assert (rr["evals"][floored] == 1).all(), "a start at the floor has a zero gradient and leaves at once"
    assert (rr["evals"] - 1 - rr["accepted"]).max() >= 1, "a rejected trial"
    gp.close()


@pytest.mark.parametrize("c", **ids("mes"))
def test_mes(m, ctx, c):
    _, i, variant = c
    case = mc.Case("mes", i)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    gp.set_sigma_mode(case.shape["mode"])
    run_all_starts(m, mc.case_name(c), case, variant, gp,
                   lambda o: gp.mes_maximize(case.y_star, case.starts, N_LOCAL, opts=o), lambda T: gp.mes_eval(case.y_star, T))
    gp.close()


@pytest.mark.parametrize("c", **ids("pair", mc.PAIR_VARIANTS))
def test_pair(m, ctx, c):
    """FindNextPoints: mean (and mu+) from a handle of N = 126 points, deviation from the same data grown by three append_point calls
    (N = 129: the two handles sit in different paddings).  The route returns its winner only."""
    _, i, variant = c
    case = mc.Case("pair", i)
    acq = case.shape["acq"]
    g_mu = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    g_sg = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    if case.shape["chol"]:
        g_mu.set_sigma_mode(m.SIGMA_CHOLESKY_SOLVE)
        g_sg.set_sigma_mode(m.SIGMA_CHOLESKY_SOLVE)
    for k in range(case.grow.shape[1]):
        x_new = case.grow[:, k]
        g_sg.append_point(x_new, float(g_sg.predict(x_new[:, None])[0][0]))
    assert g_mu.N == 126 and g_sg.N == 129
    r = g_mu.acq_maximize_pair(g_sg, case.starts, N_LOCAL, acq, mc.UCB_H)
    st = g_mu.last_stats()
    rr = mc.restated(lambda T: g_mu.acq_eval_pair(g_sg, T, acq, mc.UCB_H), case, mc.VARIANTS[variant])
    at = g_mu.acq_eval_pair(g_sg, r["x"][:, None], acq, mc.UCB_H, want_grad=False)[0]
    mc.hold_winner_to_restatement(r["value"], r["index"], rr["y_stars"], at, mc.case_name(c))
    assert np.all((r["x"] >= 0.0) & (r["x"] <= 1.0))
    cap = case.S * N_LOCAL
    assert st["evals_cap"] == cap and case.S <= st["evals_issued"] <= cap and 0 <= st["live_at_end"] <= case.S and 1 <= st["rounds"] <= N_LOCAL
    g_mu.close()
    g_sg.close()


@pytest.mark.parametrize("c", **ids("eubo"))
def test_eubo(m, ctx, c):
    _, i, variant = c
    case = mc.Case("eubo", i)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    run_all_starts(m, mc.case_name(c), case, variant, gp, lambda o: gp.eubo_maximize(case.starts, N_LOCAL, opts=o), gp.eubo_eval)
    gp.close()


@pytest.mark.parametrize("c", **ids("qeubo"))
def test_qeubo(m, ctx, c):
    _, i, variant = c
    case = mc.Case("qeubo", i)
    q = case.shape["q"]
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    run_all_starts(m, mc.case_name(c), case, variant, gp,
                   lambda o: ps.qeubo_maximize(case.starts, q, N_LOCAL, opts=o), lambda T: ps.qeubo_eval(T, q))
    ps.close()
    gp.close()


@pytest.mark.parametrize("c", **ids("qnei"))
def test_qnei(m, ctx, c):
    _, i, variant = c
    case = mc.Case("qnei", i)
    q = case.shape["q"]
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    t, _ = ps.max_over_points(case.X)
    v0, g0 = ps.qnei_eval(case.starts[:, case.dead], q, t)
    assert np.all(v0 == 0.0) and np.all(g0 == 0.0), "premise: no draw improves on its incumbent at sets made of data points"
    rg, rr = run_all_starts(m, mc.case_name(c), case, variant, gp,
                            lambda o: ps.qnei_maximize(case.starts, q, N_LOCAL, t, opts=o), lambda T: ps.qnei_eval(T, q, t))
    assert (rr["evals"][case.dead] == 1).all()
    assert np.array_equal(rg["x_stars"][:, case.dead], case.starts[:, case.dead]) and np.all(rg["y_stars"][case.dead] == 0.0)
    ps.close()
    gp.close()


@pytest.mark.parametrize("c", **ids("path"))
def test_path_draws(m, ctx, c):
    """sls_path_maximize runs all n_draws x S starts in one lock-step search (start j maximises draw j / S) and returns one winner per
    draw: the restated run gets the draw of every live column, the winners are compared per draw."""
    _, i, variant = c
    case = mc.Case("path", i)
    S, nd = case.per_draw, case.n_draws
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, nd, case.F, seed=case.path_seed)
    r = ps.maximize(case.starts, N_LOCAL, opts=opts_of(m, variant))
    rr = mc.restated(lambda T, live: ps.eval(T, live // S), case, mc.VARIANTS[variant], with_live=True)
    assert r["x"].shape == (case.D, nd) and np.all((r["x"] >= 0.0) & (r["x"] <= 1.0))
    at = ps.eval(r["x"], np.arange(nd), want_grad=False)
    for s in range(nd):
        mc.hold_winner_to_restatement(r["value"][s], int(r["index"][s]), rr["y_stars"][s * S:(s + 1) * S], at[s], f"{mc.case_name(c)} draw {s}")
    ps.close()
    gp.close()
