"""Log expected improvement on the MI355X (acquisition type 2, sls_logei_terms): the scalar terms against 60-digit values, the
combiner against the numpy restatement (tests/logei_ref.py) on the device's own predictions, agreement with expected improvement
where that is sound, the whole evaluation against the CPU oracle and central differences, the guard, the bit-level contract, the
maximiser on problems where expected improvement is exactly 0 at most starts, the other entry points and the argument errors.

Type 2 always takes the tiled evaluation and forms sigma as the gradient evaluations do.  sls_gp_predict by default takes other
routes for small problems and value-only calls, which agree with it to cond(K_y) eps, not to the bit: where a test compares with
sls_gp_predict to a few eps it pins SLS_WAVE_PATH=0 and SLS_TRI_PREDICT=0 (tests/test_gpu_mes.py does the same)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import logei_ref
from test_logei_cpu import load_fixtures, terms_errors
from util import env_switch, sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SE, MATERN52 = 0, 1
LOG_EI, FLOOR = 2, -1.0e300


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def same_route():
    with env_switch("SLS_WAVE_PATH", "0"), env_switch("SLS_TRI_PREDICT", "0"):
        yield


def problem(D, N, seed, ell=0.5, a=0.5, scale=1.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = scale * (np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N))
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


def beside(x, rng):
    """16 points next to x: eight steps to either side along a random direction (to first order one side is uphill)."""
    D = x.size
    out = []
    for _ in range(1):
        d = rng.standard_normal(D)
        d /= np.linalg.norm(d)
        out += [x + sgn * step * d for step in (1e-4, 2e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2, 2e-2) for sgn in (1.0, -1.0)]
    return np.clip(np.array(out).T, 0.0, 1.0)


def device_posterior(gp, Xs):
    """mu, sigma, dmu, dsigma of sls_gp_predict / sls_gp_predict_grad on the route type 2 takes."""
    with same_route():
        mu, sg = gp.predict(Xs)
        dmu, dsg = gp.predict_grad(Xs)
    return mu, sg, dmu, dsg


def combiner_bounds(info, sg, dmu, dsg):
    """The bounds of the combiner test: value 32 eps (1 + u^2 + |log sigma|); gradient 4e-12 s + 64 eps s, s = (B1 max|dmu| + B2
    max|dsigma|) / sigma (4e-12: twice the 2e-13 of the series' first omitted term at u = -30, in B1 and B2, with a margin of ten)."""
    s = (info["B1"] * np.abs(dmu).max(axis=0) + info["B2"] * np.abs(dsg).max(axis=0)) / sg
    return 32 * EPS * (1.0 + info["u"] ** 2 + np.abs(np.log(sg))), 4e-12 * s + 64 * EPS * s


def assert_matches_restatement(val, grad, mu, sg, mu_best, dmu, dsg, label):
    rv, rg, info = logei_ref.logei(mu, sg, mu_best, dmu, dsg)
    assert not info["bad"].any(), label
    tol_v, tol_g = combiner_bounds(info, sg, dmu, dsg)
    ev, eg = np.abs(val - rv), np.abs(grad - rg).max(axis=0)
    assert np.all(ev <= tol_v), (label, "value", (ev / tol_v).max(), info["u"][(ev / tol_v).argmax()])
    assert np.all(eg <= tol_g), (label, "gradient", (eg / tol_g).max(), info["u"][(eg / tol_g).argmax()])
    return (ev / tol_v).max(), (eg / tol_g).max(), info


# ---- 1. scalar terms ---------------------------------------------------------------------------------------------------------------
def test_scalar_terms_against_60_digit_values(ctx):
    u, want = load_fixtures()
    got = ctx.logei_terms(u)
    ratios, msg = terms_errors(u, got, want)
    print("device: " + msg)
    for r in ratios:
        assert np.all(r <= 1.0), msg
    # each output on its own, n = 0 and n = -1
    lib, dp = sls().lib(), C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    for k in range(3):
        only = np.empty(u.size)
        outs = [None, None, None]
        outs[k] = p(only)
        assert lib.sls_logei_terms(ctx.h, p(u), C.c_long(u.size), *outs) == 0
        assert np.array_equal(only, got[k])
    assert lib.sls_logei_terms(ctx.h, p(u), C.c_long(u.size), None, None, None) == 0
    assert lib.sls_logei_terms(ctx.h, None, C.c_long(0), None, None, None) == 0
    only = np.empty(u.size)
    assert lib.sls_logei_terms(ctx.h, p(u), C.c_long(-1), p(only), None, None) == -1


# ---- 2. combiner on the device's own predictions -----------------------------------------------------------------------------------
CASES = [(SE, 90, 1), (MATERN52, 700, 16), (SE, 300, 96), (SE, 90, 129), (MATERN52, 130, 257)]     # the last two: D > 128


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,N,D", CASES)
def test_combiner_on_the_devices_own_predictions(m, ctx, kernel, N, D, mode):
    """y is scaled by 40 against a signal deviation of sqrt(0.5): far from the best observation u = (mu - mu_best) / sigma lies far
    below -30; a few query points next to the best data point give u > 0."""
    X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D), scale=40.0)
    gp = m.GP(ctx, X, y, theta, 0.05, kernel)
    gp.set_sigma_mode(mode)
    mu_best = gp.summary()["mu_best"]
    rng = np.random.default_rng(7)
    worst_v = worst_g = 0.0
    us = []
    for M in (1, 255, 256, 257):
        Xs = rng.uniform(0, 1, (D, M))
        if M > 1:      # next to the best data point: mu rises above mu_best on one side of it
            Xs[:, :16] = beside(X[:, gp.summary()["best_index"]], rng)
        mu, sg, dmu, dsg = device_posterior(gp, Xs)
        val, grad = gp.acq_eval(Xs, LOG_EI)
        wv, wg, info = assert_matches_restatement(val, grad, mu, sg, mu_best, dmu, dsg, (kernel, N, D, mode, M))
        worst_v, worst_g = max(worst_v, wv), max(worst_g, wg)
        us.append(info["u"])
        with same_route():      # (by default a value-only call forms sigma from the triangular factor: equal to rounding only)
            assert np.array_equal(gp.acq_eval(Xs, LOG_EI, want_grad=False), val)  # val alone: the same bits
    u = np.concatenate(us)
    print(f"kernel {kernel} N {N} D {D} mode {mode}: u in [{u.min():.4g}, {u.max():.4g}]; largest error / bound: value {worst_v:.3f}, "
          f"gradient {worst_g:.3f}")
    assert (u > 0).any() and (u < 0).any() and u.min() < -30.0 and ((u > -30.0) & (u < 0)).any()
    gp.close()


# ---- 3. agreement with expected improvement where that is sound --------------------------------------------------------------------
def test_agrees_with_expected_improvement_where_that_is_sound(m, ctx):
    """Same handle, same route (the tiled evaluation).  For u >= -20 the direct form has lost ~u^2 eps ~ 1e-13 of its value to the
    cancellation of phi + u Phi: exp(LogEI) = EI to 1e-10, exp(LogEI) grad LogEI = grad EI to 1e-9 of the point's largest
    component."""
    D, N, M = 5, 300, 400
    X, y, theta = problem(D, N, seed=31, scale=2.0)
    gp = m.GP(ctx, X, y, theta, 0.05, MATERN52)
    rng = np.random.default_rng(5)
    Xs = rng.uniform(0, 1, (D, M))
    Xs[:, :16] = beside(X[:, gp.summary()["best_index"]], rng)
    with same_route():
        mu, sg = gp.predict(Xs)
        ei, dei = gp.acq_eval(Xs, 0)
        lv, lg = gp.acq_eval(Xs, LOG_EI)
    u = (mu - gp.summary()["mu_best"]) / sg
    ok = u >= -20.0
    print(f"{ok.sum()} of {M} points with u >= -20, u in [{u.min():.3g}, {u.max():.3g}]")
    assert ok.sum() >= 50 and (u[ok] > 0).any() and (u[ok] < -5).any()
    rel = np.abs(np.exp(lv[ok]) - ei[ok]) / ei[ok]
    gerr = np.abs(np.exp(lv[ok])[None, :] * lg[:, ok] - dei[:, ok]).max(axis=0) / np.abs(dei[:, ok]).max(axis=0)
    print(f"largest relative difference: value {rel.max():.3g}, gradient {gerr.max():.3g}")
    assert np.all(rel <= 1e-10) and np.all(gerr <= 1e-9)
    gp.close()


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,N,D", [(SE, 90, 2), (MATERN52, 700, 16)])
def test_end_to_end_against_the_cpu_oracle(m, ctx, oracle, kernel, N, D):
    b, M = 0.05, 200
    X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ref = oracle.Regressor(X, y, theta, b, kernel=kernel)
    rng = np.random.default_rng(11)
    Xs = rng.uniform(0, 1, (D, M))
    mu, sg = ref.predict_batch(Xs)
    dmu, dsg = ref.predict_grad_batch(Xs)
    val, grad = gp.acq_eval(Xs, LOG_EI)
    rv, rg, info = logei_ref.logei(mu, sg, ref.mu_best(), dmu, dsg)
    assert not info["bad"].any()
    # alpha = K_y^-1 y carries cond(K_y) eps |alpha| on both sides; k . alpha adds it to mu and to mu_best; sigma = sqrt(a - k^T K_y^-1
    # k) is accurate to cond(K_y) eps a / (2 sigma) (the terms of the MES end-to-end test)
    ev = np.linalg.eigvalsh(oracle.calc_large_ky(kernel, X, theta, b))
    cond = ev[-1] / ev[0]
    vs = np.abs(gp.matrix(m.GP_ALPHA)).max()
    tol_mu = 2 * (1e-10 * a + 4 * cond * EPS * vs * a * np.sqrt(N))          # mu and mu_best
    tol_sg = tol_mu + 4 * cond * EPS * a / (2 * sg)
    au = np.abs(info["u"])
    # first order: d LogEI = (B1 d mu + B2 d sigma) / sigma, twice that for the second-order terms
    tol_v = 32 * EPS * (1.0 + au ** 2 + np.abs(np.log(sg))) + 2 * (info["B1"] * tol_mu + info["B2"] * tol_sg) / sg
    # gradient: each of its factors (1 / sigma, B1, B2 through u, dmu, dsigma) moves by at most rho relative to its scale
    rho = (tol_mu + tol_sg) / sg * (1.0 + au) ** 2 + (tol_mu + tol_sg) / theta[1:].min() / np.maximum(np.abs(dmu).max(axis=0), np.abs(dsg).max(axis=0))
    scale = (info["B1"] * np.abs(dmu).max(axis=0) + info["B2"] * np.abs(dsg).max(axis=0)) / sg
    tol_g = 1e-9 * np.abs(rg).max(axis=0) + 8 * rho * scale
    e_v, e_g = np.abs(val - rv), np.abs(grad - rg).max(axis=0)
    print(f"N {N}: cond {cond:.3g}, u in [{info['u'].min():.3g}, {info['u'].max():.3g}]; largest error / bound: value "
          f"{(e_v / tol_v).max():.3g}, gradient {(e_g / tol_g).max():.3g}; largest errors {e_v.max():.3g} {e_g.max():.3g}")
    assert np.all(e_v <= tol_v), ((e_v / tol_v).max(), cond)
    assert np.all(e_g <= tol_g), ((e_g / tol_g).max(), cond)
    # the device gradient against central differences of device values
    h, sub = 1e-6, np.arange(8)
    for d in range(min(D, 4)):
        E = np.zeros((D, 8))
        E[d] = h
        fd = (gp.acq_eval(Xs[:, sub] + E, LOG_EI, want_grad=False) - gp.acq_eval(Xs[:, sub] - E, LOG_EI, want_grad=False)) / (2 * h)
        err = np.abs(fd - grad[d, sub]).max()
        print(f"  central differences, d = {d}: {err:.3g} (|grad| max {np.abs(grad[:, sub]).max():.3g})")
        assert err <= 1e-6 * (1.0 + np.abs(grad[:, sub]).max())
    gp.close()


# ---- 5. guard ------------------------------------------------------------------------------------------------------------------------
def test_points_at_the_data_take_the_guard(m, ctx):
    """b = 0, query points on the data points (the grid problem of the MES guard test): sigma^2 is rounding noise of either sign around
    0 there and is clamped to sigma = 0 at about half of them.  Wherever the device's sigma is below 1e-10 the value is exactly the
    floor and the gradient exactly 0; everything is finite; the one point off the grid lies above the floor."""
    D, N = 2, 25
    g = np.linspace(0.05, 0.95, 5)
    X = np.array([[a, c] for a in g for c in g]).T.copy()
    y = np.sin(3 * X[0]) * np.cos(2 * X[1])
    theta = np.array([0.5, 0.15, 0.15])
    gp = m.GP(ctx, X, y, theta, 0.0, MATERN52)
    Xs = np.concatenate([X, np.full((D, 1), 0.5001)], axis=1)
    with same_route():
        _, sg = gp.predict(Xs)
    guard = sg < 1e-10
    print(f"sigma at the data: {guard.sum()} of {N} below 1e-10, largest {sg[:N].max():.3g}")
    assert guard[:N].sum() >= 1 and not guard[N]
    val, grad = gp.acq_eval(Xs, LOG_EI)
    assert np.array_equal(val[guard], np.full(guard.sum(), FLOOR)) and np.array_equal(grad[:, guard], np.zeros((D, guard.sum())))
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad)) and val[N] > FLOOR
    with same_route():
        assert np.array_equal(gp.acq_eval(Xs, LOG_EI, want_grad=False), val)
    gp.close()


# ---- 6. bit contract -----------------------------------------------------------------------------------------------------------------
def test_bit_contract(m, ctx, monkeypatch):
    D, N, M = 5, 300, 300
    X, y, theta = problem(D, N, seed=21, scale=10.0)
    gp = m.GP(ctx, X, y, theta, 0.05, MATERN52)
    rng = np.random.default_rng(3)
    Xs = rng.uniform(0, 1, (D, M))
    val, grad = gp.acq_eval(Xs, LOG_EI)
    v2, g2 = gp.acq_eval(Xs, LOG_EI)
    assert np.array_equal(val, v2) and np.array_equal(grad, g2)                      # repeated call
    perm = rng.permutation(M)
    vp, gpm = gp.acq_eval(Xs[:, perm], LOG_EI)
    assert np.array_equal(vp, val[perm]) and np.array_equal(gpm, grad[:, perm])      # the column does not matter
    sub = np.array([7, 200, 131])
    vs, gs = gp.acq_eval(Xs[:, sub], LOG_EI)
    assert np.array_equal(vs, val[sub]) and np.array_equal(gs, grad[:, sub])         # nor do the other points
    ctx.set_candidate_chunk(128)
    vc, gc = gp.acq_eval(Xs, LOG_EI)
    ctx.set_candidate_chunk(16384)
    assert np.array_equal(vc, val) and np.array_equal(gc, grad)                      # nor the candidate chunk
    starts = rng.uniform(0, 1, (D, 200))
    r1 = gp.acq_maximize(starts, 12, LOG_EI)
    monkeypatch.setenv("SLS_COMPACT", "0")
    r0 = gp.acq_maximize(starts, 12, LOG_EI)
    monkeypatch.delenv("SLS_COMPACT")
    assert np.array_equal(r1["x_stars"], r0["x_stars"]) and np.array_equal(r1["y_stars"], r0["y_stars"])
    assert r1["index"] == r0["index"] and r1["value"] == r0["value"]
    assert np.all(np.isfinite(val)) and np.all(val > FLOOR) and np.all(r1["y_stars"] >= gp.acq_eval(starts, LOG_EI)[0])
    gp.close()


# ---- 7. the maximiser where expected improvement is dead ------------------------------------------------------------------------------
def dead_problem(D, N, ell):
    rng = np.random.default_rng(1)
    X = rng.uniform(0, 1, (D, N))
    y = 60.0 * (1.0 + 0.1 * np.sin(2.0 * X.sum(axis=0) / np.sqrt(D))) + 0.05 * rng.standard_normal(N)
    starts = rng.uniform(0, 1, (D, 256))
    return X, y, np.concatenate([[1.0], np.full(D, ell)]), starts


@pytest.mark.parametrize("D,N,ell,cpu_dead", [(5, 40, 0.2, 174), (2, 20, 0.06, 193)])
def test_maximiser_where_expected_improvement_is_dead(m, ctx, D, N, ell, cpu_dead):
    """Observations around 60 under a zero prior mean: away from the data u = (mu - mu_best) / sigma ~ -60 and expected improvement is
    exactly 0 with a zero gradient (on the CPU at 174 and 193 of the 256 starts): those starts never leave.  LogEI is finite with a
    usable gradient at every start."""
    S, n_local = 256, 100
    X, y, theta, starts = dead_problem(D, N, ell)
    gp = m.GP(ctx, X, y, theta, 0.01, SE)
    # the premise, on the device
    ei, dei = gp.acq_eval(starts, 0)
    dead = (ei == 0.0) & np.all(dei == 0.0, axis=0)
    print(f"D {D}: expected improvement and its gradient exactly 0 at {dead.sum()} of {S} starts (CPU: {cpu_dead})")
    assert dead.sum() >= S // 2
    re = gp.acq_maximize(starts, n_local, 0)
    st_ei = gp.last_stats()
    assert np.array_equal(re["x_stars"][:, dead], starts[:, dead])
    moved_ei = np.any(re["x_stars"] != starts, axis=0)
    # LogEI at the starts
    v0, g0 = gp.acq_eval(starts, LOG_EI)
    assert np.all(np.isfinite(v0)) and np.all(np.isfinite(g0)) and np.all(v0 > FLOOR)
    mu, sg, dmu, dsg = device_posterior(gp, starts)
    wv, wg, info = assert_matches_restatement(v0, g0, mu, sg, gp.summary()["mu_best"], dmu, dsg, ("starts", D))
    print(f"  u at the starts in [{info['u'].min():.4g}, {info['u'].max():.4g}]; largest error / bound: value {wv:.3f}, gradient {wg:.3f}")
    # the maximiser
    ctx.prof_enable(True)
    ctx.prof_reset()
    r = gp.acq_maximize(starts, n_local, LOG_EI, offset=1000)
    st = gp.last_stats()
    launches, wave_launches = ctx.prof_get("logei")[1], ctx.prof_get("acq_wave")[1]
    ctx.prof_enable(False)
    moved = np.any(r["x_stars"] != starts, axis=0)
    print(f"  starts that move: {moved.sum()} (EI: {moved_ei.sum()}); evaluations issued {st['evals_issued']} (EI: {st_ei['evals_issued']}) "
          f"of {st['evals_cap']}; rounds {st['rounds']}; live at the end {st['live_at_end']}")
    assert np.all(r["y_stars"] >= v0)
    assert moved.sum() > moved_ei.sum() and st["evals_issued"] > st_ei["evals_issued"]
    assert 1 <= st["rounds"] <= n_local and launches == st["rounds"] and wave_launches == 0
    assert st["evals_cap"] == S * n_local and st["evals_issued"] <= st["evals_cap"]
    assert np.all(np.isfinite(r["y_stars"])) and np.all((r["x_stars"] >= 0) & (r["x_stars"] <= 1))
    if D == 2:
        g1 = np.linspace(0, 1, 401)
        G = np.stack(np.meshgrid(g1, g1, indexing="ij")).reshape(2, -1)
        gmu, gsg = gp.predict(G)
        grid_best = logei_ref.logei(gmu, gsg, gp.summary()["mu_best"])[0].max()
        print(f"  winner {r['value']:.12g}, dense-grid maximum {grid_best:.12g}")
        assert r["value"] >= grid_best - 1e-6
        x = r["x"]
        v, g = gp.acq_eval(x[:, None], LOG_EI)
        assert v[0] == r["value"]
        pg = np.where(((x <= 0) & (g[:, 0] < 0)) | ((x >= 1) & (g[:, 0] > 0)), 0.0, g[:, 0])    # maximisation: may push outwards
        print(f"  projected gradient {np.abs(pg).max():.3g} (largest gradient at the starts {np.abs(g0).max():.3g})")
        assert np.abs(pg).max() <= 1e-5 * max(1.0, np.abs(g0).max())
        assert r["index"] - 1000 == int(np.argmax(r["y_stars"])) and r["value"] == r["y_stars"].max()
        assert np.array_equal(r["x_stars"][:, r["index"] - 1000], x)
    gp.close()


# ---- 8. the other entry points -------------------------------------------------------------------------------------------------------
def test_device_starts_equal_host_starts(m, ctx):
    D, N, S, n_local = 5, 90, 129, 12
    X, y, theta = problem(D, N, seed=17, scale=10.0)
    gp = m.GP(ctx, X, y, theta, 0.05, MATERN52)
    starts = np.random.default_rng(2).uniform(0, 1, (D, S))
    starts_dev = torch.from_numpy(np.ascontiguousarray(starts.T)).to("cuda")     # D x S column-major
    torch.cuda.synchronize()
    rh = gp.acq_maximize(starts, n_local, LOG_EI, offset=7, want_all=False)
    sh = gp.last_stats()
    rd = gp.acq_maximize_dev(starts_dev.data_ptr(), S, n_local, LOG_EI, offset=7)
    assert rd["index"] == rh["index"] and rd["value"] == rh["value"] and np.array_equal(rd["x"], rh["x"])
    assert gp.last_stats() == sh and np.isfinite(rd["value"]) and 7 <= rd["index"] < 7 + S
    gp.close()


def test_pair_entry_points(m, ctx):
    """objective_for_multiple_points: mu, mu_best from the mean handle, sigma from a handle grown by two points."""
    D, N, M, S = 3, 120, 150, 100
    X, y, theta = problem(D, N, seed=23, scale=10.0)
    g_mu = m.GP(ctx, X, y, theta, 0.05, MATERN52)
    g_sg = m.GP(ctx, X, y, theta, 0.05, MATERN52)
    rng = np.random.default_rng(4)
    for _ in range(2):
        x_new = rng.uniform(0, 1, D)
        g_sg.append_point(x_new, float(g_sg.predict(x_new[:, None])[0][0]))
    Xs = rng.uniform(0, 1, (D, M))
    val, grad = g_mu.acq_eval_pair(g_sg, Xs, LOG_EI)
    with same_route():
        mu = g_mu.predict(Xs)[0]
        dmu = g_mu.predict_grad(Xs)[0]
        sg = g_sg.predict(Xs)[1]
        dsg = g_sg.predict_grad(Xs)[1]
    wv, wg, _ = assert_matches_restatement(val, grad, mu, sg, g_mu.summary()["mu_best"], dmu, dsg, "pair")
    print(f"pair evaluation: largest error / bound: value {wv:.3f}, gradient {wg:.3f}")
    with same_route():
        assert np.array_equal(g_mu.acq_eval_pair(g_sg, Xs, LOG_EI, want_grad=False), val)
    single = g_mu.acq_eval(Xs, LOG_EI)[0]
    assert not np.array_equal(single, val)                                        # the grown handle's sigma is in it
    r = g_mu.acq_maximize_pair(g_sg, rng.uniform(0, 1, (D, S)), 15, LOG_EI)
    at = g_mu.acq_eval_pair(g_sg, r["x"][:, None], LOG_EI)[0][0]
    assert np.isfinite(r["value"]) and abs(at - r["value"]) <= 1e-12 and 0 <= r["index"] < S
    g_mu.close()
    g_sg.close()


def test_sharded_maximisation_reproduces_the_single_handle_call(m):
    D, N, S, n_local = 4, 200, 199, 12
    X, y, theta = problem(D, N, seed=29, scale=10.0)
    starts = np.random.default_rng(6).uniform(0, 1, (D, S))
    c = m.Context(0)
    gp = m.GP(c, X, y, theta, 0.05, MATERN52)
    one = gp.acq_maximize(starts, n_local, LOG_EI)
    issued = gp.last_stats()["evals_issued"]
    multi = m.Multi([0, 0])
    mgp = m.MultiGP(multi, X, y, theta, 0.05, MATERN52)
    r = mgp.acq_maximize(starts, n_local, LOG_EI)
    assert r["index"] == one["index"] and r["value"] == one["value"] and np.array_equal(r["x"], one["x"])
    assert r["evals_issued"] == issued and r["index"] == int(np.argmax(one["y_stars"])) and r["value"] < 0
    mgp.close(); multi.close(); gp.close(); c.close()


# ---- 9. arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_errors(m, ctx):
    D, N, S = 2, 30, 3
    X, y, theta = problem(D, N, seed=9)
    gp = m.GP(ctx, X, y, theta, 0.05, SE)
    gs = m.GP(ctx, X, y, theta, 0.05, SE)
    multi = m.Multi([0, 0])
    mgp = m.MultiGP(multi, X, y, theta, 0.05, SE)
    lib, dp = m.lib(), C.POINTER(C.c_double)
    lib.sls_last_error.restype = C.c_char_p
    Xs = np.asfortranarray(np.full((D, S), 0.5))
    Xs_dev = torch.from_numpy(np.ascontiguousarray(Xs.T)).to("cuda")
    torch.cuda.synchronize()
    val, grad = np.empty(S), np.empty((D, S), order="F")
    p = lambda a: None if a is None else a.ctypes.data_as(dp)
    x, v, idx, issued = np.empty(D), C.c_double(), C.c_long(), C.c_long()
    h1 = C.c_double(1.0)

    def ev(acq, h=gp.h, Xp=Xs, M=S, vp=val, gp_=grad):
        return lib.sls_acq_eval(h, acq, h1, p(Xp), M, p(vp), p(gp_))

    def evp(acq, h=gp.h, hs=gs.h, Xp=Xs, M=S, vp=val, gp_=grad):
        return lib.sls_acq_eval_pair(h, hs, acq, h1, p(Xp), M, p(vp), p(gp_))

    def mx(acq, h=gp.h, sp=Xs, n=S, opts=None):
        return lib.sls_acq_maximize(h, acq, h1, p(sp), n, 5, opts, C.c_long(0), p(x), C.byref(v), C.byref(idx), None, None)

    def mxp(acq, h=gp.h, hs=gs.h, sp=Xs, n=S):
        return lib.sls_acq_maximize_pair(h, hs, acq, h1, p(sp), n, 5, None, p(x), C.byref(v), C.byref(idx))

    def mxd(acq, h=gp.h, ptr=Xs_dev.data_ptr(), n=S):
        return lib.sls_acq_maximize_dev(h, acq, h1, C.c_void_p(ptr), n, 5, None, C.c_long(0), p(x), C.byref(v), C.byref(idx))

    def mxm(acq, h=mgp.h, sp=Xs, n=S):
        return lib.sls_multi_acq_maximize(h, acq, h1, p(sp), n, 5, None, p(x), C.byref(v), C.byref(idx), C.byref(issued))

    calls = (ev, evp, mx, mxp, mxd, mxm)
    for call in calls:
        for acq in (3, -1):
            rc, msg = call(acq), lib.sls_last_error().decode()
            assert rc == -1 and "unknown acquisition type" in msg, (call.__name__, acq, rc, msg)
        assert call(LOG_EI) == 0, (call.__name__, lib.sls_last_error())
    assert np.all(np.isfinite(val)) and np.all(val > FLOOR) and np.isfinite(v.value)
    # NULLs and M = 0: as for types 0 and 1
    variants = [lambda a: ev(a, h=None), lambda a: ev(a, Xp=None), lambda a: ev(a, M=0), lambda a: ev(a, Xp=None, M=0, vp=None, gp_=None),
                lambda a: ev(a, M=-1), lambda a: ev(a, gp_=None), lambda a: ev(a, vp=None),
                lambda a: evp(a, h=None), lambda a: evp(a, hs=None), lambda a: evp(a, Xp=None), lambda a: evp(a, M=0), lambda a: evp(a, vp=None),
                lambda a: mx(a, h=None), lambda a: mx(a, sp=None), lambda a: mx(a, n=0),
                lambda a: mxp(a, hs=None), lambda a: mxp(a, sp=None), lambda a: mxd(a, h=None), lambda a: mxd(a, ptr=None),
                lambda a: mxm(a, h=None), lambda a: mxm(a, sp=None)]
    for k, variant in enumerate(variants):
        rcs = [variant(a) for a in (0, 1, LOG_EI)]
        assert rcs[0] == rcs[1] == rcs[2] and rcs[0] in (0, -1), (k, rcs)
    opts = m.LbfgsOpts()
    opts.struct_size = 999
    assert mx(LOG_EI, opts=C.byref(opts)) == -1 and "struct_size" in lib.sls_last_error().decode()
    mgp.close(); multi.close(); gs.close(); gp.close()
