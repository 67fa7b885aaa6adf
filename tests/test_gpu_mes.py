"""Max-value entropy search on the MI355X (sls_mes_terms / sls_mes_eval / sls_mes_maximize): the scalar terms against 60-digit
values, the combiner against the numpy restatement (tests/mes_ref.py) on the device's own predictions, points at the data (guard),
the whole evaluation against the CPU oracle and against central differences, the bit-level contract, the maximiser and the argument
errors.

The MES entry points always take the tiled evaluation and form sigma as the gradient evaluations do (explicit inverse, or the Cholesky
solve of sigma mode 1).  sls_gp_predict by default takes other routes for small problems (one wavefront per point) and for value-only
calls (the triangular form of sigma), which agree with it to rounding (cond(K_y) eps), not to the bit: where a test compares with
sls_gp_predict to a few eps it pins SLS_WAVE_PATH=0 and SLS_TRI_PREDICT=0, so that both sides run the same route."""
import ctypes as C
import os

import numpy as np
import pytest

import mes_ref
from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SE, MATERN52 = 0, 1


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.fixture
def same_route(monkeypatch):
    monkeypatch.setenv("SLS_WAVE_PATH", "0")
    monkeypatch.setenv("SLS_TRI_PREDICT", "0")


def problem(D, N, seed, ell=0.5, a=0.5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


def max_value_samples(rng, K, y, mu):
    """K samples around max(y); from K = 7 on every fourth lies below the mean of mu, so that gamma < 0 occurs."""
    ys = y.max() + 0.2 * rng.standard_normal(K)
    if K >= 7:
        ys[1::4] = mu.mean() - 0.1 * np.abs(rng.standard_normal(ys[1::4].size))
    return ys


def test_scalar_terms_against_60_digit_values(ctx):
    z = np.load(os.path.join(ROOT, "tests", "golden", "mes_terms.npz"))
    t, g, dg = z["t"], z["g"], z["dg"]
    gv, dv = ctx.mes_terms(t)
    err_g = np.abs(gv - g) / (EPS * np.maximum(1.0, t * t))
    err_d = np.abs(dv - dg) / (np.abs(dg) + 1e-300)
    msg = (f"largest value error {err_g.max():.2f} eps max(1, t^2) at t = {t[err_g.argmax()]:.4g}; "
           f"largest g' error {err_d.max():.3g} at t = {t[err_d.argmax()]:.4g}")
    print(msg)
    assert np.all(np.abs(gv - g) <= 16 * EPS * np.maximum(1.0, t * t)), msg
    assert np.all(np.abs(dv - dg) <= 1e-9 * np.abs(dg) + 1e-300), msg
    # either output on its own, and n = 0
    lib, dp = sls().lib(), C.POINTER(C.c_double)
    only = np.empty(t.size)
    assert lib.sls_mes_terms(ctx.h, t.ctypes.data_as(dp), C.c_long(t.size), only.ctypes.data_as(dp), None) == 0
    assert np.array_equal(only, gv)
    assert lib.sls_mes_terms(ctx.h, t.ctypes.data_as(dp), C.c_long(t.size), None, only.ctypes.data_as(dp)) == 0
    assert np.array_equal(only, dv)
    assert lib.sls_mes_terms(ctx.h, None, C.c_long(0), None, None) == 0
    assert lib.sls_mes_terms(ctx.h, t.ctypes.data_as(dp), C.c_long(-1), only.ctypes.data_as(dp), None) == -1


CASES = [(SE, 90, 2), (MATERN52, 700, 16), (SE, 300, 96), (MATERN52, 300, 300), (SE, 90, 129), (MATERN52, 130, 257)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,N,D", CASES)
def test_combiner_on_the_devices_own_predictions(m, ctx, same_route, kernel, N, D, mode):
    X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, 0.05, kernel)
    gp.set_sigma_mode(mode)
    rng = np.random.default_rng(7)
    worst_v = worst_g = 0.0
    for M in (1, 129, 300):
        Xs = rng.uniform(0, 1, (D, M))
        mu, sg = gp.predict(Xs)
        dmu, dsg = gp.predict_grad(Xs)
        for K in (1, 7, 64, 4096):
            ys = max_value_samples(rng, K, y, mu)
            val, grad = gp.mes_eval(ys, Xs)
            rv, rg, info = mes_ref.alpha(mu, sg, ys, dmu, dsg)
            assert not info["bad"].any()
            if K >= 7:
                assert (info["gamma"] < 0).any()
            tol_v = 32 * EPS * (1.0 + (info["gamma"] ** 2).max(axis=0))
            tol_g = 1e-9 * np.abs(rg).max(axis=0) + 64 * EPS * (np.abs(info["A1"]) * np.abs(dmu).max(axis=0) +
                                                                np.abs(info["A2"]) * np.abs(dsg).max(axis=0)) / sg
            ev, eg = np.abs(val - rv), np.abs(grad - rg).max(axis=0)
            worst_v, worst_g = max(worst_v, (ev / tol_v).max()), max(worst_g, (eg / tol_g).max())
            assert np.all(ev <= tol_v), (M, K, (ev / tol_v).max())
            assert np.all(eg <= tol_g), (M, K, (eg / tol_g).max())
            assert np.array_equal(gp.mes_eval(ys, Xs, want_grad=False), val)      # val alone: dmu / dsigma are not needed
    print(f"kernel {kernel} N {N} D {D} mode {mode}: largest error / bound: value {worst_v:.3f}, gradient {worst_g:.3f}")
    gp.close()


def test_points_at_the_data_take_the_guard(m, ctx, same_route):
    """b = 0, query points on the data points: sigma^2 = a - k^T K^-1 k is rounding noise of either sign around 0 there, so that at
    about half of them it is clamped to sigma = 0 (the others keep a sigma of ~1e-7).  Wherever the device's sigma is below 1e-10 the
    value and the gradient are exactly 0; everywhere they are finite."""
    D, N = 2, 25
    g = np.linspace(0.05, 0.95, 5)
    X = np.array([[a, c] for a in g for c in g]).T.copy()
    y = np.sin(3 * X[0]) * np.cos(2 * X[1])
    theta = np.array([0.5, 0.15, 0.15])
    gp = m.GP(ctx, X, y, theta, 0.0, MATERN52)
    Xs = np.concatenate([X, np.full((D, 1), 0.5001)], axis=1)
    _, sg = gp.predict(Xs)
    guard = sg < 1e-10
    print(f"sigma at the data: {guard.sum()} of {N} below 1e-10, largest {sg[:N].max():.3g}")
    assert guard[:N].sum() >= 1 and not guard[N]
    val, grad = gp.mes_eval(np.array([y.max() + 0.1, y.max() + 0.3, 0.0]), Xs)
    assert np.array_equal(val[guard], np.zeros(guard.sum())) and np.array_equal(grad[:, guard], np.zeros((D, guard.sum())))
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad)) and val[N] > 0
    gp.close()


@pytest.mark.parametrize("kernel,N,D", [(SE, 90, 2), (MATERN52, 700, 16)])
def test_end_to_end_against_the_cpu_oracle(m, ctx, oracle, kernel, N, D):
    b, M, K = 0.05, 200, 64
    X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ref = oracle.Regressor(X, y, theta, b, kernel=kernel)
    rng = np.random.default_rng(11)
    Xs = rng.uniform(0, 1, (D, M))
    mu, sg = ref.predict_batch(Xs)
    dmu, dsg = ref.predict_grad_batch(Xs)
    ys = max_value_samples(rng, K, y, mu)
    val, grad = gp.mes_eval(ys, Xs)
    rv, rg, info = mes_ref.alpha(mu, sg, ys, dmu, dsg)
    # alpha = K_y^-1 y carries cond(K_y) eps |alpha| on both sides; k . alpha adds it to mu (the term of test_gpu_path_sample.py); sigma
    # = sqrt(a - k^T K_y^-1 k) is accurate to cond(K_y) eps a / (2 sigma) (include/sls_hip.h, sls_gp_set_sigma_mode)
    ev = np.linalg.eigvalsh(oracle.calc_large_ky(kernel, X, theta, b))
    cond = ev[-1] / ev[0]
    vs = np.abs(gp.matrix(m.GP_ALPHA)).max()
    tol_mu = 1e-10 * a + 4 * cond * EPS * vs * a * np.sqrt(N)
    tol_sg = tol_mu + 4 * cond * EPS * a / (2 * sg)
    # first order: d alpha = -(A1 d mu + A2 d sigma) / sigma, twice that for the second-order terms
    tol_v = 32 * EPS * (1.0 + (info["gamma"] ** 2).max(axis=0)) + 2 * (np.abs(info["A1"]) * tol_mu + np.abs(info["A2"]) * tol_sg) / sg
    # gradient: each of its factors (1 / sigma, A1, A2 through gamma, dmu, dsigma) moves by at most rho relative to its scale
    gmax = np.abs(info["gamma"]).max(axis=0)
    rho = (tol_mu + tol_sg) / sg * (1.0 + gmax) ** 2 + (tol_mu + tol_sg) / theta[1:].min() / np.maximum(np.abs(dmu).max(axis=0), np.abs(dsg).max(axis=0))
    scale = (np.abs(info["A1"]) * np.abs(dmu).max(axis=0) + np.abs(info["A2"]) * np.abs(dsg).max(axis=0)) / sg
    tol_g = 1e-9 * np.abs(rg).max(axis=0) + 8 * rho * scale
    e_v, e_g = np.abs(val - rv), np.abs(grad - rg).max(axis=0)
    print(f"N {N}: cond {cond:.3g}; largest error / bound: value {(e_v / tol_v).max():.3g}, gradient {(e_g / tol_g).max():.3g}; "
          f"largest errors {e_v.max():.3g} {e_g.max():.3g}")
    assert np.all(e_v <= tol_v), ((e_v / tol_v).max(), cond)
    assert np.all(e_g <= tol_g), ((e_g / tol_g).max(), cond)
    # the device gradient against central differences of device values
    h, sub = 1e-6, np.arange(8)
    for d in range(min(D, 4)):
        E = np.zeros((D, 8))
        E[d] = h
        fd = (gp.mes_eval(ys, Xs[:, sub] + E, want_grad=False) - gp.mes_eval(ys, Xs[:, sub] - E, want_grad=False)) / (2 * h)
        err = np.abs(fd - grad[d, sub]).max()
        print(f"  central differences, d = {d}: {err:.3g} (|grad| max {np.abs(grad[:, sub]).max():.3g})")
        assert err <= 1e-6 * (1.0 + np.abs(grad[:, sub]).max())
    gp.close()


def test_bit_contract(m, ctx, monkeypatch):
    D, N, M, K = 5, 300, 300, 64
    X, y, theta = problem(D, N, seed=21)
    gp = m.GP(ctx, X, y, theta, 0.05, MATERN52)
    rng = np.random.default_rng(3)
    Xs = rng.uniform(0, 1, (D, M))
    ys = max_value_samples(rng, K, y, y)
    val, grad = gp.mes_eval(ys, Xs)
    v2, g2 = gp.mes_eval(ys, Xs)
    assert np.array_equal(val, v2) and np.array_equal(grad, g2)                      # repeated call
    perm = rng.permutation(M)
    vp, gpm = gp.mes_eval(ys, Xs[:, perm])
    assert np.array_equal(vp, val[perm]) and np.array_equal(gpm, grad[:, perm])      # the column does not matter
    sub = np.array([7, 200, 131])
    vs, gs = gp.mes_eval(ys, Xs[:, sub])
    assert np.array_equal(vs, val[sub]) and np.array_equal(gs, grad[:, sub])         # nor do the other points
    ctx.set_candidate_chunk(128)
    vc, gc = gp.mes_eval(ys, Xs)
    ctx.set_candidate_chunk(16384)
    assert np.array_equal(vc, val) and np.array_equal(gc, grad)                      # nor the candidate chunk
    starts = rng.uniform(0, 1, (D, 200))
    r1 = gp.mes_maximize(ys, starts, 12)
    monkeypatch.setenv("SLS_COMPACT", "0")
    r0 = gp.mes_maximize(ys, starts, 12)
    monkeypatch.delenv("SLS_COMPACT")
    assert np.array_equal(r1["x_stars"], r0["x_stars"]) and np.array_equal(r1["y_stars"], r0["y_stars"])
    assert r1["index"] == r0["index"] and r1["value"] == r0["value"]
    gp.close()


@pytest.mark.parametrize("D", [1, 2])
def test_maximiser_small(m, ctx, D):
    N, S, n_local, K = 20, 256, 50, 16
    X, y, theta = problem(D, N, seed=40 + D, ell=0.3)
    gp = m.GP(ctx, X, y, theta, 0.01, SE)
    rng = np.random.default_rng(8)
    ys = np.maximum(y.max() + 0.15 * rng.standard_normal(K), gp.summary()["mu_best"])
    starts = rng.uniform(0, 1, (D, S))
    r = gp.mes_maximize(ys, starts, n_local, offset=1000)
    if D == 1:
        G = np.linspace(0, 1, 20001)[None, :]
    else:
        g1 = np.linspace(0, 1, 401)
        G = np.stack(np.meshgrid(g1, g1, indexing="ij")).reshape(2, -1)
    mu, sg = gp.predict(G)
    grid_best = mes_ref.alpha(mu, sg, ys)[0].max()
    print(f"D {D}: winner {r['value']:.12g}, dense-grid maximum {grid_best:.12g}")
    assert r["value"] >= grid_best - 1e-8
    x = r["x"]
    assert np.all((x >= 0) & (x <= 1))
    v, g = gp.mes_eval(ys, x[:, None])
    assert abs(v[0] - r["value"]) <= 1e-12
    pg = np.where(((x <= 0) & (g[:, 0] < 0)) | ((x >= 1) & (g[:, 0] > 0)), 0.0, g[:, 0])    # maximisation: may push outwards
    print(f"  projected gradient {np.abs(pg).max():.3g}")
    assert np.abs(pg).max() <= 1e-5
    assert r["index"] - 1000 == int(np.argmax(r["y_stars"])) and r["value"] == r["y_stars"].max()
    assert np.array_equal(r["x_stars"][:, r["index"] - 1000], x)
    st = gp.last_stats()
    assert 0 < st["evals_issued"] <= S * n_local and st["evals_cap"] == S * n_local and st["rounds"] <= n_local
    gp.close()


def test_maximiser_takes_the_general_path_where_the_wave_path_would_apply(m, ctx):
    """N = 700, D = 4, 64 starts: expected improvement runs this shape in one launch (one wavefront per start) and reports
    rounds = n_local whatever happens; the MES maximiser has no such kernel and goes through the lock-step rounds."""
    D, N, S, n_local = 4, 700, 64, 10
    X, y, theta = problem(D, N, seed=2)
    gp = m.GP(ctx, X, y, theta, 0.05, MATERN52)
    rng = np.random.default_rng(1)
    ys = y.max() + 0.1 * np.abs(rng.standard_normal(8))
    ctx.prof_enable(True)
    ctx.prof_reset()
    r = gp.mes_maximize(ys, rng.uniform(0, 1, (D, S)), n_local)
    st = gp.last_stats()
    ms, launches = ctx.prof_get("mes")
    ctx.prof_enable(False)
    assert 1 <= st["rounds"] <= n_local and launches == st["rounds"] and ctx.prof_get("acq_wave")[1] == 0
    assert st["evals_issued"] <= S * n_local
    assert np.isfinite(r["value"]) and np.all(np.isfinite(r["x_stars"])) and np.all(np.isfinite(r["y_stars"]))
    assert np.all((r["x"] >= 0) & (r["x"] <= 1)) and r["value"] > 0
    gp.close()


def test_argument_errors(m, ctx):
    D, N = 2, 30
    X, y, theta = problem(D, N, seed=9)
    gp = m.GP(ctx, X, y, theta, 0.05, SE)
    lib, dp = m.lib(), C.POINTER(C.c_double)
    Xs = np.asfortranarray(np.full((D, 3), 0.5))
    val, grad = np.empty(3), np.empty((D, 3), order="F")
    ys = np.array([1.0, 1.2, 1.4])
    p = lambda a: a.ctypes.data_as(dp)
    x, v, idx = np.empty(D), C.c_double(), C.c_long()

    def ev(h, ysp, K, Xp, M, vp):
        return lib.sls_mes_eval(h, ysp, K, Xp, M, vp, p(grad))

    def mx(h, ysp, K, sp, opts=None):
        return lib.sls_mes_maximize(h, ysp, K, sp, 3, 5, opts, C.c_long(0), p(x), C.byref(v), C.byref(idx), None, None)

    def refused(rc, word):
        msg = lib.sls_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    big = np.ones(4097)
    for call in (lambda ysp, K: ev(gp.h, ysp, K, p(Xs), 3, p(val)), lambda ysp, K: mx(gp.h, ysp, K, p(Xs))):
        refused(call(p(ys), 0), "K = 0")
        refused(call(p(big), 4097), "K = 4097")
        for bad in (np.nan, np.inf, -np.inf):
            yb = ys.copy()
            yb[1] = bad
            refused(call(p(yb), 3), "y_star[1]")
        refused(call(None, 3), "y_star is NULL")
    refused(ev(None, p(ys), 3, p(Xs), 3, p(val)), "gp is NULL")
    refused(ev(gp.h, p(ys), 3, None, 3, p(val)), "Xs is NULL")
    refused(ev(gp.h, p(ys), 3, p(Xs), 3, None), "val is NULL")
    refused(ev(gp.h, p(ys), 3, p(Xs), -1, p(val)), "M = -1")
    refused(mx(None, p(ys), 3, p(Xs)), "gp is NULL")
    refused(mx(gp.h, p(ys), 3, None), "starts is NULL")
    opts = m.LbfgsOpts()
    opts.struct_size = 999
    refused(mx(gp.h, p(ys), 3, p(Xs), C.byref(opts)), "struct_size")
    assert ev(gp.h, p(ys), 3, None, 0, None) == 0                  # M = 0: nothing to do
    assert ev(gp.h, p(ys), 3, p(Xs), 3, p(val)) == 0 and np.all(val > 0)
    assert mx(gp.h, p(ys), 3, p(Xs)) == 0
    gp.close()
