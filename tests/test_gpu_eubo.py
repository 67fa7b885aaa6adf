"""Expected utility of the best option of a query pair on the MI355X (sls_eubo_eval / sls_eubo_maximize): the whole evaluation
against the numpy restatement (tests/eubo_ref.py) on the device's own fit with derived tolerances, the variance of the difference
against sls_gp_predict_cov, central differences of device values, the two-sided invariant and the swap symmetry, the guard, the
bit-level contract, the maximiser over [0,1]^(2D) and the argument errors.

The entry points always take the tiled evaluation.  Where a test compares with sls_gp_predict to the bit it pins SLS_WAVE_PATH=0 and
SLS_TRI_PREDICT=0, so that both sides form mu on the same route (tests/test_gpu_mes.py)."""
import ctypes as C

import numpy as np
import pytest

import eubo_ref
import lbfgs_ref
import maximize_cases
from util import sls

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SE, MATERN52 = 0, 1
B = 0.05


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


def swap(P):
    D = P.shape[0] // 2
    return np.concatenate([P[D:], P[:D]], axis=0)


def tolerances(info, theta, N, alpha_max):
    """Bounds on |device - reference| for the value and the gradient (per pair), from the accuracy of the ingredients.
    mu = k . alpha: alpha = K_y^-1 y carries cond(K_y) eps |alpha| on both sides (the term of tests/test_gpu_mes.py's oracle test).
    s^2 = 2a - 2 k(x, x') - d^T K_y^-1 d: cond(K_y) eps a per kernel vector as for sigma^2 there, and d is the difference of two:
    tol_s2 = 16 cond eps a, tol_s = tol_s2 / (2 s).  Value: dEUBO/dmu = Phi, dEUBO/dmu' = Phi', dEUBO/ds = phi, plus the rounding of
    the three products.  Gradient Phi dmu + phi ds2 / (2 s), first order in every factor: u = (mu - mu') / s moves by
    du = (2 tol_mu + |u| tol_s) / s, Phi by phi du, phi by |u| phi du, 1 / (2s) by tol_s / (2 s^2); grad mu moves by tol_mu over the
    shortest length scale and grad s^2 by 2 tol_s2 over it (one derivative of a quantity known to that accuracy)."""
    a, cond = theta[0], info["cond"]
    mu, s, u, Phi, phi = info["mu"], info["s"], np.abs(info["u"]), info["Phi"], info["phi"]
    tol_mu = 1e-10 * a + 4 * cond * EPS * alpha_max * a * np.sqrt(N)
    tol_s2 = 16 * cond * EPS * a
    tol_s = tol_s2 / (2 * s)
    tol_v = (Phi[0] + Phi[1]) * tol_mu + phi * tol_s + 32 * EPS * (np.abs(mu[0]) + np.abs(mu[1]) + s)
    du = (2 * tol_mu + u * tol_s) / s
    ell = theta[1:].min()
    tol_g = []
    for o in range(2):
        dm, ds2 = np.abs(info["dmu"][o]).max(axis=0), np.abs(info["ds2"][o]).max(axis=0)
        first = phi * du * dm + Phi[o] * tol_mu / ell + (u * phi * du / (2 * s) + phi * tol_s / (2 * s * s)) * ds2 + phi / (2 * s) * 2 * tol_s2 / ell
        scale = Phi[o] * dm + phi / (2 * s) * ds2
        tol_g.append(8 * first + 64 * EPS * scale)
    return tol_v, np.stack(tol_g)


SHAPES = [(1, 1), (90, 2), (129, 8), (300, 33), (300, 96), (90, 129), (130, 257)]     # the last two: 2 and 3 column tiles per option


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N,D", SHAPES)
@pytest.mark.parametrize("kernel", [SE, MATERN52])
def test_against_the_reference_on_the_devices_own_fit(m, ctx, kernel, N, D, mode):
    X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, B, kernel)
    gp.set_sigma_mode(mode)
    alpha_max = np.abs(gp.matrix(m.GP_ALPHA)).max()
    rng = np.random.default_rng(5)
    worst_v = worst_g = worst_sv = worst_sg = 0.0
    for M in (1, 129, 300):
        P = rng.uniform(0, 1, (2 * D, M))
        val, grad = gp.eubo_eval(P)
        rv, rg, info = eubo_ref.eubo(X, y, theta, B, kernel, P)
        assert not info["bad"].any() and info["s"].min() >= 1e-3, info["s"].min()
        tol_v, tol_g = tolerances(info, theta, N, alpha_max)
        ev = np.abs(val - rv)
        eg = np.stack([np.abs(grad[:D] - rg[:D]).max(axis=0), np.abs(grad[D:] - rg[D:]).max(axis=0)])
        bound_g = 1e-9 * np.abs(rg).max(axis=0)[None, :] + tol_g
        worst_v, worst_g = max(worst_v, (ev / tol_v).max()), max(worst_g, (eg / bound_g).max())
        assert np.all(ev <= tol_v), (M, (ev / tol_v).max())
        assert np.all(eg <= bound_g), (M, (eg / bound_g).max())
        assert np.array_equal(gp.eubo_eval(P, want_grad=False), val)          # the value does not depend on asking for the gradient
        # two-sided invariant: 0 <= EUBO - max(mu, mu') <= s / sqrt(2 pi), up to what the value itself is known to
        excess = val - np.maximum(info["mu"][0], info["mu"][1])
        assert np.all(excess >= -tol_v) and np.all(excess <= info["s"] / np.sqrt(2 * np.pi) + tol_v)
        # (x', x): the same value and the mirrored gradient
        vs, gs = gp.eubo_eval(swap(P))
        scale = np.abs(info["mu"][0]) + np.abs(info["mu"][1]) + info["s"]
        gscale = np.stack([info["Phi"][o] * np.abs(info["dmu"][o]).max(axis=0) +
                           info["phi"] / (2 * info["s"]) * np.abs(info["ds2"][o]).max(axis=0) for o in range(2)])
        sv = np.abs(vs - val) / (8 * EPS * scale)
        sg = np.stack([np.abs(gs[D:] - grad[:D]).max(axis=0), np.abs(gs[:D] - grad[D:]).max(axis=0)]) / (8 * EPS * gscale + 1e-300)
        worst_sv, worst_sg = max(worst_sv, sv.max()), max(worst_sg, sg.max())
        assert np.all(sv <= 1.0) and np.all(sg <= 1.0), (M, sv.max(), sg.max())
    print(f"kernel {kernel} N {N} D {D} mode {mode}: largest error / bound: value {worst_v:.3g}, gradient {worst_g:.3g}; "
          f"swap: value {worst_sv:.3g}, gradient {worst_sg:.3g}")
    gp.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,N,D", [(SE, 90, 2), (MATERN52, 129, 8)])
def test_variance_of_the_difference_against_the_joint_covariance(m, ctx, same_route, kernel, N, D, mode):
    """The reference evaluated with s^2 = cov00 + cov11 - 2 cov01 of sls_gp_predict_cov at the two options: the device's value must
    agree within the value's bound (both routes know s^2 to tol_s2)."""
    X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, B, kernel)
    gp.set_sigma_mode(mode)
    M = 129
    P = np.random.default_rng(6).uniform(0, 1, (2 * D, M))
    pts = np.empty((D, 2 * M))
    pts[:, 0::2], pts[:, 1::2] = P[:D], P[D:]
    _, cov = gp.predict_cov(pts)
    i = np.arange(M)
    s2 = cov[2 * i, 2 * i] + cov[2 * i + 1, 2 * i + 1] - 2 * cov[2 * i, 2 * i + 1]
    val = gp.eubo_eval(P, want_grad=False)
    rv, _, info = eubo_ref.eubo(X, y, theta, B, kernel, P, s2=s2)
    tol_v, _ = tolerances(info, theta, N, np.abs(gp.matrix(m.GP_ALPHA)).max())
    own = np.abs(info["own_s2"] - s2).max() / (16 * info["cond"] * EPS * theta[0])
    print(f"kernel {kernel} N {N} mode {mode}: |s^2 (reference) - s^2 (predict_cov)| / tol_s2 {own:.3g}; "
          f"value error / bound {(np.abs(val - rv) / tol_v).max():.3g}")
    assert own <= 1.0
    assert np.all(np.abs(val - rv) <= tol_v)
    gp.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,N,D", [(SE, 90, 2), (MATERN52, 129, 8)])
def test_gradient_against_central_differences_of_device_values(m, ctx, kernel, N, D, mode):
    """h = 1e-5: the values carry ~1e-13 of noise (tol_v above), i.e. 1e-8 in the quotient, and the truncation h^2 f''' / 6 is of the
    same order at these length scales."""
    X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, B, kernel)
    gp.set_sigma_mode(mode)
    P = np.random.default_rng(9).uniform(0.05, 0.95, (2 * D, 8))
    _, grad = gp.eubo_eval(P)
    h = 1e-5
    for o in range(2):
        for d in range(min(D, 4)):
            E = np.zeros_like(P)
            E[o * D + d] = h
            fd = (gp.eubo_eval(P + E, want_grad=False) - gp.eubo_eval(P - E, want_grad=False)) / (2 * h)
            err = np.abs(fd - grad[o * D + d]).max()
            print(f"  option {o}, d = {d}: {err:.3g} (|grad| max {np.abs(grad).max():.3g})")
            assert err <= 1e-6 * (1.0 + np.abs(grad).max())
    gp.close()


def test_collapsed_pairs_take_the_guard(m, ctx, same_route):
    """x = x': d = 0 and k(x, x') = a exactly, so s^2 = 0 and the guard applies: the value is the mean there, bit for bit, and the
    gradient is zero.  b = 0 and two DIFFERENT data points: s^2 is rounding noise of either sign around 0; where it is not positive
    (or s < 1e-10) the device writes fmax(mu, mu') and the zero gradient, elsewhere a finite value that respects the invariant."""
    D, N = 2, 25
    g = np.linspace(0.05, 0.95, 5)
    X = np.array([[a, c] for a in g for c in g]).T.copy()
    y = np.sin(3 * X[0]) * np.cos(2 * X[1])
    theta = np.array([0.5, 0.15, 0.15])
    for mode in (0, 1):
        gp = m.GP(ctx, X, y, theta, 0.0, MATERN52)
        gp.set_sigma_mode(mode)
        rng = np.random.default_rng(4)
        same = np.concatenate([X[:, :10], rng.uniform(0, 1, (D, 10))], axis=1)
        P = np.concatenate([same, same], axis=0)
        val, grad = gp.eubo_eval(P)
        mu, _ = gp.predict(same)
        assert np.array_equal(val, mu) and np.array_equal(grad, np.zeros_like(grad))
        perm = (np.arange(N) + 7) % N
        P = np.concatenate([X, X[:, perm]], axis=0)
        val, grad = gp.eubo_eval(P)
        mu_all, _ = gp.predict(X)
        guarded = np.all(grad == 0.0, axis=0)
        print(f"mode {mode}: {guarded.sum()} of {N} data-point pairs take the guard")
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
        hi = np.maximum(mu_all, mu_all[perm])
        assert np.array_equal(val[guarded], hi[guarded])
        assert np.all(val >= hi - 1e-9)
        gp.close()


def test_bit_contract(m, ctx, monkeypatch):
    D, N, M = 5, 300, 300
    X, y, theta = problem(D, N, seed=21)
    for mode in (0, 1):
        gp = m.GP(ctx, X, y, theta, B, MATERN52)
        gp.set_sigma_mode(mode)
        rng = np.random.default_rng(3)
        P = rng.uniform(0, 1, (2 * D, M))
        val, grad = gp.eubo_eval(P)
        v2, g2 = gp.eubo_eval(P)
        assert np.array_equal(val, v2) and np.array_equal(grad, g2)                      # repeated call
        perm = rng.permutation(M)
        vp, gpm = gp.eubo_eval(P[:, perm])
        assert np.array_equal(vp, val[perm]) and np.array_equal(gpm, grad[:, perm])      # the column does not matter
        sub = np.array([7, 200, 131])
        vs, gs = gp.eubo_eval(P[:, sub])
        assert np.array_equal(vs, val[sub]) and np.array_equal(gs, grad[:, sub])         # nor do the other pairs
        ctx.set_candidate_chunk(256)                                                     # 128 pairs per pass: three passes
        vc, gc = gp.eubo_eval(P)
        ctx.set_candidate_chunk(16384)
        assert np.array_equal(vc, val) and np.array_equal(gc, grad)                      # nor the candidate chunk
        starts = rng.uniform(0, 1, (2 * D, 200))
        r1 = gp.eubo_maximize(starts, 12)
        monkeypatch.setenv("SLS_COMPACT", "0")
        r0 = gp.eubo_maximize(starts, 12)
        monkeypatch.delenv("SLS_COMPACT")
        assert np.array_equal(r1["x_stars"], r0["x_stars"]) and np.array_equal(r1["y_stars"], r0["y_stars"])
        assert r1["index"] == r0["index"] and r1["value"] == r0["value"]
        gp.close()


def test_maximiser_small(m, ctx):
    D, N, S, n_local = 1, 20, 256, 50
    X, y, theta = problem(D, N, seed=41, ell=0.3)
    gp = m.GP(ctx, X, y, theta, 0.01, SE)
    rng = np.random.default_rng(8)
    starts = rng.uniform(0, 1, (2 * D, S))
    r = gp.eubo_maximize(starts, n_local, offset=1000)
    g1 = np.linspace(0, 1, 401)
    G = np.stack(np.meshgrid(g1, g1, indexing="ij")).reshape(2, -1)
    grid_best = gp.eubo_eval(G, want_grad=False).max()
    print(f"winner {r['value']:.12g} at {r['x']}, maximum over the 401 x 401 grid of pairs {grid_best:.12g}")
    assert r["value"] >= grid_best - 1e-8
    x = r["x"]
    assert x.shape == (2 * D,) and np.all((x >= 0) & (x <= 1))
    v, g = gp.eubo_eval(x[:, None])
    assert abs(v[0] - r["value"]) <= 1e-12
    pg = np.where(((x <= 0) & (g[:, 0] < 0)) | ((x >= 1) & (g[:, 0] > 0)), 0.0, g[:, 0])    # maximisation: may push outwards
    print(f"  projected gradient {np.abs(pg).max():.3g}")
    assert np.abs(pg).max() <= 1e-5
    assert r["index"] - 1000 == int(np.argmax(r["y_stars"])) and r["value"] == r["y_stars"].max()
    assert np.array_equal(r["x_stars"][:, r["index"] - 1000], x)
    st = gp.last_stats()
    assert 0 < st["evals_issued"] <= S * n_local and st["evals_cap"] == S * n_local and st["rounds"] <= n_local
    gp.close()


@pytest.mark.parametrize("D", [8, 9, 32, 33])
def test_maximiser_at_the_switch_points_of_the_step_kernel(m, ctx, D):
    """2D = 16, 18, 64, 66 variables: either side of the two switch points of launch_lbfgs_step.  N = 90 and 128 starts is a shape that
    expected improvement runs in one launch (one wavefront per start); the pair objective always takes the lock-step rounds."""
    N, S, n_local = 90, 128, 12
    X, y, theta = problem(D, N, seed=60 + D, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, B, MATERN52)
    starts = np.random.default_rng(2).uniform(0, 1, (2 * D, S))
    at_start = gp.eubo_eval(starts, want_grad=False)
    ctx.prof_enable(True)
    ctx.prof_reset()
    r = gp.eubo_maximize(starts, n_local)
    st = gp.last_stats()
    launches = ctx.prof_get("eubo")[1]
    wave = ctx.prof_get("acq_wave")[1]
    ctx.prof_enable(False)
    assert 1 <= st["rounds"] <= n_local and launches == 2 * st["rounds"] and wave == 0
    assert np.isfinite(r["value"]) and np.all(np.isfinite(r["x_stars"])) and np.all(np.isfinite(r["y_stars"]))
    assert r["x_stars"].shape == (2 * D, S) and np.all((r["x_stars"] >= 0) & (r["x_stars"] <= 1))
    assert np.all((r["x"] >= 0) & (r["x"] <= 1))
    assert np.all(r["y_stars"] >= at_start)
    assert r["value"] == r["y_stars"].max() and np.array_equal(r["x_stars"][:, r["index"]], r["x"])
    print(f"D {D}: rounds {st['rounds']}, best start value {at_start.max():.6g} -> {r['value']:.6g}")
    # what depends on the DIRECTION: every start's trajectory against the restated L-BFGS on the device's own evaluations
    # (tests/test_gpu_maximize_restated.py; these starts are vetted on the CPU by tests/test_maximize_restated_seeds_cpu.py)
    rr = lbfgs_ref.run(gp.eubo_eval, starts, n_local, order="lanes")
    maximize_cases.hold_to_restatement(r, rr, f"eubo switch points D={D} uniform starts", stats=st, n_local=n_local)
    gp.close()


def test_argument_errors(m, ctx):
    D, N = 2, 30
    X, y, theta = problem(D, N, seed=9)
    gp = m.GP(ctx, X, y, theta, B, SE)
    lib, dp = m.lib(), C.POINTER(C.c_double)
    P = np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (2 * D, 3)))
    val, grad = np.empty(3), np.empty((2 * D, 3), order="F")
    p = lambda a: a.ctypes.data_as(dp)
    x, v, idx = np.empty(2 * D), C.c_double(), C.c_long()

    def ev(h, Pp, M, vp):
        return lib.sls_eubo_eval(h, Pp, M, vp, p(grad))

    def mx(h, sp, S=3, n_local=5, opts=None):
        return lib.sls_eubo_maximize(h, sp, S, n_local, opts, C.c_long(0), p(x), C.byref(v), C.byref(idx), None, None)

    def refused(rc, word):
        msg = lib.sls_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(ev(None, p(P), 3, p(val)), "gp is NULL")
    refused(ev(gp.h, None, 3, p(val)), "pairs is NULL")
    refused(ev(gp.h, p(P), -1, p(val)), "M = -1")
    refused(mx(None, p(P)), "gp is NULL")
    refused(mx(gp.h, None), "starts is NULL")
    refused(mx(gp.h, p(P), S=0), "S = 0")
    refused(mx(gp.h, p(P), n_local=0), "n_local = 0")
    opts = m.LbfgsOpts()
    opts.struct_size = 999
    refused(mx(gp.h, p(P), opts=C.byref(opts)), "struct_size")
    assert ev(gp.h, p(P), 0, None) == 0                            # M = 0: nothing to do
    assert ev(gp.h, p(P), 3, p(val)) == 0 and np.all(np.isfinite(val))
    g2 = grad.copy()
    assert ev(gp.h, p(P), 3, None) == 0 and np.array_equal(grad, g2)       # val may be NULL
    assert mx(gp.h, p(P)) == 0
    gp.close()
