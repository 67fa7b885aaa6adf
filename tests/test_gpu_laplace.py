"""The Laplace posterior for preference data on the device (include/sls_hip.h "Laplace posterior": sls_gp_set_laplace and every route
that reads the handle's variance) against the numpy restatement tests/laplace_ref.py.

Shapes: (N, D) = (40, 3) -- one tile, the plain fit is the single launch --, (130, 5) -- two tiles, ragged edge --, (300, 2) -- three
tiles; both kernels; b = 0.005 and 1e-6; btl_scale 0.01 and 1.0; both sigma modes; tuples of 2-4 options with a point in no tuple, a
point in at least 10 tuples and a tuple given twice; y the Newton mode of the restatement, and in the (300, 2) case a y that is NOT a
mode.  Query points: 50 and 200 (the latter crosses a 128-column tile).

Tolerances: the project's flat rtol = 1e-6, atol = 1e-8 (tests/test_gpu_parity.py) for sigma, UCB, EI, the summary and -- relative to
each matrix's largest entry -- W, Sigma_g and M; the gradient bound 2e-5 of a column's largest component; path values as
tests/test_gpu_path_sample.py holds them to path_ref."""
import ctypes as C

import numpy as np
import pytest
import torch      # before libsls_hip.so is loaded, as in tests/test_gpu_device_entry.py: the two then share one HIP runtime

import laplace_ref as lr
import lbfgs_ref
import maximize_cases as mc
import qbald_ref as br
import qeubo_ref as qr
from util import sls

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
RTOL, ATOL = 1e-6, 1e-8

# What a Laplace handle does on the entry points that may honour or refuse (mirrors the table in include/sls_hip.h).
MAY_REFUSE = {
    "sls_eubo_eval": "refuse", "sls_eubo_maximize": "refuse", "sls_acq_eval_pair": "refuse", "sls_acq_maximize_pair": "refuse",
    "sls_jes_create": "refuse", "sls_kg_create": "refuse", "sls_gp_loo": "refuse", "sls_multi_gp_create_from": "refuse",
    "sls_multi_acq_maximize": "refuse", "sls_multi_gp_predict": "refuse",      # when a shard carries the state and the others do not
}

#        name      N    D  kernel       b      s     sigma mode  y
SHAPES = [("n40", 40, 3, lr.MATERN52, 0.005, 0.01, 0, "map"),
          ("n130", 130, 5, lr.SE, 1e-6, 1.0, 1, "map"),
          ("n300", 300, 2, lr.MATERN52, 0.005, 0.01, 0, "any"),
          ("n130m", 130, 5, lr.MATERN52, 0.005, 0.01, 1, "map")]
NAMES = [s[0] for s in SHAPES]


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


class Case:
    pass


@pytest.fixture(scope="module")
def cases(m, ctx):
    """Per shape: the restatement, a plain handle, a Laplace handle and the query points -- built once, left unchanged."""
    out = {}
    for name, N, D, kernel, b, s, mode, ykind in SHAPES:
        rng = np.random.default_rng(1000 + N + D)
        c = Case()
        c.name, c.N, c.D, c.kernel, c.b, c.s, c.mode = name, N, D, kernel, b, s, mode
        c.X = rng.uniform(0, 1, (D, N))
        c.theta = np.full(D + 1, 0.5)
        c.prefs = lr.example_prefs(N, rng)
        c.y = lr.newton_map(c.X, c.theta, b, kernel, c.prefs, s) if ykind == "map" else 0.3 * rng.normal(size=N)
        c.ref = lr.LaplaceRef(c.X, c.y, c.theta, b, kernel, c.prefs, s)
        c.plain = m.GP(ctx, c.X, c.y, c.theta, b, kernel)
        c.plain.set_sigma_mode(mode)
        c.gp = m.GP(ctx, c.X, c.y, c.theta, b, kernel)
        c.gp.set_sigma_mode(mode)
        c.gp.set_laplace(c.prefs, s)
        c.Xs = {M: np.random.default_rng(7 + M).uniform(0.02, 0.98, (D, M)) for M in (50, 200)}
        out[name] = c
    yield out
    for c in out.values():
        c.gp.close()
        c.plain.close()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def close_rel_to_max(A, R, what):
    scale = np.abs(R).max()
    err = np.abs(A - R) / scale
    print(f"{what}: largest |device - reference| / largest entry = {err.max():.3e}")
    assert np.all(err <= ATOL + RTOL * np.abs(R) / scale), (what, err.max())


@pytest.mark.parametrize("name", NAMES)
def test_matrices_and_summary(m, cases, name):
    c = cases[name]
    W, S, Mx = (c.gp.laplace_matrix(w) for w in (m.LAPLACE_W, m.LAPLACE_COV, m.LAPLACE_M))
    close_rel_to_max(W, c.ref.W, name + " W")
    close_rel_to_max(S, c.ref.cov_g, name + " Sigma_g")
    close_rel_to_max(Mx, c.ref.M, name + " M")
    for A in (W, S, Mx):
        assert np.array_equal(bits(A), bits(A.T))
    assert not W[c.N - 1].any() and not W[:, c.N - 1].any()          # the point in no tuple
    sm = c.gp.laplace_summary()
    print(name, sm, c.ref.log_lik, c.ref.logdet_B, c.ref.log_evidence)
    np.testing.assert_allclose(sm["log_lik"], c.ref.log_lik, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(sm["logdet_B"], c.ref.logdet_B, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(sm["log_evidence"], c.ref.log_evidence, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("M", [50, 200])
@pytest.mark.parametrize("name", NAMES)
def test_predictions_and_acquisitions(m, cases, monkeypatch, name, M):
    c = cases[name]
    Xs = c.Xs[M]
    mu, sg = c.gp.predict(Xs)
    mu_r, sg_r = c.ref.predict(Xs)
    print(f"{name} M {M}: sigma err {np.abs(sg - sg_r).max():.3e}, median Laplace sigma {np.median(sg):.3f}, plain {np.median(c.ref.plain_sigma(Xs)):.3f}")
    np.testing.assert_allclose(sg, sg_r, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(mu, mu_r, rtol=RTOL, atol=ATOL)
    # the mean is the plain handle's, bit for bit, on the same (tiled) route
    monkeypatch.setenv("SLS_WAVE_PATH", "0")
    mu_p, sg_p = c.plain.predict(Xs)
    assert np.array_equal(bits(mu), bits(mu_p))
    assert np.all(sg >= sg_p - ATOL)
    ucb = c.gp.acq_eval(Xs, m.ACQ_UCB, 1.5, want_grad=False)
    np.testing.assert_allclose(ucb, c.ref.acq(Xs, 1, 1.5), rtol=RTOL, atol=ATOL)
    assert abs(c.gp.summary()["mu_best"] - c.ref.mu_best) <= 1e-8
    ei = c.gp.acq_eval(Xs, m.ACQ_EI, want_grad=False)
    np.testing.assert_allclose(ei, c.ref.acq(Xs, 0), rtol=RTOL, atol=ATOL)
    # with and without the gradient the tiled route gives one sigma
    ei_g, _ = c.gp.acq_eval(Xs, m.ACQ_EI)
    np.testing.assert_allclose(ei_g, ei, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", NAMES)
def test_sigma_gradient(cases, name):
    c = cases[name]
    Xs = c.Xs[50]
    dmu, dsg = c.gp.predict_grad(Xs)
    dmu_r, dsg_r = c.ref.predict_grad(Xs)
    colmax = np.abs(dsg_r).max(axis=0, keepdims=True)
    print(f"{name}: grad sigma err / column max {np.max(np.abs(dsg - dsg_r) / colmax):.3e}")
    assert np.all(np.abs(dsg - dsg_r) <= 2e-5 * colmax + 1e-12)
    assert np.all(np.abs(dmu - dmu_r) <= 2e-5 * np.abs(dmu_r).max(axis=0, keepdims=True) + 1e-12)
    h = 1e-5
    for d in range(c.D):
        E = np.zeros_like(Xs)
        E[d] = h
        fd = (c.gp.predict(Xs + E)[1] - c.gp.predict(Xs - E)[1]) / (2 * h)
        assert np.all(np.abs(fd - dsg[d]) <= 2e-5 * colmax[0] + 1e-9), (d, np.max(np.abs(fd - dsg[d]) / colmax[0]))


@pytest.mark.parametrize("M", [50, 200])
@pytest.mark.parametrize("name", NAMES)
def test_joint_posterior(cases, name, M):
    c = cases[name]
    Xs = c.Xs[M]
    mu, cov = c.gp.predict_cov(Xs)
    cov_r = c.ref.cov(Xs)
    print(f"{name} M {M}: cov err {np.abs(cov - cov_r).max():.3e}")
    np.testing.assert_allclose(cov, cov_r, rtol=RTOL, atol=ATOL)
    assert np.array_equal(bits(cov), bits(cov.T))
    _, sg = c.gp.predict(Xs)
    np.testing.assert_allclose(np.diag(cov), sg * sg, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(mu, c.gp.predict(Xs)[0], rtol=1e-12, atol=1e-14)
    if M == 50:
        f5 = c.gp.sample_posterior(Xs, 5, seed=11)[0]
        f2 = c.gp.sample_posterior(Xs, 2, seed=11)[0]
        assert f5.shape == (M, 5) and np.array_equal(bits(f5[:, :2]), bits(f2))
        assert np.array_equal(bits(f5), bits(c.gp.sample_posterior(Xs, 5, seed=11)[0]))
        assert not np.array_equal(f5, c.plain.sample_posterior(Xs, 5, seed=11)[0])


def test_path_draws(m, ctx, cases):
    c = cases["n130m"]
    F, seed = 64, 4242
    before = m.PathSamples(c.plain, 4, F, seed=seed)          # a handle the state never touched
    ps4, ps2 = m.PathSamples(c.gp, 4, F, seed=seed), m.PathSamples(c.gp, 2, F, seed=seed)
    ref = lr.LaplacePathRef(c.ref, 4, F, seed)
    Xq = np.concatenate([c.X, c.Xs[50]], axis=1)
    v4, v2 = ps4.eval_all(Xq), ps2.eval_all(Xq)
    ev = np.linalg.eigvalsh(ref.Ky)
    cond, vs, a = ev[-1] / ev[0], np.abs(ref.v).max(), c.theta[0]
    tol_v = 1e-10 * a + 4 * cond * EPS * vs * a * np.sqrt(c.N)
    err = np.abs(v4 - ref.eval_all(Xq)).max()
    print(f"path: err {err:.3e}, tolerance {tol_v:.3e}, cond {cond:.3e}")
    assert err <= tol_v
    assert np.array_equal(bits(v4[:, :2]), bits(v2))
    dr = np.arange(Xq.shape[1]) % 4
    val, grad = ps4.eval(Xq, dr)
    rv, rg = ref.eval(Xq, dr)
    assert np.abs(val - rv).max() <= tol_v
    assert np.abs(grad - rg).max() <= 1e-9 * a + 4 * cond * EPS * vs * a * np.sqrt(c.N) / c.theta[1:].min()
    # the draws differ from the plain handle's: the goodness vector is sampled too
    assert np.abs(v4 - before.eval_all(Xq)).max() > 1e-3
    # set then clear on another handle: the plain 2F + N layout is back, bit for bit
    g2 = m.GP(ctx, c.X, c.y, c.theta, c.b, c.kernel)
    g2.set_sigma_mode(c.mode)
    g2.set_laplace(c.prefs, c.s)
    g2.clear_laplace()
    after = m.PathSamples(g2, 4, F, seed=seed)
    assert np.array_equal(bits(after.eval_all(Xq)), bits(before.eval_all(Xq)))
    for p in (before, ps4, ps2, after):
        p.close()
    g2.close()


def test_criteria_on_laplace_draws(m, cases):
    """qEUBO and qBALD only consume the object's (W, V): on a Laplace path object they equal the restatements evaluated on that
    object's own eval_all values."""
    c = cases["n130m"]
    F, seed, q, S, nsets = 64, 99, 3, 8, 40
    ps = m.PathSamples(c.gp, S, F, seed=seed)

    class OnDevice(lr.LaplacePathRef):
        def eval_all(self, Xs):
            return ps.eval_all(Xs)
    ref = OnDevice(c.ref, S, F, seed)
    # the criteria form the draws' values on another product than eval_all: held as tests/test_gpu_qeubo.py holds that consistency
    ev = np.linalg.eigvalsh(ref.Ky)
    tol_v = 1e-10 * c.theta[0] + 4 * (ev[-1] / ev[0]) * EPS * np.abs(ref.v).max() * c.theta[0] * np.sqrt(c.N)
    sets = np.random.default_rng(5).uniform(0, 1, (q * c.D, nsets))
    val = ps.qeubo_eval(sets, q, want_grad=False)
    rv, _, _, gap = qr.qeubo(ref, sets, q)
    ok = gap > 100 * tol_v
    assert ok.sum() >= nsets - 2
    print(f"qeubo on Laplace draws: err {np.abs(val - rv)[ok].max():.3e}, tolerance {tol_v:.3e}")
    assert np.abs(val - rv)[ok].max() <= tol_v
    tau = 0.05
    bv = ps.qbald_eval(sets, q, scale=tau, want_grad=False)
    V = np.stack([ps.eval_all(sets[i * c.D:(i + 1) * c.D]) for i in range(q)])
    rb, cw, _, _ = br.weights(V, tau)
    amp = np.abs(cw).sum(axis=(0, 2))                  # |d value / d V| summed: what an error of tol_v in every value may do
    print(f"qbald on Laplace draws: err {np.abs(bv - rb).max():.3e}, tolerance {(2 * amp * tol_v + 1e-12).min():.3e}")
    assert np.all(np.abs(bv - rb) <= 2 * amp * tol_v + 1e-12)
    ps.close()


def test_maximiser_start_by_start(m, cases):
    c = cases["n130m"]
    starts = np.random.default_rng(21).uniform(0, 1, (c.D, 64))
    rg = c.gp.acq_maximize(starts, 10, m.ACQ_EI)
    st = c.gp.last_stats()
    rr = lbfgs_ref.run(lambda T: c.gp.acq_eval(T, m.ACQ_EI), starts, 10)
    mc.hold_to_restatement(rg, rr, "laplace EI n130m", stats=st, n_local=10)
    # the plain handle's search is another search
    rp = c.plain.acq_maximize(starts, 10, m.ACQ_EI)
    assert not np.array_equal(rp["y_stars"], rg["y_stars"])


def snapshot(m, gp, c):
    Xs = c.Xs[50]
    ps = m.PathSamples(gp, 2, 32, seed=3)
    out = (gp.predict(Xs), gp.acq_eval(Xs, m.ACQ_EI), gp.predict_cov(Xs), ps.eval_all(Xs))
    ps.close()
    return [bits(np.concatenate([np.ravel(a) for a in part])) if isinstance(part, tuple) else bits(part) for part in out]


@pytest.mark.parametrize("name", ["n40", "n130"])
def test_state_lifecycle(m, ctx, cases, name):
    c = cases[name]
    want_plain, want_lap = snapshot(m, c.plain, c), snapshot(m, c.gp, c)
    g = m.GP(ctx, c.X, c.y, c.theta, c.b, c.kernel)
    g.set_sigma_mode(c.mode)
    gen0 = g.generation()
    other = [tuple(reversed(p)) for p in c.prefs[:-5]]
    g.set_laplace(other, 2.0 * c.s)
    gen1 = g.generation()
    g.set_laplace(c.prefs, c.s)                      # set twice = a fresh set
    gen2 = g.generation()
    got = snapshot(m, g, c)
    assert all(np.array_equal(a, b) for a, b in zip(got, want_lap))
    g.clear_laplace()
    gen3 = g.generation()
    assert len({gen0, gen1, gen2, gen3}) == 4
    got = snapshot(m, g, c)
    assert all(np.array_equal(a, b) for a, b in zip(got, want_plain))
    with pytest.raises(m.SlsError):
        g.laplace_summary()
    g.clear_laplace()                                # no state: a no-op
    assert g.generation() == gen3
    g.close()


def test_frozen_fit(m, cases):
    c = cases["n40"]
    Xs = c.Xs[50]
    before = [bits(a) for a in c.gp.predict(Xs)]
    gen = c.gp.generation()
    with pytest.raises(m.Unsupported):
        c.gp.set_sigma_mode(1 - c.mode)
    with pytest.raises(m.Unsupported):
        c.gp.append_point(np.full(c.D, 0.5), 0.1)
    assert c.gp.N == c.N
    Xd = torch.from_numpy(np.ascontiguousarray(c.X.T)).to("cuda")      # D x N column-major = N x D in C order
    yd = torch.from_numpy(np.ascontiguousarray(c.y)).to("cuda")
    torch.cuda.synchronize()
    with pytest.raises(m.Unsupported):
        c.gp.refit_dev(Xd.data_ptr(), yd.data_ptr())
    assert c.gp.generation() == gen
    assert all(np.array_equal(a, bits(b)) for a, b in zip(before, c.gp.predict(Xs)))


def test_may_honour_or_refuse(m, ctx, cases):
    """No entry point uses the plain variance on a Laplace handle: each of these raises Unsupported, as the header's table says."""
    c = cases["n40"]
    D = c.D
    Xs = c.Xs[50]
    pairs = np.concatenate([Xs, Xs[:, ::-1]], axis=0)
    calls = {
        "sls_eubo_eval": lambda: c.gp.eubo_eval(pairs),
        "sls_eubo_maximize": lambda: c.gp.eubo_maximize(pairs, 3),
        "sls_acq_eval_pair": lambda: c.plain.acq_eval_pair(c.gp, Xs),
        "sls_acq_maximize_pair": lambda: c.gp.acq_maximize_pair(c.plain, Xs, 3),
        "sls_jes_create": lambda: c.gp.jes_create(Xs[:, :4], np.zeros(4)),
        "sls_kg_create": lambda: c.gp.kg_create(Xs[:, :4]),
        "sls_gp_loo": lambda: c.gp.loo(),
    }
    assert set(calls) | {"sls_multi_gp_create_from", "sls_multi_acq_maximize", "sls_multi_gp_predict"} == set(MAY_REFUSE)
    for name, call in calls.items():
        assert MAY_REFUSE[name] == "refuse"
        with pytest.raises(m.Unsupported) as e:
            call()
        assert "Laplace" in str(e.value), name
    multi = m.Multi([0, 0])
    out = C.c_void_p()
    assert m.lib().sls_multi_gp_create_from(multi.h, c.gp.h, C.byref(out)) == m.ERR_UNSUPPORTED
    assert "Laplace" in m.lib().sls_last_error().decode()
    # replicas made from a plain handle that is given the state AFTERWARDS: the borrowed shard would search on the Laplace variance and
    # the other shard on the plain one -- refused, and served again once the state is cleared
    g2 = m.GP(ctx, c.X, c.y, c.theta, c.b, c.kernel)
    L = m.lib()
    assert L.sls_multi_gp_create_from(multi.h, g2.h, C.byref(out)) == 0
    dp = C.POINTER(C.c_double)
    starts = np.asfortranarray(Xs[:, :8])
    x, val, idx, mu2 = np.empty(D), C.c_double(), C.c_long(), np.empty(8)

    def maximise():
        return L.sls_multi_acq_maximize(out, m.ACQ_EI, C.c_double(1.0), starts.ctypes.data_as(dp), 8, 3, None, x.ctypes.data_as(dp),
                                        C.byref(val), C.byref(idx), None)

    def predict():
        return L.sls_multi_gp_predict(out, starts.ctypes.data_as(dp), 8, mu2.ctypes.data_as(dp), None)
    assert maximise() == 0 and predict() == 0
    g2.set_laplace(c.prefs, c.s)
    assert maximise() == m.ERR_UNSUPPORTED and "Laplace" in L.sls_last_error().decode()
    assert predict() == m.ERR_UNSUPPORTED
    g2.clear_laplace()
    assert maximise() == 0 and predict() == 0
    L.sls_multi_gp_destroy(out)
    g2.close()
    multi.close()
    # the handle still answers, and the plain handle still takes every one of them
    assert np.isfinite(c.gp.predict(Xs)[1]).all()
    c.plain.eubo_eval(pairs)
    c.plain.loo()


def test_invalid_input_leaves_the_handle_unchanged(m, ctx, cases):
    c = cases["n40"]
    Xs = c.Xs[50]
    for gp in (c.gp, c.plain):
        before = [bits(a) for a in gp.predict(Xs)]
        gen = gp.generation()
        for prefs, s in (([(0, c.N)], 0.01), ([(0, 1), (2,)], 0.01), ([], 0.01), ([(0, 1)], 0.0), ([(0, 1)], -1.0), ([(0, 1)], float("nan"))):
            with pytest.raises(m.SlsError) as e:
                gp.set_laplace(prefs, s)
            assert e.value.code == m.ERR_INVALID, (prefs, s)
        assert gp.generation() == gen
        assert all(np.array_equal(a, bits(b)) for a, b in zip(before, gp.predict(Xs)))
    with pytest.raises(m.SlsError):
        c.plain.laplace_matrix(m.LAPLACE_W)


@pytest.mark.parametrize("name", ["n40", "n300"])
def test_determinism(m, ctx, cases, name):
    c = cases[name]
    g = m.GP(ctx, c.X, c.y, c.theta, c.b, c.kernel)
    g.set_sigma_mode(c.mode)
    g.set_laplace(c.prefs, c.s)
    for w in (m.LAPLACE_W, m.LAPLACE_COV, m.LAPLACE_M):
        assert np.array_equal(bits(g.laplace_matrix(w)), bits(c.gp.laplace_matrix(w)))
    assert g.laplace_summary() == c.gp.laplace_summary()
    g.close()


def test_profiler_scopes(m, ctx, cases):
    c = cases["n300"]
    g = m.GP(ctx, c.X, c.y, c.theta, c.b, c.kernel)
    ctx.prof_enable(True)
    ctx.prof_reset()
    g.set_laplace(c.prefs, c.s)
    counts = {k: ctx.prof_get(k)[1] for k in ("laplace_w", "laplace_b", "laplace_potri", "laplace_m")}
    g.predict(c.Xs[50])
    wave = ctx.prof_get("acq_wave")[1]
    ctx.prof_enable(False)
    assert all(v >= 1 for v in counts.values()), counts
    assert wave == 0
    g.close()
