"""Path draws, set criteria, EUBO pairs, posterior samples and the LogEI / MES / pair combiners on handles whose fit lies beyond the
guard of the norm expansion, against the direct-difference, extended-precision reference of tests/path_short_ref.py.

The handle's gram_direct flag sends the cross Gram of sls_path_eval / _maximize (point-major and candidate-major strides, chunk
offset), of the draw values behind sls_qeubo_eval / sls_qnei_eval / sls_line_eval (option-major offsets), of
sls_path_max_over_points, of the EUBO pairs (with the gradient's raw-difference contraction per option) and of the posterior
covariance behind sls_gp_sample_posterior to the direct form.  A wrong stride, offset, leading dimension or Matern C pointer in any
of these calls is an O(1) error that no test at ordinary length scales sees.

Cases (path_short_ref.CASES): gram_ref.problem at (N, D) in {(129, 6), (300, 33), (200, 65)}, l in {0.3 (inside the guard), 3e-3,
1e-5, 1e-8, one ARD case}, l = 0.02 at D = 65 (just beyond the guard), both kernels, F = 200, 5 draws and one case of 130; the points
are gram_ref's 40 candidates (ordinary, outside the box, 0.7 scaled units from a training point, a near-duplicate pair).  And
gram_ref.WIDE_CASES: D = 129, 192, 257 on both sides of the guard, where the feature and gradient kernels run over two and three
128-column tiles and every route is the tiled one.

Tolerances, one scheme (path_short_ref.reference): the tolerance the entry point's ordinary restatement test uses (tol_v / tol_g of
test_eval_agrees_with_the_restatement, the tolerances() of test_gpu_eubo.py) with this case's cond(K_y), |v| and shortest length
scale, plus 16 bands, band = max |float64 - longdouble| of the reference itself for that case and quantity: device and restatement
are two fp64 evaluations of one expression in different summation orders, which scatter by about an order of magnitude around the
restatement's own rounding.  The device is never compared with itself to set a tolerance.  Winners (wins, arg) are compared exactly
where the longdouble reference's winner leads by 100 value tolerances (at most 10 % of a case's sets do not:
tests/test_path_short_ref_cpu.py).  Every case records error, band and tolerance per quantity (kind "short_length_scales_paths").

Measured on MI355X (profiles/short_length_scales_paths.json): see DESIGN.md 9a."""
import numpy as np
import pytest

import gram_ref as gr
import line_ref as lr
import mes_ref
import path_short_ref as sr
import qeubo_ref as qr
import qnei_ref as nr
from test_gpu_eubo import tolerances as eubo_tolerances
from test_gpu_logei import assert_matches_restatement as assert_logei_matches, device_posterior
from test_gpu_mes import max_value_samples
from util import env_switch, record, sls

pytestmark = pytest.mark.gpu
EPS = gr.EPS
KIND = "short_length_scales_paths"
CASE_IDS = [f"N{N}-D{D}-l{case}-nd{nd}" for (N, D, case, nd) in sr.CASES]
FIVE = [c for c in sr.CASES if c[3] == 5]
FIVE_IDS = [f"N{N}-D{D}-l{case}" for (N, D, case, _) in FIVE]


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def handles(m, ctx, r, sigma_mode=0):
    gp = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], r["kernel"])
    if sigma_mode:
        gp.set_sigma_mode(sigma_mode)
    return gp, m.PathSamples(gp, r["nd"], sr.F, seed=r["seed"])


def err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble)).max())


def hold(r, route, items, **extra):
    """items: name -> (device array, reference array, tolerance, band).  Records every figure, then asserts every one."""
    errors = {k: err(g, ref) for k, (g, ref, _, _) in items.items()}
    record(KIND, route=route, N=r["N"], D=r["D"], ell=str(r["case"]), kernel=r["kernel"], n_draws=r["nd"], errors=errors,
           band={k: float(v[3]) for k, v in items.items()}, tolerance={k: float(v[2]) for k, v in items.items()},
           scale={k: float(np.abs(np.asarray(v[1], dtype=np.float64)).max()) for k, v in items.items()}, **extra)
    for k, (_, _, tol, _) in items.items():
        assert errors[k] <= tol, (route, k, errors[k], tol)


def item(r, got, key, ref=None, tol=None):
    return (got, r["q80"][key] if ref is None else ref, r["tol"][key] if tol is None else tol, r["band"][key])


# ---- a, b: the path entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case,nd", sr.CASES, ids=CASE_IDS)
def test_path_eval_and_the_identity_at_the_data(m, ctx, N, D, case, nd, kernel):
    """sls_path_eval, gathered (value, gradient) and every-draw, against the reference and against each other; and
    f_s(x_i) = y_i - sqrt(b) eps_{s,i} - b v_{s,i} at the training points with v from the longdouble reference."""
    r = sr.reference(N, D, case, kernel, nd)
    assert sr.beyond_guard(r["ell"], D) == ((N, D, case) not in sr.INSIDE)
    gp, ps = handles(m, ctx, r)
    dr = sr.draws_of_points(gr.N_CAND, nd)
    val, grad = ps.eval(r["Xs"], dr)
    allv = ps.eval_all(r["Xs"])
    at_data = ps.eval_all(r["X"])
    ps.close()
    gp.close()
    # the identity's right-hand side moves by b |dv|: v's own tolerance is cond eps |v|, the term the value tolerance carries
    hold(r, "path_eval", dict(val=item(r, val, "val"), grad=item(r, grad, "grad"), all=item(r, allv, "all"),
                              gathered_vs_all=item(r, allv[np.arange(gr.N_CAND), dr], "val", ref=val, tol=r["tol"]["val"]),
                              identity=item(r, at_data, "all", ref=r["ref80"].data_identity())),
         grad_band_prior=r["band"]["grad_prior"], grad_band_data=r["band"]["grad_data"])


# ---- d, e: the set criteria and the per-draw maximum ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case,nd", sr.CASES, ids=CASE_IDS)
def test_max_over_points_qeubo_and_qnei(m, ctx, N, D, case, nd, kernel):
    """sls_path_max_over_points at Xb = X (N = 300: three 128-point blocks), then sls_qeubo_eval and sls_qnei_eval (value, gradient,
    wins) at q = 2, 5, 16 with the device's own baseline on both sides."""
    r = sr.reference(N, D, case, kernel, nd)
    ref, q80 = r["ref80"], r["q80"]
    gp, ps = handles(m, ctx, r)
    t, arg = ps.max_over_points(r["X"])
    items = dict(t=item(r, t, "t"))
    kept_t = r["kept"]["t"]
    checks = [("t_arg", np.array_equal(arg[kept_t], q80["t_arg"][kept_t]))]
    dropped = dict(t=float((~kept_t).mean()))
    for q in sr.QS:
        sets = sr.sets_of(r["Xs"], q)
        val, grad, wins = ps.qeubo_eval(sets, q, want_wins=True)
        kept = r["kept"][f"qeubo{q}"]
        items[f"qeubo{q}_val"] = item(r, val[kept], f"qeubo{q}_val", ref=q80[f"qeubo{q}_val"][kept])
        items[f"qeubo{q}_grad"] = item(r, grad[:, kept], f"qeubo{q}_grad", ref=q80[f"qeubo{q}_grad"][:, kept])
        checks.append((f"qeubo{q}_wins", np.array_equal(wins[:, kept], q80[f"qeubo{q}_wins"][:, kept]) and np.all(wins.sum(axis=0) == nd)))
        dropped[f"qeubo{q}"] = float((~kept).mean())
        # qNEI at the baseline the device formed, on both sides
        val, grad, wins = ps.qnei_eval(sets, q, t, want_wins=True)
        rv, rg, rw, gap = nr.qnei(ref, sets, q, t)
        kept = gap >= r["margin"]
        assert (~kept).mean() <= sr.MAX_DROPPED, (q, float((~kept).mean()))
        items[f"qnei{q}_val"] = item(r, val[kept], f"qnei{q}_val", ref=rv[kept])
        items[f"qnei{q}_grad"] = item(r, grad[:, kept], f"qnei{q}_grad", ref=rg[:, kept])
        checks.append((f"qnei{q}_wins", np.array_equal(wins[:, kept], rw[:, kept]) and np.all(wins.sum(axis=0) <= nd)))
        dropped[f"qnei{q}"] = float((~kept).mean())
    ps.close()
    gp.close()
    hold(r, "sets", items, dropped=dropped, exact={k: bool(v) for k, v in checks})
    assert all(ok for _, ok in checks), checks


# ---- f: the line route -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchored", [False, True], ids=["free", "anchored"])
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case,nd", FIVE, ids=FIVE_IDS)
def test_line_bits_are_those_of_the_set_routes(m, ctx, N, D, case, nd, kernel, anchored):
    """The contract of test_bits_are_those_of_the_set_routes on the same guarded handle: value and wins of sls_line_eval are those of
    sls_qeubo_eval / sls_qnei_eval at the expanded set, the gradient is the folded set gradient."""
    r = sr.reference(N, D, case, kernel, nd)
    gp, ps = handles(m, ctx, r)
    lines, anchor = sr.lines_of(r["Xs"], anchored)
    sets = lr.expand(lines, sr.LINE_Q, D, anchor)
    t = ps.max_over_points(r["X"])[0]
    for base in (None, t):
        val, grad, wins = ps.line_eval(lines, sr.LINE_Q, anchor=anchor, baseline=base, want_wins=True)
        sv, sg, sw = ps.qeubo_eval(sets, sr.LINE_Q, want_wins=True) if base is None else ps.qnei_eval(sets, sr.LINE_Q, base, want_wins=True)
        assert same(val, sv) and np.array_equal(wins, sw)
        assert same(grad, lr.fold(sg, sr.LINE_Q, D, anchored=anchored))
    # and the set route itself is held to the reference at these sets
    rv, rg, rw, gap = lr.line(r["ref80"], lines, sr.LINE_Q, anchor)
    v64, g64, _, _ = lr.line(r["ref64"], lines, sr.LINE_Q, anchor)
    band_v, band_g = err(v64, rv), err(g64, rg)
    kept = gap >= r["margin"]
    assert (~kept).mean() <= sr.MAX_DROPPED
    val, grad, wins = ps.line_eval(lines, sr.LINE_Q, anchor=anchor, want_wins=True)
    ps.close()
    gp.close()
    hold(r, "line_anchored" if anchored else "line",
         dict(val=(val[kept], rv[kept], r["tol_v"] + sr.BAND_FACTOR * band_v, band_v),
              grad=(grad[:, kept], rg[:, kept], r["tol_g"] + sr.BAND_FACTOR * band_g, band_g)))
    assert np.array_equal(wins[:, kept], rw[:, kept])


# ---- g: EUBO pairs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case,nd", FIVE, ids=FIVE_IDS)
def test_eubo_pairs(m, ctx, N, D, case, nd, kernel, mode):
    """sls_eubo_eval on (ordinary, ordinary), (near a training point, ordinary), (outside the box, ordinary) and the near-duplicate
    pair against eubo_ref's closed form on the longdouble posterior, with the bounds of test_gpu_eubo.py plus 16 bands, per pair."""
    r = sr.reference(N, D, case, kernel, nd)
    e = sr.eubo_reference(N, D, case, kernel)
    rv, rg, info = e["e80"]
    gp = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], kernel)
    gp.set_sigma_mode(mode)
    alpha_max = np.abs(gp.matrix(m.GP_ALPHA)).max()
    val, grad = gp.eubo_eval(e["pairs"])
    gp.close()
    tol_v, tol_g = eubo_tolerances(info, np.asarray(r["theta"]), N, alpha_max)
    tol_v = tol_v + sr.BAND_FACTOR * e["band"]["val"]
    tol_g = 1e-9 * np.abs(rg).max(axis=0)[None, :] + tol_g + sr.BAND_FACTOR * e["band"]["grad"]
    ev = np.abs(val - rv)
    eg = np.stack([np.abs(grad[:D] - rg[:D]).max(axis=0), np.abs(grad[D:] - rg[D:]).max(axis=0)])
    k = sr.PAIR_NAMES.index("near_duplicate")
    record(KIND, route="eubo", N=N, D=D, ell=str(case), kernel=kernel, sigma_mode=mode, pairs=list(sr.PAIR_NAMES),
           errors=dict(val=[float(v) for v in ev], grad=[float(v) for v in eg.max(axis=0)]),
           band=dict(val=[float(v) for v in e["band"]["val"]], grad=[float(v) for v in e["band"]["grad"].max(axis=0)]),
           tolerance=dict(val=[float(v) for v in tol_v], grad=[float(v) for v in tol_g.min(axis=0)]),
           scale=dict(val=[float(v) for v in np.abs(rv)], grad=[float(v) for v in np.abs(rg).max(axis=0)]),
           near_duplicate=dict(val=float(ev[k]), grad=float(eg[:, k].max()), s=float(info["s"][k]), tol_val=float(tol_v[k]),
                               tol_grad=float(tol_g[:, k].min())))
    assert np.all(ev <= tol_v), (ev / tol_v)
    assert np.all(eg <= tol_g), (eg / tol_g)


# ---- c: chunk crossing in the direct form ------------------------------------------------------------------------------------------------
def chunk_problem(kernel):
    """test_eval_across_a_chunk_boundary's shape at l = 3e-3 (beyond the guard at D = 3); every candidate sits 0.7 scaled units from a
    training point, so that the data term is there at every column on both sides of the boundary."""
    F, N, D, nd, M, b = 16384, 90, 3, 3, 2200, 0.05
    rng = np.random.default_rng(400 + kernel)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], 3e-3 * rng.uniform(0.8, 1.25, D)])
    Xs = np.clip(X[:, rng.integers(0, N, M)] + theta[1:, None] * 0.7 * rng.standard_normal((D, M)) / np.sqrt(D), 0.0, 1.0)
    return F, N, D, nd, M, b, X, y, theta, Xs, rng


@pytest.mark.parametrize("kernel", [0, 1])
def test_eval_across_a_chunk_boundary_in_the_direct_form(m, ctx, kernel):
    """M = 2200 candidates at F = 16384: chunks of 2048, columns 2048 .. 2199 are a second, ragged chunk (s0 > 0 in the direct cross
    Gram's candidate pointer).  The assertions of test_eval_across_a_chunk_boundary, against the direct-difference reference."""
    import path_ref as ph
    F, N, D, nd, M, b, X, y, theta, Xs, rng = chunk_problem(kernel)
    assert sr.beyond_guard(theta[1:], D)
    chunk = ph.eval_chunk(ph.round_up(N, 128), ph.round_up(F, 128))
    assert chunk == 2048 and chunk < M < 2 * chunk and (M - chunk) % 128 != 0
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=77)
    ref = sr.ShortPathRef(X, y, theta, b, kernel, nd, F, 77)
    tol_v, tol_g, cond = sr.tolerances(ref)
    dr = rng.integers(0, nd, M)
    dr[chunk - 2:chunk + 3] = [0, 1, 2, 1, 0]
    val, grad = ps.eval(Xs, dr)
    allv = ps.eval_all(Xs)
    sl = slice(1900, 2200)
    rv, rg = ref.eval(Xs[:, sl], dr[sl])
    rall = ref.eval_all(Xs[:, sl])
    err_v, err_g, err_all = np.abs(val[sl] - rv).max(), np.abs(grad[:, sl] - rg).max(), np.abs(allv[sl] - rall).max()
    record(KIND, route="chunk_boundary", kernel=kernel, errors=dict(val=float(err_v), grad=float(err_g), all=float(err_all)),
           tolerance=dict(val=tol_v, grad=tol_g, all=tol_v), data_term=float(np.abs(ref.data_all(Xs[:, sl])).max()))
    assert np.abs(ref.data_all(Xs[:, sl])).max() > 0.1 * theta[0]          # the data term is there
    assert err_v <= tol_v, (err_v, tol_v, cond)
    assert err_g <= tol_g, (err_g, tol_g, cond)
    assert err_all <= tol_v, (err_all, tol_v, cond)
    assert np.abs(allv[np.arange(M), dr] - val).max() <= tol_v
    tail = slice(chunk, M)
    v2, g2 = ps.eval(Xs[:, tail], dr[tail])
    assert v2.shape == (152,)
    assert same(v2, val[tail]) and same(g2, grad[:, tail])
    assert same(ps.eval_all(Xs[:, tail]), allv[tail])
    ps.close()
    gp.close()


@pytest.mark.parametrize("kernel", [0, 1])
def test_maximize_across_a_chunk_boundary_in_the_direct_form(m, ctx, kernel):
    """sls_path_maximize with n_local = 1 on 3 x 734 = 2202 starts: the one evaluation of every start runs in two chunks on the
    maximiser's layout of the candidates, and each draw's winner is the best of sls_path_eval's values at its starts, bit for bit
    (a point's bits depend on neither its column nor the rest of the call); draw 2's starts straddle column 2048."""
    F, N, D, nd, M, b, X, y, theta, Xs, rng = chunk_problem(kernel)
    S = 734
    starts = np.asfortranarray(np.concatenate([Xs, Xs[:, :nd * S - M]], axis=1))
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=77)
    val = ps.eval(starts, np.repeat(np.arange(nd), S), want_grad=False).reshape(nd, S)
    r = ps.maximize(starts, 1)
    ps.close()
    gp.close()
    assert same(r["value"], val.max(axis=1)) and np.array_equal(r["index"], val.argmax(axis=1))
    assert same(r["x"], starts[:, np.arange(nd) * S + val.argmax(axis=1)])


# ---- h: posterior samples ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D", sr.SIZES + gr.WIDE_SIZES)
def test_posterior_samples_are_mu_plus_cholesky_times_z(m, ctx, N, D, kernel):
    """The assertion of test_samples_are_mu_plus_cholesky_times_z at l = 1e-5 with mean and covariance from gram_ref (longdouble), the
    near-duplicate candidate pair among the points: its prior covariance is neither 0 nor a."""
    r = gr.reference(N, D, 1e-5, kernel, np.longdouble)
    S, seed, M, a = 37, 1234, gr.N_CAND, gr.A
    mu, cov = np.asarray(r["pred"]["mean"], dtype=np.float64), np.asarray(r["pred"]["cov"], dtype=np.float64)
    ev = np.linalg.eigvalsh(cov)
    assert ev[-1] / ev[0] <= 1e6, ev[-1] / ev[0]
    i, j = gr.CAND_PAIR
    assert 0.3 * a < cov[i, j] < 0.99 * a
    gp = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], kernel)
    Fs, jit = gp.sample_posterior(r["Xs"], S, seed)
    gp.close()
    assert Fs.shape == (M, S) and jit == 0.0
    Z = ctx.random_normal(seed, 0, M * S).reshape((S, M)).T
    want = mu[:, None] + np.linalg.cholesky(cov) @ Z
    e = np.abs(Fs - want)
    record(KIND, route="sample_posterior", N=N, D=D, ell="1e-05", kernel=kernel, errors=dict(samples=float(e.max()), pair=float(e[[i, j]].max())),
           tolerance=dict(samples=1e-9 * a))
    assert e.max() <= 1e-9 * a


# ---- i: the combiners on top of the guarded prediction -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0, 1])
def test_logei_and_mes_combiners_on_the_devices_own_predictions(m, ctx, kernel):
    """l = 1e-5, N = 300, D = 33: type 2 (LogEI) and sls_mes_eval on a handle beyond the guard, held to logei_ref / mes_ref on the
    device's own mu, sigma and their gradients with the bounds of the two combiner tests."""
    r = gr.reference(300, 33, 1e-5, kernel)
    Xs = r["Xs"]
    for mode in (0, 1):
        gp = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], kernel)
        gp.set_sigma_mode(mode)
        mu, sg, dmu, dsg = device_posterior(gp, Xs)
        gr.check(dict(mean=mu, dev=sg), gr.quantities(r), 33, 1.0)            # the predictions themselves are the guarded ones
        val, grad = gp.acq_eval(Xs, 2)
        wv, wg, _ = assert_logei_matches(val, grad, mu, sg, gp.summary()["mu_best"], dmu, dsg, ("logei", kernel, mode))
        ys = max_value_samples(np.random.default_rng(7), 7, r["y"], mu)
        with env_switch("SLS_WAVE_PATH", "0"), env_switch("SLS_TRI_PREDICT", "0"):
            mu, sg = gp.predict(Xs)
            dmu, dsg = gp.predict_grad(Xs)
            mv, mg = gp.mes_eval(ys, Xs)
        gp.close()
        rv, rg, info = mes_ref.alpha(mu, sg, ys, dmu, dsg)
        assert not info["bad"].any() and (info["gamma"] < 0).any()
        tol_v = 32 * EPS * (1.0 + (info["gamma"] ** 2).max(axis=0))
        tol_g = 1e-9 * np.abs(rg).max(axis=0) + 64 * EPS * (np.abs(info["A1"]) * np.abs(dmu).max(axis=0) +
                                                            np.abs(info["A2"]) * np.abs(dsg).max(axis=0)) / sg
        ev, eg = np.abs(mv - rv), np.abs(mg - rg).max(axis=0)
        live = tol_g > 0                                 # far from every training point the gradient and its bound are exactly 0
        record(KIND, route="combiners", kernel=kernel, sigma_mode=mode,
               errors=dict(logei_val_over_bound=float(wv), logei_grad_over_bound=float(np.nan_to_num(wg)),
                           mes_val_over_bound=float((ev / tol_v).max()), mes_grad_over_bound=float((eg[live] / tol_g[live]).max())))
        assert np.all(ev <= tol_v), (ev / tol_v).max()
        assert np.all(eg <= tol_g), (eg / tol_g).max()


@pytest.mark.parametrize("acq", [0, 1])
@pytest.mark.parametrize("kernel", [0, 1])
def test_pair_objective_with_both_handles_beyond_the_guard(m, ctx, kernel, acq):
    """sls_acq_eval_pair at l = 1e-5: the mean (and mu+) from a handle on N = 129 points, the deviation from one grown by three
    near-duplicates of its points (N = 132), composed from two gram_ref posteriors the way
    test_pair_objective_of_find_next_points composes two oracle regressors, with its tolerances."""
    import math
    N, D, h = 129, 6, 1.7
    r = gr.reference(N, D, 1e-5, kernel)
    rng = np.random.default_rng(9)
    extra = np.stack([r["X"][:, 60 + 5 * k] + gr._offset(rng, r["ell"], 0.7, D) for k in range(3)], axis=1)
    X2, y2 = np.asfortranarray(np.concatenate([r["X"], extra], axis=1)), np.concatenate([r["y"], [0.3, 0.1, -0.2]])
    f1, f2 = r["fit"], gr.fit(X2, y2, r["ell"], gr.A, gr.B, kernel)
    p1, p2 = r["pred"], gr.predict(f2, r["Xs"], want_grad=True)
    mu, dmu, sg, dsg = p1["mean"], p1["dmean"], p2["dev"], p2["ddev"]
    if acq == 0:
        mu_best = (f1["y"] - gr.B * f1["alpha"]).max()
        u = (mu - mu_best) / sg
        Phi = np.array([0.5 * math.erfc(-v / math.sqrt(2.0)) for v in u])
        phi = np.exp(-0.5 * u * u) / np.sqrt(2 * np.pi)
        vo, go = (mu - mu_best) * Phi + sg * phi, Phi * dmu + phi * dsg
    else:
        vo, go = mu + h * sg, dmu + h * dsg
    g1, g2 = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], kernel), m.GP(ctx, X2, y2, r["theta"], r["b"], kernel)
    v, g = g1.acq_eval_pair(g2, r["Xs"], acq, h)
    g1.close()
    g2.close()
    record(KIND, route="acq_eval_pair", kernel=kernel, acq=acq, errors=dict(val=err(v, vo), grad=err(g, go)),
           scale=dict(val=float(np.abs(vo).max()), grad=float(np.abs(go).max())))
    np.testing.assert_allclose(v, vo, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(g, go, rtol=1e-6, atol=1e-9 * np.abs(go).max())


# ---- j: the switch -----------------------------------------------------------------------------------------------------------------------
def every_entry_point(m, ctx, r):
    """Everything a - g evaluate, as a flat dict of arrays."""
    D, nd = r["D"], r["nd"]
    gp, ps = handles(m, ctx, r)
    out = {}
    out["val"], out["grad"] = ps.eval(r["Xs"], sr.draws_of_points(gr.N_CAND, nd))
    out["all"], out["at_data"] = ps.eval_all(r["Xs"]), ps.eval_all(r["X"])
    out["t"], out["t_arg"] = ps.max_over_points(r["X"])
    for q in sr.QS:
        sets = sr.sets_of(r["Xs"], q)
        out[f"qeubo{q}_val"], out[f"qeubo{q}_grad"], out[f"qeubo{q}_wins"] = ps.qeubo_eval(sets, q, want_wins=True)
        out[f"qnei{q}_val"], out[f"qnei{q}_grad"], out[f"qnei{q}_wins"] = ps.qnei_eval(sets, q, out["t"], want_wins=True)
    for anchored in (False, True):
        lines, anchor = sr.lines_of(r["Xs"], anchored)
        for base in (None, out["t"]):
            key = f"line{int(anchored)}{int(base is not None)}"
            out[key + "_val"], out[key + "_grad"], out[key + "_wins"] = ps.line_eval(lines, sr.LINE_Q, anchor=anchor, baseline=base, want_wins=True)
    pairs = sr.pairs_of(r["Xs"])
    for mode in (0, 1):
        gp.set_sigma_mode(mode)
        out[f"eubo{mode}_val"], out[f"eubo{mode}_grad"] = gp.eubo_eval(pairs)
    ps.close()
    gp.close()
    return out


@pytest.mark.parametrize("kernel", [0, 1])
def test_guard_switch_inside_the_guard_changes_no_bit(m, ctx, kernel):
    """l = 0.3: with SLS_GRAM_GUARD on and off every entry point of the tests above returns the same bits."""
    r = sr.reference(129, 6, 0.3, kernel)
    res = {}
    for v in (1, 0):
        with env_switch("SLS_GRAM_GUARD", v):
            res[v] = every_entry_point(m, ctx, r)
    for k in res[1]:
        assert np.array_equal(res[1][k], res[0][k]) if res[1][k].dtype.kind == "i" else same(res[1][k], res[0][k]), k


@pytest.mark.parametrize("kernel", [0, 1])
def test_guard_switch_just_beyond_the_guard_stays_within_the_expansions_bound(m, ctx, kernel):
    """l = 3e-3, D = 6: the two forms differ by the cancellation of the norm expansion, |dq| <= eps D / (2 l^2), i.e.
    dk = (a/2) eps D / (2 l^2) per Gram entry (|dk/dq| <= a/2 for both kernels).  Propagated without a reference of the results:
      a path value  sum_i k_i v_i : dk sum|v| + |k*|_2 |dv|_2, with dv = -K_y^-1 dK v: |dv|_2 <= N dk |v|_2 / lambda_min(K_y);
      its gradient: the weights c move by (25/6) a dq = (25/3) dk at most (Matern; dk for SE) and multiply |x_d - x_id| / l^2 <= 1.6 / l^2;
      t, qEUBO, qNEI and line values are maxima and means of such values (1-Lipschitz; qNEI sees t twice);
      EUBO: mu as the path value with alpha for v; s^2 = 2a - 2 k12 - d^T K_y^-1 d moves by
      dk (2 + 2 |d|_2 sqrt(2N) / lambda_min + |d|_2^2 N / lambda_min^2), s by that over 2 s, the value by (Phi + Phi') dmu + phi ds.
    K_y, v, alpha, k*, d and s are the reference's (tests/path_short_ref.py).  A wiring check: a wrong stride or pointer in either
    form is O(1)."""
    N, D = 129, 6
    r = sr.reference(N, D, 3e-3, kernel)
    assert sr.beyond_guard(r["ell"], D)
    res = {}
    for v in (1, 0):
        with env_switch("SLS_GRAM_GUARD", v):
            res[v] = every_entry_point(m, ctx, r)
    ref = r["ref64"]
    a, ell = gr.A, float(r["ell"].min())
    dk = 0.5 * a * EPS * D / (2 * ell * ell)
    lam = float(np.linalg.eigvalsh(ref.Ky)[0])
    kstar = float(np.sqrt((ref.kc(np.concatenate([r["Xs"], r["X"]], axis=1))[0] ** 2).sum(axis=1)).max())

    def value_bound(w):
        return dk * np.abs(w).sum(axis=0).max() + kstar * N * dk * np.sqrt((w * w).sum(axis=0)).max() / lam
    bv = value_bound(ref.v)
    bg = (25.0 / 3.0) * 1.6 / (ell * ell) * bv
    info = sr.eubo_reference(N, D, 3e-3, kernel)["e64"][2]
    pairs = sr.pairs_of(r["Xs"])
    dvec = ref.kc(pairs[:D])[0] - ref.kc(pairs[D:])[0]                           # M x N
    dn = float(np.sqrt((dvec ** 2).sum(axis=1)).max())
    ds2 = dk * (2 + 2 * dn * np.sqrt(2 * N) / lam + dn * dn * N / lam ** 2)
    be = 2 * value_bound(info["alpha"][:, None]) + 0.4 * ds2 / (2 * info["s"].min())
    bounds = dict(val=bv, all=bv, at_data=bv, t=bv, grad=bg)
    worst = {}
    for k in res[1]:
        if k.endswith("_wins") or k == "t_arg":
            continue
        bound = be if k.startswith("eubo") and k.endswith("_val") else bounds.get(k, 2 * bv if k.endswith("_val") else None)
        if bound is None:
            continue                                                            # set and pair gradients: through the winners, below
        worst[k] = (float(np.abs(res[1][k] - res[0][k]).max()), float(bound))
    record(KIND, route="guard_switch", N=N, D=D, ell="0.003", kernel=kernel, dk=dk, differences={k: v[0] for k, v in worst.items()},
           bounds={k: v[1] for k, v in worst.items()}, differ=bool(any(v[0] > 0 for v in worst.values())))
    assert any(v[0] > 0 for v in worst.values()), "the switch changed nothing: both runs took the same form"
    for k, (d, bound) in worst.items():
        assert d <= bound, (k, d, bound)
    # the winners where the reference's margin is clear, and on those sets the gradient (a wins-weighted mean of path gradients)
    for q in sr.QS:
        for name in ("qeubo", "qnei"):
            kept = r["kept"][f"{name}{q}"]
            assert np.array_equal(res[1][f"{name}{q}_wins"][:, kept], res[0][f"{name}{q}_wins"][:, kept])
            assert np.abs(res[1][f"{name}{q}_grad"][:, kept] - res[0][f"{name}{q}_grad"][:, kept]).max() <= bg
