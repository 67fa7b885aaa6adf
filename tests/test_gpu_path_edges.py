"""Pathwise posterior draws (sls_path_*) at the shapes where the host loops split the work, against the numpy restatement
(tests/path_ref.py): a second evaluation chunk (the s0 > 0 offsets of path_eval_device, a ragged last chunk), a second row block of
sls_path_create, draw indices beyond the first 128-column tile of W / V up to the limit of 4096 draws, the n_freq limit, the
maximiser's segmentation at draw boundaries inside a tile (index, first-wins ties, the clamp of the starts, history 1 and 8) and the
shared lock-step driver when all the starts of one draw finish in the first round.

Every case restates the host rule it means to cross (path_ref.eval_chunk / create_rows) and asserts that its shape crosses it."""
import numpy as np
import pytest

import path_ref as ph
from util import sls

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def problem(D, N, seed, ell=0.5, a=0.5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


def tolerances(ref):
    """(tol_v, tol_g, cond) of test_gpu_path_sample.test_eval_agrees_with_the_restatement:
    v = K_y^-1 r carries cond(K_y) eps |v| on both sides; k . v adds it to f (a sqrt(N) bounds |k|), the gradient divides by l."""
    ev = np.linalg.eigvalsh(ref.Ky)
    cond = ev[-1] / ev[0]
    a, N = ref.a, ref.N
    vs = np.abs(ref.v).max()
    tol_v = 1e-10 * a + 4 * cond * EPS * vs * a * np.sqrt(N)
    tol_g = 1e-9 * a + 4 * cond * EPS * vs * a * np.sqrt(N) / ref.ell.min()
    return tol_v, tol_g, cond


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _report(name, **ratios):
    print("RATIO", name, " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


@pytest.mark.parametrize("kernel", [ph.SE, ph.MATERN52])
def test_eval_across_a_chunk_boundary(m, ctx, kernel):
    """M = 2200 candidates at F = 16384 (the n_freq limit): chunks of 2048, so columns 2048 .. 2199 are a second, ragged chunk
    (Cp = 256, which also moves G = PG + Cp Np)."""
    F, N, D, nd, M, b = 16384, 90, 3, 3, 2200, 0.05
    chunk = ph.eval_chunk(ph.round_up(N, 128), ph.round_up(F, 128))
    assert chunk == 2048 and chunk < M < 2 * chunk and (M - chunk) % 128 != 0
    X, y, theta = problem(D, N, seed=400 + kernel)
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=77)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=77)
    tol_v, tol_g, cond = tolerances(ref)
    rng = np.random.default_rng(11)
    Xs = rng.uniform(0, 1, (D, M))
    dr = rng.integers(0, nd, M)
    dr[chunk - 2:chunk + 3] = [0, 1, 2, 1, 0]        # the draws differ on both sides of the boundary
    val, grad = ps.eval(Xs, dr)
    allv = ps.eval_all(Xs)
    # against the restatement on a slice that straddles column 2048
    sl = slice(1900, 2200)
    assert sl.start < chunk < sl.stop
    rv, rg = ref.eval(Xs[:, sl], dr[sl])
    rall = ref.eval_all(Xs[:, sl])
    err_v, err_g, err_all = np.abs(val[sl] - rv).max(), np.abs(grad[:, sl] - rg).max(), np.abs(allv[sl] - rall).max()
    _report(f"chunk_boundary[{kernel}]", v=err_v / tol_v, g=err_g / tol_g, all=err_all / tol_v)
    assert err_v <= tol_v, (err_v, tol_v, cond)
    assert err_g <= tol_g, (err_g, tol_g, cond)
    assert err_all <= tol_v, (err_all, tol_v, cond)
    assert np.abs(allv[np.arange(M), dr] - val).max() <= tol_v
    # column independence (sls_hip.h): the points of the second chunk, evaluated in a call of their own, have the same bits
    tail = slice(chunk, M)
    v2, g2 = ps.eval(Xs[:, tail], dr[tail])
    assert v2.shape == (152,)
    assert np.array_equal(_bits(v2), _bits(val[tail])) and np.array_equal(_bits(g2), _bits(grad[:, tail]))
    assert np.array_equal(_bits(ps.eval_all(Xs[:, tail])), _bits(allv[tail]))
    ps.close()
    gp.close()


def test_create_across_a_row_block(m, ctx):
    """N = 2200 at F = 16384: sls_path_create builds the prior at the training points in blocks of 2048 rows, so rows 2048 .. 2303
    of V come from a second block (g.XT + i0, V + i0)."""
    F, N, D, nd, M, b, kernel = 16384, 2200, 3, 3, 300, 0.01, ph.SE
    Np, Fp = ph.round_up(N, 128), ph.round_up(F, 128)
    rows = ph.create_rows(Np, Fp)
    assert rows == 2048 and Np == 2304 and Np > rows and N > rows + 128
    X, y, theta = problem(D, N, seed=2200)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=31)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=31)
    tol_v, tol_g, cond = tolerances(ref)
    rng = np.random.default_rng(12)
    Xs = rng.uniform(0, 1, (D, M))
    dr = rng.integers(0, nd, M)
    val, grad = ps.eval(Xs, dr)
    allv = ps.eval_all(Xs)
    rv, rg = ref.eval(Xs, dr)
    rall = ref.eval_all(Xs)
    err_v, err_g, err_all = np.abs(val - rv).max(), np.abs(grad - rg).max(), np.abs(allv - rall).max()
    # the identity at the data for training rows behind the first block, f_s(x_i) = y_i - sqrt(b) eps_si - b v_si.  Bound of
    # test_identity_at_the_data, 1e-9 (a + |y|max), plus the cond term of tol_v: the device's v_s carries cond(K_y) eps |v| and
    # k(x_i, X) . v_s brings it into f_s(x_i) times |k| <= a sqrt(N); the restatement's b v_s carries b times the same error, which
    # is smaller (b < a sqrt(N))
    tr = np.arange(2040, 2200)
    assert tr[0] < rows < tr[-1]
    f = ps.eval_all(X[:, tr])
    tol_id = 1e-9 * (a + np.abs(y).max()) + 4 * cond * EPS * np.abs(ref.v).max() * a * np.sqrt(N)
    err_id = np.abs(f - ref.data_identity(tr)).max()
    _report("row_block", v=err_v / tol_v, g=err_g / tol_g, all=err_all / tol_v, identity=err_id / tol_id, cond=cond)
    assert err_v <= tol_v, (err_v, tol_v, cond)
    assert err_g <= tol_g, (err_g, tol_g, cond)
    assert err_all <= tol_v, (err_all, tol_v, cond)
    assert err_id <= tol_id, (err_id, tol_id, cond)
    ps.close()
    gp.close()


@pytest.mark.parametrize("kernel", [ph.SE, ph.MATERN52])
def test_draws_beyond_the_first_tile(m, ctx, kernel):
    """300 draws: W and V have Rp = 384 columns, the every-draw GEMM writes three column tiles, the gathered form reads columns
    beyond 128."""
    nd, F, N, D, M, b = 300, 256, 150, 4, 200, 0.05
    assert ph.round_up(nd, 128) // 128 == 3
    X, y, theta = problem(D, N, seed=300 + kernel)
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=19)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=19)
    tol_v, tol_g, cond = tolerances(ref)
    rng = np.random.default_rng(13)
    Xs = rng.uniform(0, 1, (D, M))
    dr = rng.integers(0, nd, M)
    forced = [0, 127, 128, 255, 256, 299]
    dr[rng.choice(M, len(forced), replace=False)] = forced
    assert set(forced) <= set(dr.tolist()) and dr.max() == nd - 1
    val, grad = ps.eval(Xs, dr)
    allv = ps.eval_all(Xs)
    rv, rg = ref.eval(Xs, dr)
    rall = ref.eval_all(Xs)
    assert allv.shape == (M, nd)
    err_v, err_g = np.abs(val - rv).max(), np.abs(grad - rg).max()
    err_cols = np.abs(allv - rall).max(axis=0)             # per draw: a permuted or mixed-up draw shows in its own column
    _report(f"draw_tiles[{kernel}]", v=err_v / tol_v, g=err_g / tol_g, all=err_cols.max() / tol_v)
    assert err_v <= tol_v, (err_v, tol_v, cond)
    assert err_g <= tol_g, (err_g, tol_g, cond)
    assert np.all(err_cols <= tol_v), (np.flatnonzero(err_cols > tol_v)[:10], err_cols.max(), tol_v, cond)
    assert np.abs(allv[np.arange(M), dr] - val).max() <= tol_v
    ps.close()
    gp.close()


@pytest.mark.parametrize("kernel", [ph.SE, ph.MATERN52])
def test_draw_limit(m, ctx, kernel):
    """n_draws = 4096 (the limit): every one of the 32 column tiles of the every-draw form, and the gathered form at the first and
    the last draw, in the middle and just behind a tile edge."""
    nd, F, N, D, M, b = 4096, 128, 40, 2, 130, 0.05
    X, y, theta = problem(D, N, seed=4096 + kernel)
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=23)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=23)
    tol_v, tol_g, cond = tolerances(ref)
    rng = np.random.default_rng(14)
    Xs = rng.uniform(0, 1, (D, M))
    allv = ps.eval_all(Xs)
    assert allv.shape == (M, nd)
    err_cols = np.abs(allv - ref.eval_all(Xs)).max(axis=0)
    dr = np.array([0, 4095, 2048, 129])[np.arange(M) % 4]
    val, grad = ps.eval(Xs, dr)
    rv, rg = ref.eval(Xs, dr)
    err_v, err_g = np.abs(val - rv).max(), np.abs(grad - rg).max()
    _report(f"draw_limit[{kernel}]", v=err_v / tol_v, g=err_g / tol_g, all=err_cols.max() / tol_v)
    assert np.all(err_cols <= tol_v), (np.flatnonzero(err_cols > tol_v)[:10], err_cols.max(), tol_v, cond)
    assert err_v <= tol_v, (err_v, tol_v, cond)
    assert err_g <= tol_g, (err_g, tol_g, cond)
    assert np.abs(allv[np.arange(M), dr] - val).max() <= tol_v
    ps.close()
    gp.close()


# ---- the maximiser: D = 3, N = 60, F = 300, 5 draws of S = 37 starts: the draws meet at columns 37, 74, 111, 148, inside tiles ----

SEG = dict(D=3, N=60, F=300, nd=5, S=37, b=0.01)


def _seg_setup(m, ctx, kernel):
    D, N, F, nd, S, b = (SEG[k] for k in ("D", "N", "F", "nd", "S", "b"))
    assert all((s * S) % 128 != 0 for s in range(1, nd)) and nd * S > 128
    X, y, theta = problem(D, N, seed=60 + kernel, ell=0.3)
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=7)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=7)
    rng = np.random.default_rng(15)
    # starts over [-0.25, 1.25]^D; every start of draw 0 has its first coordinate outside [0, 1], so the winner of draw 0 is a
    # clamped start whichever it is
    starts = rng.uniform(-0.25, 1.25, (D, nd * S))
    starts[0, :S] = np.where(rng.uniform(size=S) < 0.5, rng.uniform(-0.3, -0.01, S), rng.uniform(1.01, 1.3, S))
    return gp, ps, ref, theta, starts


@pytest.mark.parametrize("kernel", [ph.SE, ph.MATERN52])
def test_one_evaluation_picks_the_first_best_clamped_start(m, ctx, kernel):
    D, nd, S = SEG["D"], SEG["nd"], SEG["S"]
    gp, ps, ref, theta, starts = _seg_setup(m, ctx, kernel)
    draw_of = np.repeat(np.arange(nd), S)

    def check(starts):
        clipped = np.clip(starts, 0.0, 1.0)
        v0 = ps.eval(clipped, draw_of, want_grad=False).reshape(nd, S)
        r = ps.maximize(starts, 1)
        assert np.array_equal(r["index"], np.argmax(v0, axis=1)), (r["index"], np.argmax(v0, axis=1))
        win = np.arange(nd) * S + r["index"]
        assert np.array_equal(_bits(r["x"]), _bits(clipped[:, win]))
        assert np.array_equal(_bits(r["value"]), _bits(v0[np.arange(nd), r["index"]]))
        assert np.array_equal(_bits(r["value"]), _bits(ps.eval(r["x"], np.arange(nd), want_grad=False)))
        return r, v0, win

    r, v0, win = check(starts)
    outside = np.any((starts < 0.0) | (starts > 1.0), axis=0)
    assert outside[:S].all() and outside[win[0]] and not outside.all()
    assert np.any(np.clip(starts, 0, 1)[:, win[0]] != starts[:, win[0]])
    # a tie: the best start of a draw once more at the draw's last position; the earlier one is returned
    t = next(s for s in range(1, nd) if r["index"][s] < S - 1)
    tied = starts.copy()
    tied[:, t * S + S - 1] = starts[:, win[t]]
    r2, v2, _ = check(tied)
    assert _bits(v2[t, S - 1]) == _bits(v2[t, r["index"][t]])        # a tie in the bits, not just in the value
    assert r2["index"][t] == r["index"][t] and np.array_equal(r2["index"], r["index"])
    # and at the draw's FIRST position: now that one wins
    if r["index"][t] > 0:
        tied0 = starts.copy()
        tied0[:, t * S] = starts[:, win[t]]
        r3, _, _ = check(tied0)
        assert r3["index"][t] == 0
    ps.close()
    gp.close()


@pytest.mark.parametrize("history", [None, 1, 8])
@pytest.mark.parametrize("kernel", [ph.SE, ph.MATERN52])
def test_maximizer_segments_inside_tiles(m, ctx, kernel, history):
    """40 rounds; history 1 and 8 are the two ends of the workspace sizing rule (LbfgsWs: S Dh m doubles per history block)."""
    D, nd, S = SEG["D"], SEG["nd"], SEG["S"]
    gp, ps, ref, theta, starts = _seg_setup(m, ctx, kernel)
    a = theta[0]
    tol_v, _, cond = tolerances(ref)
    opts = None if history is None else m.LbfgsOpts(history=history)
    r = ps.maximize(starts, 40, opts=opts)
    x = r["x"]
    assert np.all((x >= 0) & (x <= 1))
    assert np.all((r["index"] >= 0) & (r["index"] < S))
    v, gr = ps.eval(x, np.arange(nd))
    assert np.array_equal(_bits(v), _bits(r["value"]))
    v0 = ps.eval(np.clip(starts, 0.0, 1.0), np.repeat(np.arange(nd), S), want_grad=False).reshape(nd, S)
    assert np.all(r["value"] >= v0.max(axis=1)), (r["value"], v0.max(axis=1))
    # projected gradient (maximisation in [0,1]^D): components pushing out of the box at a bound do not count
    pg = np.where((x <= 0) & (gr < 0), 0.0, np.where((x >= 1) & (gr > 0), 0.0, gr))
    scale = a / theta[1:].min()
    rv, _ = ref.eval(x, np.arange(nd))
    err = np.abs(rv - r["value"]).max()
    _report(f"segments[{kernel},{history}]", pg=np.abs(pg).max() / (1e-4 * scale), v=err / tol_v)
    assert np.abs(pg).max() <= 1e-4 * scale, (np.abs(pg).max(), scale)
    assert err <= tol_v, (err, tol_v, cond)
    ps.close()
    gp.close()


def test_a_draw_whose_starts_all_finish_in_the_first_round(m, ctx):
    """All the starts of draw 1 sit at its optimum: with a gradient tolerance they leave the active set after the first round, and
    the 128 columns 256 .. 383, all theirs, empty at once while the other draws go on.  The finished draw keeps its first
    evaluation; the others end with the bits of a run in which draw 1 has ordinary starts (independence), and draw 0 with the
    bits of a one-draw object that never saw the other starts (prefix)."""
    D, N, F, nd, S, b, kernel, n_local = 3, 60, 300, 4, 200, 0.01, ph.MATERN52, 25
    fin = 1
    assert fin * S <= 256 and 384 <= (fin + 1) * S       # a whole 128-column tile inside the finished draw's range
    X, y, theta = problem(D, N, seed=88, ell=0.3)
    a = theta[0]
    scale = a / theta[1:].min()
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=3)
    ps1 = m.PathSamples(gp, 1, F, seed=3)
    rng = np.random.default_rng(16)
    starts = rng.uniform(0, 1, (D, nd * S))
    opts = m.LbfgsOpts(gtol=1e-3 * scale)
    xopt = ps.maximize(starts, 80)["x"][:, fin]
    v_f, g_f = ps.eval(xopt[:, None], [fin])
    pg = np.where((xopt <= 0) & (g_f[:, 0] < 0), 0.0, np.where((xopt >= 1) & (g_f[:, 0] > 0), 0.0, g_f[:, 0]))
    assert np.abs(pg).max() <= 1e-4 * scale < opts.gtol    # stationary for the driver: it stops at pgmax <= gtol
    base = ps.maximize(starts, n_local, opts=opts)
    parked = starts.copy()
    parked[:, fin * S:(fin + 1) * S] = xopt[:, None]
    r = ps.maximize(parked, n_local, opts=opts)
    assert _bits(r["value"][fin]) == _bits(v_f[0]) and np.array_equal(_bits(r["x"][:, fin]), _bits(xopt)) and r["index"][fin] == 0
    others = [s for s in range(nd) if s != fin]
    # the other draws did go on: they moved away from their best start
    v0 = ps.eval(starts, np.repeat(np.arange(nd), S), want_grad=False).reshape(nd, S)
    assert np.all(r["value"][others] > v0.max(axis=1)[others])
    assert np.array_equal(_bits(r["x"][:, others]), _bits(base["x"][:, others]))
    assert np.array_equal(_bits(r["value"][others]), _bits(base["value"][others]))
    assert np.array_equal(r["index"][others], base["index"][others])
    r1 = ps1.maximize(starts[:, :S], n_local, opts=opts)
    assert np.array_equal(_bits(r1["x"][:, 0]), _bits(r["x"][:, 0])) and _bits(r1["value"][0]) == _bits(r["value"][0])
    assert r1["index"][0] == r["index"][0]
    for p in (ps, ps1):
        p.close()
    gp.close()
