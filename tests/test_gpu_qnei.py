"""qNEI, noisy expected improvement of q points on posterior draws, on the MI355X (sls_path_max_over_points / sls_qnei_eval /
sls_qnei_maximize): agreement with the numpy restatement (tests/qnei_ref.py) in incumbents, value, gradient and win counts, the
shapes of the incumbent reduction (one point, tile edges, several passes, duplicates, NaN), identities against qEUBO and the
every-draw evaluation, the bit-level contract (column, other sets, sets per pass, permuted and duplicated options, SLS_COMPACT=0),
the guard, central differences of the device values, the closed form of expected improvement on the same frequency set, the maximiser
against a grid, and argument errors."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import path_ref as ph
import posterior_ref as pr
import qnei_ref as nr
from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    """tests/test_gpu_path_sample.py's generator."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def tolerances(ref):
    """tests/test_gpu_qeubo.py's bounds: v = K_y^-1 r carries cond(K_y) eps |v| on both sides; k . v adds it to f.  An incumbent is one
    such value, a qNEI value a mean of differences of such values from a given baseline, a gradient block wins_i / S <= 1 times a mean
    of such gradients."""
    ev = np.linalg.eigvalsh(ref.Ky)
    cond = ev[-1] / ev[0]
    vs = np.abs(ref.v).max()
    tol_v = 1e-10 * ref.a + 4 * cond * EPS * vs * ref.a * np.sqrt(ref.N)
    tol_g = 1e-9 * ref.a + 4 * cond * EPS * vs * ref.a * np.sqrt(ref.N) / ref.ell.min()
    return tol_v, tol_g


def setup(m, ctx, kernel, N, D, F, nd, b=0.05):
    X, y, theta = problem(D, N, seed=N + D + F, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=1234 + D)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=1234 + D)
    return gp, ps, ref


# tests/test_gpu_qeubo.py's cases
CASES = [(ph.SE, 90, 2, 100, 3, 64), (ph.MATERN52, 90, 16, 1024, 4, 64), (ph.SE, 300, 96, 700, 2, 37), (ph.MATERN52, 700, 7, 300, 5, 130)]
# D > 128, as there: with 37 draws some of the 300 sets improve on no draw's incumbent and most do (measured on the restatement)
CASES += [(ph.SE, 90, 129, 100, 2, 37), (ph.MATERN52, 130, 257, 300, 4, 37)]


@pytest.mark.parametrize("kernel,N,D,F,q,nd", CASES)
def test_agrees_with_the_restatement(m, ctx, kernel, N, D, F, q, nd):
    gp, ps, ref = setup(m, ctx, kernel, N, D, F, nd)
    tol_v, tol_g = tolerances(ref)
    rt, rarg, inc_gap = nr.max_over_points(ref, ref.X)
    print(f"smallest incumbent gap {inc_gap.min():.3g} = {inc_gap.min() / tol_v:.3g} tol_v")
    assert inc_gap.min() >= 100 * tol_v                # a condition on the inputs: no incumbent can differ between the two sides
    t, arg = ps.max_over_points(ref.X)
    err_t = np.abs(t - rt).max()
    print(f"incumbent error {err_t:.3g} (tol {tol_v:.3g})")
    assert err_t <= tol_v and np.array_equal(arg, rarg)
    # the objective at the baseline the device formed, on both sides
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 300))
    rv, rg, rw, gap = nr.qnei(ref, sets, q, t)
    print(f"smallest gap {gap.min():.3g} = {gap.min() / tol_v:.3g} tol_v, {np.mean(rv > 0):.2f} of the sets improve")
    assert gap.min() >= 100 * tol_v                    # no winner, and no draw's having one, can differ between the two sides
    assert np.any(rv == 0.0) and np.any(rv > 0.0)      # both branches
    val, grad, wins = ps.qnei_eval(sets, q, t, want_wins=True)
    err_v, err_g = np.abs(val - rv).max(), np.abs(grad - rg).max()
    print(f"value error {err_v:.3g} (tol {tol_v:.3g}), gradient error {err_g:.3g} (tol {tol_g:.3g})")
    assert np.array_equal(wins, rw) and np.all(wins.sum(axis=0) <= nd)
    assert np.array_equal(val == 0.0, rv == 0.0) and np.all(val >= 0.0) and not np.any(np.signbit(val))
    assert np.all(grad[:, val == 0.0] == 0.0)
    assert err_v <= tol_v, (err_v, tol_v)
    assert err_g <= tol_g, (err_g, tol_g)
    # every output is optional and does not change the others
    assert np.array_equal(_bits(ps.qnei_eval(sets, q, t, want_grad=False)), _bits(val))
    ps.close()
    gp.close()


def test_max_over_points_shapes(m, ctx):
    kernel, N, D, F, _, nd = CASES[3]                  # 130 draws: two 128-column tiles of the values block
    gp, ps, ref = setup(m, ctx, kernel, N, D, F, nd)
    tol_v, _ = tolerances(ref)
    Xb = np.random.default_rng(4).uniform(0, 1, (D, 300))
    full = None
    for Mb in (1, 127, 128, 129, 300):
        P = Xb[:, :Mb]
        rt, rarg, gap = nr.max_over_points(ref, P)
        assert gap.min() >= 100 * tol_v
        t, arg = ps.max_over_points(P)
        assert np.abs(t - rt).max() <= tol_v and np.array_equal(arg, rarg), Mb
        assert np.abs(t - ps.eval_all(P).max(axis=0)).max() <= tol_v
        full = (t, arg)
    lib, dp = m.lib(), C.POINTER(C.c_double)
    t1, a1 = np.empty(nd), np.empty(nd, dtype=np.int32)                          # either output may be NULL
    Xf = np.asfortranarray(Xb)
    assert lib.sls_path_max_over_points(ps.h, Xf.ctypes.data_as(dp), 300, t1.ctypes.data_as(dp), None) == 0
    assert lib.sls_path_max_over_points(ps.h, Xf.ctypes.data_as(dp), 300, None, a1.ctypes.data_as(C.POINTER(C.c_int))) == 0
    assert np.array_equal(_bits(t1), _bits(full[0])) and np.array_equal(a1, full[1])
    # the point that is draw 0's maximiser, at column 3 (first pass of three) and again at column 290 (third pass)
    j0 = int(full[1][0])
    dup = Xb.copy()
    dup[:, 3] = dup[:, 290] = Xb[:, j0]
    ctx.set_candidate_chunk(128)
    try:
        tc, ac = ps.max_over_points(Xb)
        tdc, adc = ps.max_over_points(dup)
    finally:
        ctx.set_candidate_chunk(16384)
    assert np.array_equal(_bits(tc), _bits(full[0])) and np.array_equal(ac, full[1])
    td, ad = ps.max_over_points(dup)
    assert np.array_equal(_bits(td), _bits(tdc)) and np.array_equal(ad, adc)
    first = min(3, j0)
    assert ad[0] == first and _bits(td)[0] == _bits(full[0])[0]
    assert not np.any(ad == 290)                       # wherever that point is a draw's maximiser, the lower index is reported
    assert j0 <= 3 or not np.any(ad == j0)
    # the value does not depend on where the point stands
    perm = np.random.default_rng(5).permutation(300)
    tp, ap = ps.max_over_points(Xb[:, perm])
    assert np.array_equal(_bits(tp), _bits(full[0])) and np.array_equal(perm[ap], full[1])
    # a NaN coordinate in one point: every draw is poisoned, whichever pass the point is in
    for col in (2, 299):
        hit = Xb.copy()
        hit[1, col] = np.nan
        for chunk in (16384, 128):
            ctx.set_candidate_chunk(chunk)
            try:
                tn, an = ps.max_over_points(hit)
            finally:
                ctx.set_candidate_chunk(16384)
            assert np.all(np.isnan(tn)) and np.all(an == -1)
    ps.close()
    gp.close()


def test_identities_against_existing_entry_points(m, ctx):
    kernel, N, D, F, q, nd = CASES[0]
    gp, ps, ref = setup(m, ctx, kernel, N, D, F, nd)
    tol_v, _ = tolerances(ref)
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 300))
    ev, eg, ew = ps.qeubo_eval(sets, q, want_wins=True)
    # a baseline below every value: every draw has a winner, qEUBO's
    val, grad, wins = ps.qnei_eval(sets, q, np.full(nd, -1.0e3), want_wins=True)
    assert np.array_equal(wins, ew) and np.array_equal(_bits(grad), _bits(eg))
    assert np.abs(val - (ev + 1.0e3)).max() <= 8 * nd * EPS * 1.0e3
    # a baseline above every value: nobody improves
    val, grad, wins = ps.qnei_eval(sets, q, np.full(nd, 1.0e3), want_wins=True)
    assert np.all(val == 0.0) and not np.any(np.signbit(val)) and np.all(grad == 0.0) and np.all(wins == 0)
    # one point: the mean improvement
    t, _ = ps.max_over_points(ref.X)
    Xs = sets[:D]
    val, wins = ps.qnei_eval(Xs, 1, t, want_grad=False, want_wins=True)
    imp = np.maximum(ps.eval_all(Xs) - t[None, :], 0.0)
    assert np.abs(val - imp.mean(axis=1)).max() <= tol_v
    assert np.any(val > 0.0)
    ps.close()
    gp.close()


def test_bit_contract(m, ctx):
    D, N, F, q, nd, M = 3, 120, 300, 4, 20, 300
    X, y, theta = problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    t, _ = ps.max_over_points(X)
    rng = np.random.default_rng(3)
    sets = rng.uniform(0, 1, (q * D, M))
    val, grad, wins = ps.qnei_eval(sets, q, t, want_wins=True)
    assert np.any(val > 0.0) and np.any(wins.sum(axis=0) < nd)
    v2, g2, w2 = ps.qnei_eval(sets, q, t, want_wins=True)
    assert np.array_equal(_bits(val), _bits(v2)) and np.array_equal(_bits(grad), _bits(g2)) and np.array_equal(wins, w2)
    # a set alone, and among others at another column
    v1, g1, w1 = ps.qnei_eval(sets[:, 17:18], q, t, want_wins=True)
    assert _bits(v1)[0] == _bits(val)[17] and np.array_equal(_bits(g1[:, 0]), _bits(grad[:, 17])) and np.array_equal(w1[:, 0], wins[:, 17])
    perm = rng.permutation(M)
    vp, gp_, wp = ps.qnei_eval(sets[:, perm], q, t, want_wins=True)
    assert np.array_equal(_bits(vp), _bits(val[perm])) and np.array_equal(_bits(gp_), _bits(grad[:, perm])) and np.array_equal(wp, wins[:, perm])
    # 256 POINTS per pass = 64 sets, rounded to the 128-set minimum: three passes instead of one
    ctx.set_candidate_chunk(256)
    try:
        vc, gc, wc = ps.qnei_eval(sets, q, t, want_wins=True)
    finally:
        ctx.set_candidate_chunk(16384)
    assert np.array_equal(_bits(vc), _bits(val)) and np.array_equal(_bits(gc), _bits(grad)) and np.array_equal(wc, wins)
    # options permuted: the value's bits stay, gradient blocks and win counts move with their options
    order = np.array([2, 0, 3, 1])
    rows = np.concatenate([np.arange(i * D, (i + 1) * D) for i in order])
    vo, go, wo = ps.qnei_eval(sets[rows], q, t, want_wins=True)
    assert np.array_equal(_bits(vo), _bits(val)) and np.array_equal(_bits(go), _bits(grad[rows])) and np.array_equal(wo, wins[order])
    # x_1 = x_0: the duplicate never wins, has an exactly zero gradient, and the value is the set's without it
    dup = sets.copy()
    dup[D:2 * D] = dup[:D]
    vd, gd, wd = ps.qnei_eval(dup, q, t, want_wins=True)
    rest = np.concatenate([np.arange(0, D), np.arange(2 * D, q * D)])
    v3, g3, w3 = ps.qnei_eval(dup[rest], q - 1, t, want_wins=True)
    assert np.all(wd[1] == 0) and np.all(gd[D:2 * D] == 0.0)
    assert np.array_equal(_bits(vd), _bits(v3)) and np.array_equal(_bits(gd[rest]), _bits(g3)) and np.array_equal(wd[[0, 2, 3]], w3)
    ps.close()
    gp.close()


def test_guard_on_the_device(m, ctx):
    """A NaN coordinate in one option: that set gets the value 0 and the zero gradient (the select kernel's flag, the finish kernel's
    scan), with or without the gradient asked for; its neighbours keep their bits.  A baseline entry that is not finite is refused."""
    D, N, F, q, nd = 3, 120, 300, 3, 20
    X, y, theta = problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    t, _ = ps.max_over_points(X)
    t = t - 0.2                                                     # most sets improve: a guarded 0 is not the value anyway
    for M, bad in ((3, [1]), (300, [0, 130, 299])):
        sets = np.random.default_rng(5).uniform(0, 1, (q * D, M))
        val, grad, wins = ps.qnei_eval(sets, q, t, want_wins=True)
        assert np.all(val[bad] > 0.0)
        hit = sets.copy()
        for k, n in enumerate(bad):
            hit[(k % q) * D + 1, n] = np.nan                       # another option each time
        v, g, w = ps.qnei_eval(hit, q, t, want_wins=True)
        good = np.setdiff1d(np.arange(M), bad)
        assert np.all(v[bad] == 0.0) and np.all(g[:, bad] == 0.0)
        assert np.array_equal(_bits(v[good]), _bits(val[good])) and np.array_equal(_bits(g[:, good]), _bits(grad[:, good]))
        assert np.array_equal(w[:, good], wins[:, good])
        assert np.array_equal(_bits(ps.qnei_eval(hit, q, t, want_grad=False)), _bits(v))
    sets = np.random.default_rng(5).uniform(0, 1, (q * D, 3))
    want = ps.qnei_eval(sets, q, t, want_grad=False)
    for poison in (np.nan, np.inf, -np.inf):
        tb = t.copy()
        tb[nd - 1] = poison
        with pytest.raises(m.SlsError, match="not finite"):
            ps.qnei_eval(sets, q, tb)
        with pytest.raises(m.SlsError, match="not finite"):
            ps.qnei_maximize(sets, q, 3, tb)
    assert np.array_equal(_bits(ps.qnei_eval(sets, q, t, want_grad=False)), _bits(want))     # the context stays usable
    ps.close()
    gp.close()


COMPACT_SCRIPT = r"""
import sys, importlib, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
m = importlib.import_module('sequential-line-search_amd')
rng = np.random.default_rng(12)
D, N, q = 3, 200, 3
X = rng.uniform(0, 1, (D, N)); y = np.sin(X.sum(0)); theta = np.concatenate([[0.6], np.full(D, 0.4)])
ctx = m.Context(0)
gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
ps = m.PathSamples(gp, 24, 300, seed=8)
t, arg = ps.max_over_points(X)
r = ps.qnei_maximize(rng.uniform(0, 1, (q * D, 300)), q, 25, t, opts=m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6))
st = gp.last_stats()
np.savez(sys.argv[2], x=r['x'], value=r['value'], index=r['index'], x_stars=r['x_stars'], y_stars=r['y_stars'], t=t, arg=arg,
         issued=st['evals_issued'], cap=st['evals_cap'])
ps.close(); gp.close(); ctx.close()
"""


def test_compaction_off_gives_the_same_bits(tmp_path):
    script = tmp_path / "compact.py"
    script.write_text(COMPACT_SCRIPT)
    out = {}
    for flag in ("1", "0"):
        env = dict(os.environ, SLS_COMPACT=flag)
        r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / f"c{flag}.npz")], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        out[flag] = np.load(tmp_path / f"c{flag}.npz")
    for k in ("x", "value", "x_stars", "y_stars", "t"):
        assert np.array_equal(_bits(out["1"][k]), _bits(out["0"][k])), k
    assert out["1"]["index"] == out["0"]["index"] and np.array_equal(out["1"]["arg"], out["0"]["arg"])
    assert out["1"]["value"] > 0.0
    assert out["1"]["issued"] < out["1"]["cap"]           # starts did leave the batch: the two schedules differed


def test_central_differences_of_device_values(m, ctx):
    D, N, F, q, nd, M = 3, 50, 150, 3, 5, 64
    X, y, theta = problem(D, N, seed=24)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, 0.02, ph.SE)
    ps = m.PathSamples(gp, nd, F, seed=3)
    ref = ph.PathRef(X, y, theta, 0.02, ph.SE, nd, F, seed=3)
    t, _ = ps.max_over_points(X)
    sets = np.random.default_rng(7).uniform(0.05, 0.95, (q * D, M))
    gap = nr.qnei(ref, sets, q, t)[3]
    ok = gap >= 1e-4 * a                               # no winner, and no draw's having one, changes inside the stencil
    assert ok.sum() >= 8, ok.sum()
    val, grad = ps.qnei_eval(sets, q, t)
    assert np.any(val[ok] > 0.0)
    h = 1e-6
    for r in range(q * D):
        E = np.zeros((q * D, M))
        E[r] = h
        fd = (ps.qnei_eval(sets + E, q, t, want_grad=False) - ps.qnei_eval(sets - E, q, t, want_grad=False)) / (2 * h)
        assert np.abs(fd - grad[r])[ok].max() <= 1e-6 * (a + np.abs(grad[:, ok]).max())
    ps.close()
    gp.close()


def test_one_point_against_the_fixed_basis_closed_form(m, ctx):
    """With a constant baseline c the one-point estimator is Monte-Carlo expected improvement: its expectation is s h(u), h(u) = phi(u)
    + u Phi(u), u = (mu - c) / s, with the exact posterior mean and the variance THIS frequency set gives."""
    D, N, F, S, b = 3, 200, 1024, 4096, 0.02
    X, y, theta = problem(D, N, seed=9, ell=0.35)
    gp = m.GP(ctx, X, y, theta, b, ph.SE)
    ps = m.PathSamples(gp, S, F, seed=F)
    ref = ph.PathRef(X, y, theta, b, ph.SE, S, F, seed=F)
    tol_v, _ = tolerances(ref)
    P = np.random.default_rng(2).uniform(0, 1, (D, 64))
    KsX = pr.ard_kernel(P, X, theta, ph.SE)                                     # 64 x N
    mu = KsX @ np.linalg.solve(ref.Ky, y)
    Ps, PX = ph.features(ref.om, ref.a, P, ref.ell), ph.features(ref.om, ref.a, X, ref.ell)
    s = np.sqrt(np.diag(ph.pathwise_cov(Ps.T @ Ps, Ps.T @ PX, PX.T @ PX, KsX.T, ref.Ky, b)))
    c = float(np.median(mu))
    u = (mu - c) / s
    exact = s * (np.exp(-0.5 * u * u) / math.sqrt(2 * math.pi) + u * 0.5 * np.array([math.erfc(-x / math.sqrt(2)) for x in u]))
    val = ps.qnei_eval(P, 1, np.full(S, c), want_grad=False)
    se = np.maximum(ps.eval_all(P) - c, 0.0).std(axis=1, ddof=1) / np.sqrt(S)
    ok = np.abs(u) <= 2
    assert ok.sum() >= 32, ok.sum()
    dev = np.abs(val - exact)
    print(f"{ok.sum()} of 64 points qualify, largest deviation {(dev[ok] / se[ok]).max():.2f} standard errors")
    assert np.all(dev[ok] <= 5 * se[ok] + tol_v), (dev[ok] / se[ok]).max()
    ps.close()
    gp.close()


def test_maximiser_against_the_grid(m, ctx):
    D, N, q, nd, F, S, n_local = 1, 30, 3, 32, 256, 1024, 60
    X, y, theta = problem(D, N, seed=41, ell=0.3)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.SE)
    ps = m.PathSamples(gp, nd, F, seed=17)
    t, _ = ps.max_over_points(X)
    starts = np.random.default_rng(8).uniform(0, 1, (q * D, S))
    at_start = ps.qnei_eval(starts, q, t, want_grad=False)
    r = ps.qnei_maximize(starts, q, n_local, t, offset=1000)
    st = gp.last_stats()
    # the 101^3 grid of sets from ONE evaluation of the grid points under every draw
    g1 = np.linspace(0, 1, 101)
    V = ps.eval_all(g1[None, :])                                                # 101 x nd
    two = np.maximum(V[:, None, :], V[None, :, :])                              # 101 x 101 x nd
    grid_best = max(np.maximum(np.maximum(two, V[k][None, None, :]) - t[None, None, :], 0.0).mean(axis=2).max() for k in range(101))
    # a set moves by at most half a step per coordinate to its nearest grid set; |d qNEI / d x_i| <= max_s |f_s'(x_i)|
    _, gd = ps.eval(np.repeat(g1[None, :], nd, axis=1), np.tile(np.arange(nd), 101))
    slack = q * D * np.abs(gd).max() * 0.5 * (g1[1] - g1[0])
    print(f"winner {r['value']:.12g} at {r['x']}, grid maximum {grid_best:.12g}, resolution slack {slack:.3g}, stats {st}")
    assert r["value"] >= grid_best - slack
    x = r["x"]
    assert x.shape == (q * D,) and np.all((x >= 0) & (x <= 1))
    assert abs(ps.qnei_eval(x[:, None], q, t, want_grad=False)[0] - r["value"]) <= 1e-12
    assert r["index"] - 1000 == int(np.argmax(r["y_stars"])) and r["value"] == r["y_stars"].max()
    assert np.array_equal(r["x_stars"][:, r["index"] - 1000], x)
    assert r["x_stars"].shape == (q * D, S) and np.all((r["x_stars"] >= 0) & (r["x_stars"] <= 1))
    assert np.abs(ps.qnei_eval(r["x_stars"], q, t, want_grad=False) - r["y_stars"]).max() <= 1e-12
    assert np.all(r["y_stars"] >= at_start)
    assert 0 < st["evals_issued"] <= S * n_local and st["evals_cap"] == S * n_local and 1 <= st["rounds"] <= n_local
    r0 = ps.qnei_maximize(starts, q, n_local, t, want_all=False)
    assert r0["index"] == r["index"] - 1000 and r0["value"] == r["value"] and np.array_equal(r0["x"], x)
    ps.close()
    gp.close()


def test_argument_errors_leave_the_context_usable(m, ctx):
    D, N, q, nd = 3, 40, 2, 4
    X, y, theta = problem(D, N, seed=6)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.SE)
    ps = m.PathSamples(gp, nd, 64, seed=1)
    lib, dp, ip = m.lib(), C.POINTER(C.c_double), C.POINTER(C.c_int)
    P = np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (17 * D, 3)))
    Xf = np.asfortranarray(X)
    base, tt, aa = np.zeros(nd), np.empty(nd), np.empty(nd, dtype=np.int32)
    val, x, v, idx = np.empty(3), np.empty(17 * D), C.c_double(), C.c_long()
    p = lambda a: a.ctypes.data_as(dp)

    def ev(h, qq, bp, Pp, M):
        return lib.sls_qnei_eval(h, qq, bp, Pp, M, p(val), None, None)

    def mx(h, qq, bp, sp, S=3, n_local=5):
        return lib.sls_qnei_maximize(h, qq, bp, sp, S, n_local, None, C.c_long(0), p(x), C.byref(v), C.byref(idx), None, None)

    def mo(h, Xp, Mb):
        return lib.sls_path_max_over_points(h, Xp, Mb, p(tt), aa.ctypes.data_as(ip))

    for qq in (0, 17, -1):
        assert ev(ps.h, qq, p(base), p(P), 3) == -1 and mx(ps.h, qq, p(base), p(P)) == -1, qq
    assert ev(None, q, p(base), p(P), 3) == -1 and ev(ps.h, q, p(base), None, 3) == -1 and ev(ps.h, q, p(base), p(P), -1) == -1
    assert ev(ps.h, q, None, p(P), 3) == -1 and mx(ps.h, q, None, p(P)) == -1
    assert mx(None, q, p(base), p(P)) == -1 and mx(ps.h, q, p(base), None) == -1
    assert mx(ps.h, q, p(base), p(P), S=0) == -1 and mx(ps.h, q, p(base), p(P), n_local=0) == -1
    assert mo(None, p(Xf), N) == -1 and mo(ps.h, None, N) == -1 and mo(ps.h, p(Xf), 0) == -1 and mo(ps.h, p(Xf), -2) == -1
    assert mo(ps.h, p(Xf), N) == 0 and np.all(np.isfinite(tt)) and np.all((aa >= 0) & (aa < N))
    assert ev(ps.h, q, p(base), p(P), 0) == 0                       # M = 0: nothing to do
    assert ev(ps.h, q, p(base), p(P), 3) == 0 and np.all(np.isfinite(val))
    assert lib.sls_qnei_eval(ps.h, q, p(base), p(P), 3, None, None, None) == 0     # every output may be NULL
    assert mx(ps.h, q, p(base), p(P)) == 0 and np.isfinite(v.value)
    gp.append_point(np.full(D, 0.3), 0.1)                           # the path is stale now
    assert ev(ps.h, q, p(base), p(P), 3) == -1 and "refitted or grown" in lib.sls_last_error().decode()
    assert mx(ps.h, q, p(base), p(P)) == -1 and "refitted or grown" in lib.sls_last_error().decode()
    assert mo(ps.h, p(Xf), N) == -1 and "refitted or grown" in lib.sls_last_error().decode()
    ps.close()
    ps2 = m.PathSamples(gp, nd, 64, seed=1)                         # the context and the handle still work
    v2 = ps2.qnei_eval(P[:q * D], q, base, want_grad=False)
    assert np.all(np.isfinite(v2))
    ps2.close()
    gp.close()
