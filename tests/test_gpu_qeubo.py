"""qEUBO, the expected utility of the best of q options on posterior draws, on the MI355X (sls_qeubo_eval / sls_qeubo_maximize):
agreement with the numpy restatement (tests/qeubo_ref.py) in value, gradient and win counts, consistency with sls_path_eval's two
forms, the bit-level contract (column, other sets, sets per pass, permuted and duplicated options, SLS_COMPACT=0), central
differences of the device values, the closed form of the pair criterion on the same frequency set, the maximiser against a grid, and
argument errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import eubo_ref
import path_ref as ph
import qeubo_ref as qr
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
    """tests/test_gpu_path_sample.py's bounds: v = K_y^-1 r carries cond(K_y) eps |v| on both sides; k . v adds it to f.  A qEUBO value
    is a mean of such values, a gradient block wins_i / S <= 1 times a mean of such gradients."""
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


# (SE, 300, 96, ..): D > 64, and 37 draws: the padding up to 128 must neither win nor contribute; (MATERN52, 700, 7, .., 130): a
# second 128-deep k-tile of the aggregation GEMM
CASES = [(ph.SE, 90, 2, 100, 3, 64), (ph.MATERN52, 90, 16, 1024, 4, 64), (ph.SE, 300, 96, 700, 2, 37), (ph.MATERN52, 700, 7, 300, 5, 130)]
# D > 128: two (D = 129) and three (D = 257) 128-column tiles in the gradient contractions, tiled routes only
CASES += [(ph.SE, 90, 129, 100, 2, 37), (ph.MATERN52, 130, 257, 300, 4, 37)]


@pytest.mark.parametrize("kernel,N,D,F,q,nd", CASES)
def test_agrees_with_the_restatement(m, ctx, kernel, N, D, F, q, nd):
    gp, ps, ref = setup(m, ctx, kernel, N, D, F, nd)
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 300))
    rv, rg, rw, gap = qr.qeubo(ref, sets, q)
    tol_v, tol_g = tolerances(ref)
    print(f"smallest gap {gap.min():.3g} = {gap.min() / tol_v:.3g} tol_v")
    assert gap.min() >= 100 * tol_v                    # a condition on the inputs: no winner can differ between the two sides
    val, grad, wins = ps.qeubo_eval(sets, q, want_wins=True)
    err_v, err_g = np.abs(val - rv).max(), np.abs(grad - rg).max()
    print(f"value error {err_v:.3g} (tol {tol_v:.3g}), gradient error {err_g:.3g} (tol {tol_g:.3g})")
    assert np.array_equal(wins, rw) and np.array_equal(wins.sum(axis=0), np.full(300, nd))
    assert err_v <= tol_v, (err_v, tol_v)
    assert err_g <= tol_g, (err_g, tol_g)
    # every output is optional and does not change the others
    assert np.array_equal(_bits(ps.qeubo_eval(sets, q, want_grad=False)), _bits(val))
    ps.close()
    gp.close()


@pytest.mark.parametrize("q", [1, 16])
def test_one_and_sixteen_options_at_one_set(m, ctx, q):
    kernel, N, D, F, _, nd = CASES[0]
    gp, ps, ref = setup(m, ctx, kernel, N, D, F, nd)
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 1))
    rv, rg, rw, gap = qr.qeubo(ref, sets, q)
    tol_v, tol_g = tolerances(ref)
    assert gap.min() >= 100 * tol_v
    val, grad, wins = ps.qeubo_eval(sets, q, want_wins=True)
    assert np.array_equal(wins, rw)
    assert np.abs(val - rv).max() <= tol_v and np.abs(grad - rg).max() <= tol_g
    if q == 1:                                                                   # the mean of the draws
        assert abs(val[0] - ps.eval_all(sets).mean()) <= tol_v and wins[0, 0] == nd
    else:
        lost = np.flatnonzero(wins[:, 0] == 0)
        for i in lost:                                                           # no draw won: exactly zero
            assert np.all(grad[i * D:(i + 1) * D, 0] == 0.0)
    ps.close()
    gp.close()


def test_consistent_with_the_path_entry_points(m, ctx):
    kernel, N, D, F, q, nd = CASES[0]
    M = 40
    gp, ps, ref = setup(m, ctx, kernel, N, D, F, nd)
    tol_v, tol_g = tolerances(ref)
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 300))[:, :M]
    val, grad, wins = ps.qeubo_eval(sets, q, want_wins=True)
    V = np.stack([ps.eval_all(sets[i * D:(i + 1) * D]) for i in range(q)])      # q x M x nd
    top = np.sort(V, axis=0)
    assert (top[-1] - top[-2]).min() >= 100 * tol_v
    arg = np.argmax(V, axis=0)
    assert np.abs(val - V.max(axis=0).mean(axis=1)).max() <= tol_v
    assert np.array_equal(wins, np.stack([(arg == i).sum(axis=1) for i in range(q)]))
    # the gradient of option i: the sum over the draws it wins of sls_path_eval's gradients, over S
    mm, ss = np.meshgrid(np.arange(M), np.arange(nd), indexing="ij")
    mm, ss = mm.ravel(), ss.ravel()
    win = arg[mm, ss]
    pts = np.stack([sets[win[k] * D:(win[k] + 1) * D, mm[k]] for k in range(mm.size)], axis=1)
    _, g = ps.eval(pts, ss)
    want = np.zeros((q * D, M))
    for k in range(mm.size):
        want[win[k] * D:(win[k] + 1) * D, mm[k]] += g[:, k]
    assert np.abs(grad - want / nd).max() <= tol_g
    ps.close()
    gp.close()


def test_bit_contract(m, ctx):
    D, N, F, q, nd, M = 3, 120, 300, 4, 20, 300
    X, y, theta = problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    rng = np.random.default_rng(3)
    sets = rng.uniform(0, 1, (q * D, M))
    val, grad, wins = ps.qeubo_eval(sets, q, want_wins=True)
    v2, g2, w2 = ps.qeubo_eval(sets, q, want_wins=True)
    assert np.array_equal(_bits(val), _bits(v2)) and np.array_equal(_bits(grad), _bits(g2)) and np.array_equal(wins, w2)
    # a set alone, and among others at another column
    v1, g1, w1 = ps.qeubo_eval(sets[:, 17:18], q, want_wins=True)
    assert _bits(v1)[0] == _bits(val)[17] and np.array_equal(_bits(g1[:, 0]), _bits(grad[:, 17])) and np.array_equal(w1[:, 0], wins[:, 17])
    perm = rng.permutation(M)
    vp, gp_, wp = ps.qeubo_eval(sets[:, perm], q, want_wins=True)
    assert np.array_equal(_bits(vp), _bits(val[perm])) and np.array_equal(_bits(gp_), _bits(grad[:, perm])) and np.array_equal(wp, wins[:, perm])
    # 256 POINTS per pass = 64 sets, rounded to the 128-set minimum: three passes instead of one
    ctx.set_candidate_chunk(256)
    try:
        vc, gc, wc = ps.qeubo_eval(sets, q, want_wins=True)
    finally:
        ctx.set_candidate_chunk(16384)
    assert np.array_equal(_bits(vc), _bits(val)) and np.array_equal(_bits(gc), _bits(grad)) and np.array_equal(wc, wins)
    # options permuted: the value's bits stay, gradient blocks and win counts move with their options
    order = np.array([2, 0, 3, 1])
    rows = np.concatenate([np.arange(i * D, (i + 1) * D) for i in order])
    vo, go, wo = ps.qeubo_eval(sets[rows], q, want_wins=True)
    assert np.array_equal(_bits(vo), _bits(val)) and np.array_equal(_bits(go), _bits(grad[rows])) and np.array_equal(wo, wins[order])
    # x_1 = x_0: the duplicate never wins, has an exactly zero gradient, and the value is the set's without it
    dup = sets.copy()
    dup[D:2 * D] = dup[:D]
    vd, gd, wd = ps.qeubo_eval(dup, q, want_wins=True)
    rest = np.concatenate([np.arange(0, D), np.arange(2 * D, q * D)])
    v3, g3, w3 = ps.qeubo_eval(dup[rest], q - 1, want_wins=True)
    assert np.all(wd[1] == 0) and np.all(gd[D:2 * D] == 0.0)
    assert np.array_equal(_bits(vd), _bits(v3)) and np.array_equal(_bits(gd[rest]), _bits(g3)) and np.array_equal(wd[[0, 2, 3]], w3)
    ps.close()
    gp.close()


def test_guard_on_the_device(m, ctx):
    """A NaN coordinate in one option: that set gets SLS_QEUBO_FLOOR and the zero gradient (qeubo_select's flag, qeubo_finish's scan),
    with or without the gradient asked for; its neighbours keep their bits."""
    D, N, F, q, nd = 3, 120, 300, 3, 20
    X, y, theta = problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    for M, bad in ((3, [1]), (300, [0, 130, 299])):
        sets = np.random.default_rng(5).uniform(0, 1, (q * D, M))
        val, grad, wins = ps.qeubo_eval(sets, q, want_wins=True)
        hit = sets.copy()
        for k, n in enumerate(bad):
            hit[(k % q) * D + 1, n] = np.nan                       # another option each time
        v, g, w = ps.qeubo_eval(hit, q, want_wins=True)
        good = np.setdiff1d(np.arange(M), bad)
        assert np.all(v[bad] == -1.0e300) and np.all(g[:, bad] == 0.0)
        assert np.array_equal(_bits(v[good]), _bits(val[good])) and np.array_equal(_bits(g[:, good]), _bits(grad[:, good]))
        assert np.array_equal(w[:, good], wins[:, good])
        assert np.array_equal(_bits(ps.qeubo_eval(hit, q, want_grad=False)), _bits(v))
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
r = ps.qeubo_maximize(rng.uniform(0, 1, (q * D, 300)), q, 25, opts=m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6))
st = gp.last_stats()
np.savez(sys.argv[2], x=r['x'], value=r['value'], index=r['index'], x_stars=r['x_stars'], y_stars=r['y_stars'],
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
    for k in ("x", "value", "x_stars", "y_stars"):
        assert np.array_equal(_bits(out["1"][k]), _bits(out["0"][k])), k
    assert out["1"]["index"] == out["0"]["index"]
    assert out["1"]["issued"] < out["1"]["cap"]           # starts did leave the batch: the two schedules differed


def test_central_differences_of_device_values(m, ctx):
    D, N, F, q, nd, M = 3, 50, 150, 3, 5, 64
    X, y, theta = problem(D, N, seed=24)
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, 0.02, ph.SE)
    ps = m.PathSamples(gp, nd, F, seed=3)
    ref = ph.PathRef(X, y, theta, 0.02, ph.SE, nd, F, seed=3)
    sets = np.random.default_rng(7).uniform(0.05, 0.95, (q * D, M))
    gap = qr.qeubo(ref, sets, q)[3]
    ok = gap >= 1e-4 * a                               # no winner changes inside the stencil
    assert ok.sum() >= 8, ok.sum()
    val, grad = ps.qeubo_eval(sets, q)
    h = 1e-6
    for r in range(q * D):
        E = np.zeros((q * D, M))
        E[r] = h
        fd = (ps.qeubo_eval(sets + E, q, want_grad=False) - ps.qeubo_eval(sets - E, q, want_grad=False)) / (2 * h)
        assert np.abs(fd - grad[r])[ok].max() <= 1e-6 * (a + np.abs(grad[:, ok]).max())
    ps.close()
    gp.close()


def test_two_options_against_the_fixed_basis_closed_form(m, ctx):
    D, N, F, S, b = 3, 200, 1024, 4096, 0.02
    X, y, theta = problem(D, N, seed=9, ell=0.35)
    gp = m.GP(ctx, X, y, theta, b, ph.SE)
    ps = m.PathSamples(gp, S, F, seed=F)
    ref = ph.PathRef(X, y, theta, b, ph.SE, S, F, seed=F)
    tol_v, _ = tolerances(ref)
    pairs = np.random.default_rng(2).uniform(0, 1, (2 * D, 64))
    val, wins = ps.qeubo_eval(pairs, 2, want_grad=False, want_wins=True)
    exact = eubo_ref.eubo(X, y, theta, b, eubo_ref.SE, pairs, s2=qr.pair_variance(ref, pairs[:D], pairs[D:]))[0]
    best = np.maximum(ps.eval_all(pairs[:D]), ps.eval_all(pairs[D:]))
    se = best.std(axis=1, ddof=1) / np.sqrt(S)
    dev = np.abs(val - exact)
    print(f"largest deviation {(dev / se).max():.2f} standard errors")
    assert np.all(dev <= 5 * se + tol_v), (dev / se).max()
    assert np.array_equal(wins.sum(axis=0), np.full(64, S))
    ps.close()
    gp.close()


def test_maximiser_against_the_grid(m, ctx):
    D, N, q, nd, F, S, n_local = 1, 30, 3, 32, 256, 1024, 60
    X, y, theta = problem(D, N, seed=41, ell=0.3)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.SE)
    ps = m.PathSamples(gp, nd, F, seed=17)
    starts = np.random.default_rng(8).uniform(0, 1, (q * D, S))
    at_start = ps.qeubo_eval(starts, q, want_grad=False)
    r = ps.qeubo_maximize(starts, q, n_local, offset=1000)
    st = gp.last_stats()
    # the 101^3 grid of sets from ONE evaluation of the grid points under every draw
    g1 = np.linspace(0, 1, 101)
    V = ps.eval_all(g1[None, :])                                                # 101 x nd
    two = np.maximum(V[:, None, :], V[None, :, :])                              # 101 x 101 x nd
    grid_best = max(np.maximum(two, V[k][None, None, :]).mean(axis=2).max() for k in range(101))
    # a set moves by at most half a step per coordinate to its nearest grid set; |d qEUBO / d x_i| <= max_s |f_s'(x_i)|
    _, gd = ps.eval(np.repeat(g1[None, :], nd, axis=1), np.tile(np.arange(nd), 101))
    slack = q * D * np.abs(gd).max() * 0.5 * (g1[1] - g1[0])
    print(f"winner {r['value']:.12g} at {r['x']}, grid maximum {grid_best:.12g}, resolution slack {slack:.3g}, stats {st}")
    assert r["value"] >= grid_best - slack
    x = r["x"]
    assert x.shape == (q * D,) and np.all((x >= 0) & (x <= 1))
    assert abs(ps.qeubo_eval(x[:, None], q, want_grad=False)[0] - r["value"]) <= 1e-12
    assert r["index"] - 1000 == int(np.argmax(r["y_stars"])) and r["value"] == r["y_stars"].max()
    assert np.array_equal(r["x_stars"][:, r["index"] - 1000], x)
    assert r["x_stars"].shape == (q * D, S) and np.all((r["x_stars"] >= 0) & (r["x_stars"] <= 1))
    assert np.abs(ps.qeubo_eval(r["x_stars"], q, want_grad=False) - r["y_stars"]).max() <= 1e-12
    assert np.all(r["y_stars"] >= at_start)
    assert 0 < st["evals_issued"] <= S * n_local and st["evals_cap"] == S * n_local and 1 <= st["rounds"] <= n_local
    r0 = ps.qeubo_maximize(starts, q, n_local, want_all=False)
    assert r0["index"] == r["index"] - 1000 and r0["value"] == r["value"] and np.array_equal(r0["x"], x)
    ps.close()
    gp.close()


def test_argument_errors_leave_the_context_usable(m, ctx):
    D, N, q = 3, 40, 2
    X, y, theta = problem(D, N, seed=6)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.SE)
    ps = m.PathSamples(gp, 4, 64, seed=1)
    lib, dp = m.lib(), C.POINTER(C.c_double)
    P = np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (17 * D, 3)))
    val, x, v, idx = np.empty(3), np.empty(17 * D), C.c_double(), C.c_long()
    p = lambda a: a.ctypes.data_as(dp)

    def ev(h, qq, Pp, M):
        return lib.sls_qeubo_eval(h, qq, Pp, M, p(val), None, None)

    def mx(h, qq, sp, S=3, n_local=5):
        return lib.sls_qeubo_maximize(h, qq, sp, S, n_local, None, C.c_long(0), p(x), C.byref(v), C.byref(idx), None, None)

    for qq in (0, 17, -1):
        assert ev(ps.h, qq, p(P), 3) == -1 and mx(ps.h, qq, p(P)) == -1, qq
    assert ev(None, q, p(P), 3) == -1 and ev(ps.h, q, None, 3) == -1 and ev(ps.h, q, p(P), -1) == -1
    assert mx(None, q, p(P)) == -1 and mx(ps.h, q, None) == -1 and mx(ps.h, q, p(P), S=0) == -1 and mx(ps.h, q, p(P), n_local=0) == -1
    assert ev(ps.h, q, p(P), 0) == 0                                # M = 0: nothing to do
    assert ev(ps.h, q, p(P), 3) == 0 and np.all(np.isfinite(val))
    assert lib.sls_qeubo_eval(ps.h, q, p(P), 3, None, None, None) == 0      # every output may be NULL
    assert mx(ps.h, q, p(P)) == 0 and np.isfinite(v.value)
    gp.append_point(np.full(D, 0.3), 0.1)                           # the path is stale now
    assert ev(ps.h, q, p(P), 3) == -1 and "refitted or grown" in lib.sls_last_error().decode()
    assert mx(ps.h, q, p(P)) == -1 and "refitted or grown" in lib.sls_last_error().decode()
    ps.close()
    ps2 = m.PathSamples(gp, 4, 64, seed=1)                          # the context and the handle still work
    v2 = ps2.qeubo_eval(P[:q * D], q, want_grad=False)
    assert np.all(np.isfinite(v2))
    ps2.close()
    gp.close()
