"""Pathwise posterior function draws on the MI355X (sls_path_create / _eval / _maximize): agreement with the numpy restatement
(tests/path_ref.py) in value and gradient, the identity at the data, the statistics of 4096 draws against the posterior mean, the
closed-form pathwise covariance and the exact posterior covariance, the bit-level contract (reproducibility, prefix over draws,
independence of the other draws, SLS_COMPACT=0), the maximiser (grid optimum, consistency with eval, KKT in the box, full size) and
argument errors."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import path_ref as ph
import posterior_ref as pr
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
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


CASES = [(ph.SE, 90, 2, 100), (ph.MATERN52, 90, 16, 1024), (ph.SE, 700, 16, 4096), (ph.MATERN52, 700, 64, 100),
         (ph.SE, 2048, 64, 1024), (ph.MATERN52, 2048, 2, 4096),
         # D > 64 (the gradient GEMMs at D > 64 columns) and D > 128 (more than one 128-column output tile of the gradient GEMMs)
         (ph.SE, 300, 96, 700), (ph.MATERN52, 300, 300, 300),
         # D = 129: ONE live column in the second tile; D = 257: one in the third, with N just past one 128-row tile
         (ph.SE, 90, 129, 100), (ph.MATERN52, 130, 257, 300)]


@pytest.mark.parametrize("kernel,N,D,F", CASES)
def test_eval_agrees_with_the_restatement(m, ctx, kernel, N, D, F):
    b, nd, M = 0.05, 5, 300
    X, y, theta = problem(D, N, seed=N + D + F, ell=0.3 * np.sqrt(D))
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=1234 + D)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=1234 + D)
    rng = np.random.default_rng(1)
    Xs = rng.uniform(0, 1, (D, M))
    dr = rng.integers(0, nd, M)
    val, grad = ps.eval(Xs, dr)
    rv, rg = ref.eval(Xs, dr)
    allv = ps.eval_all(Xs)
    rall = ref.eval_all(Xs)
    # v = K_y^-1 r carries cond(K_y) eps |v| on both sides; k . v adds it to f
    ev = np.linalg.eigvalsh(ref.Ky)
    cond = ev[-1] / ev[0]
    vs = np.abs(ref.v).max()
    tol_v = 1e-10 * a + 4 * cond * EPS * vs * a * np.sqrt(N)
    tol_g = 1e-9 * a + 4 * cond * EPS * vs * a * np.sqrt(N) / theta[1:].min()
    err_v, err_all, err_g = np.abs(val - rv).max(), np.abs(allv - rall).max(), np.abs(grad - rg).max()
    assert err_v <= tol_v, (err_v, tol_v, cond)
    assert err_all <= tol_v, (err_all, tol_v, cond)
    assert err_g <= tol_g, (err_g, tol_g, cond)
    # the gathered and the every-draw forms agree
    assert np.abs(allv[np.arange(M), dr] - val).max() <= tol_v
    # gradients against central differences of the device values
    h = 1e-6
    sub = np.arange(8)
    for d in range(min(D, 4)):
        E = np.zeros((D, 8))
        E[d] = h
        fd = (ps.eval(Xs[:, sub] + E, dr[sub], want_grad=False) - ps.eval(Xs[:, sub] - E, dr[sub], want_grad=False)) / (2 * h)
        assert np.abs(fd - grad[d, sub]).max() <= 1e-6 * (a + np.abs(grad[:, sub]).max())
    ps.close()
    gp.close()


@pytest.mark.parametrize("kernel", [ph.SE, ph.MATERN52])
def test_identity_at_the_data(m, ctx, kernel):
    D, N, b, nd, F = 4, 150, 0.02, 6, 512
    X, y, theta = problem(D, N, seed=77 + kernel)
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=5)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=5)
    f = ps.eval_all(X)
    rhs = y[:, None] - np.sqrt(b) * ref.eps - b * ref.v
    assert np.abs(f - rhs).max() <= 1e-9 * (theta[0] + np.abs(y).max())
    ps.close()
    gp.close()


def test_statistics_of_4096_draws(m, ctx):
    D, N, M, S, b, kernel = 3, 200, 64, 4096, 0.02, ph.SE
    X, y, theta = problem(D, N, seed=9, ell=0.35)
    a = theta[0]
    rng = np.random.default_rng(2)
    Xs = rng.uniform(0, 1, (D, M))
    gp = m.GP(ctx, X, y, theta, b, kernel)
    mu, _ = gp.predict(Xs)
    _, cov_exact = gp.predict_cov(Xs)
    for F in (1024, 8192):
        ps = m.PathSamples(gp, S, F, seed=F)
        Fs = ps.eval_all(Xs)
        assert np.all(np.isfinite(Fs))
        mean = Fs.mean(axis=1)
        se = Fs.std(axis=1, ddof=1) / np.sqrt(S)
        assert np.all(np.abs(mean - mu) <= 5 * se + 1e-12)
        C_ = np.cov(Fs)
        om = ph.frequencies(F, D, F, kernel)
        Ps, PX = ph.features(om, a, Xs, theta[1:]), ph.features(om, a, X, theta[1:])
        KsX = pr.ard_kernel(Xs, X, theta, kernel)
        Ky = pr.ard_kernel(X, X, theta, kernel) + b * np.eye(N)
        cov = ph.pathwise_cov(Ps.T @ Ps, Ps.T @ PX, PX.T @ PX, KsX.T, Ky, b)
        sd = np.sqrt(np.outer(np.diag(cov), np.diag(cov)) + cov ** 2)
        assert np.all(np.abs(C_ - cov) <= 5 * sd / np.sqrt(S) + 1e-12)
        # against the exact posterior covariance: Monte-Carlo noise plus the shared-basis error of THIS frequency set, computed from
        # the restatement's frequencies (|cov_F - cov|, 5e-4 at F = 8192 here, about 1.5 % of the largest entry)
        delta = np.abs(cov - cov_exact)
        assert np.all(np.abs(C_ - cov_exact) <= 5 * sd / np.sqrt(S) + delta + 1e-12)
        if F == 8192:
            assert delta.max() <= 0.05 * np.abs(cov_exact).max() and delta.max() < delta_1024
        delta_1024 = delta.max()
        ps.close()
    gp.close()


def _bits(a):
    return np.asarray(a).view(np.uint64)


def test_bits_reproducible_prefix_and_independent(m, ctx):
    D, N, F, kernel = 3, 120, 300, ph.MATERN52
    X, y, theta = problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, kernel)
    rng = np.random.default_rng(3)
    Xs = rng.uniform(0, 1, (D, 200))
    dr = rng.integers(0, 3, 200)
    p8a, p8b, p3 = m.PathSamples(gp, 8, F, seed=42), m.PathSamples(gp, 8, F, seed=42), m.PathSamples(gp, 3, F, seed=42)
    va, ga = p8a.eval(Xs, dr)
    vb, gb = p8b.eval(Xs, dr)
    v3, g3 = p3.eval(Xs, dr)
    assert np.array_equal(_bits(va), _bits(vb)) and np.array_equal(_bits(ga), _bits(gb))
    assert np.array_equal(_bits(va), _bits(v3)) and np.array_equal(_bits(ga), _bits(g3))
    assert np.array_equal(_bits(p8a.eval_all(Xs)[:, :3]), _bits(p3.eval_all(Xs)))
    # a point alone, or among points of other draws, at another column: the same bits
    v1, g1 = p8a.eval(Xs[:, 17:18], dr[17:18])
    assert _bits(v1)[0] == _bits(va)[17] and np.array_equal(_bits(g1[:, 0]), _bits(ga[:, 17]))
    mixed = np.concatenate([Xs[:, 17:18]] * 5 + [Xs[:, :40]], axis=1)
    mdr = np.concatenate([[dr[17], 7, 5, 4, 6], np.full(40, 7)])
    vm_, _ = p8a.eval(mixed, mdr)
    assert _bits(vm_)[0] == _bits(va)[17]
    # maximise: the first 3 draws of the 8-draw object == the 3-draw object (the other draws' starts added)
    S = 40
    starts8 = rng.uniform(0, 1, (D, 8 * S))
    r8 = p8a.maximize(starts8, 20)
    r3 = p3.maximize(starts8[:, :3 * S], 20)
    assert np.array_equal(_bits(r8["x"][:, :3]), _bits(r3["x"]))
    assert np.array_equal(_bits(r8["value"][:3]), _bits(r3["value"]))
    assert np.array_equal(r8["index"][:3], r3["index"])
    for p in (p8a, p8b, p3):
        p.close()
    gp.close()


COMPACT_SCRIPT = r"""
import sys, importlib, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
m = importlib.import_module('sequential-line-search_amd')
rng = np.random.default_rng(12)
D, N = 5, 300
X = rng.uniform(0, 1, (D, N)); y = np.sin(X.sum(0)); theta = np.concatenate([[0.6], np.full(D, 0.4)])
ctx = m.Context(0)
gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
ps = m.PathSamples(gp, 6, 700, seed=8)
r = ps.maximize(rng.uniform(0, 1, (D, 6 * 50)), 30)
np.savez(sys.argv[2], x=r['x'], value=r['value'], index=r['index'])
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
    for k in ("x", "value", "index"):
        assert np.array_equal(out["1"][k].view(np.uint64) if k != "index" else out["1"][k],
                              out["0"][k].view(np.uint64) if k != "index" else out["0"][k]), k


@pytest.mark.parametrize("kernel", [ph.SE, ph.MATERN52])
def test_maximizer_beats_the_grid_and_is_stationary(m, ctx, kernel):
    D, N, nd, F, S = 2, 30, 4, 256, 256
    X, y, theta = problem(D, N, seed=50 + kernel)
    theta[1:] = [0.25, 0.3]
    a = theta[0]
    gp = m.GP(ctx, X, y, theta, 0.01, kernel)
    ps = m.PathSamples(gp, nd, F, seed=99)
    ref = ph.PathRef(X, y, theta, 0.01, kernel, nd, F, seed=99)
    rng = np.random.default_rng(4)
    starts = rng.uniform(0, 1, (D, nd * S))
    r = ps.maximize(starts, 60)
    g = np.linspace(0, 1, 512)
    G = np.stack(np.meshgrid(g, g, indexing="ij"), 0).reshape(2, -1)
    gmax = np.concatenate([ref.eval_all(G[:, i:i + 32768]) for i in range(0, G.shape[1], 32768)], axis=0).max(axis=0)
    assert np.all(r["value"] >= gmax - 1e-6 * a), (r["value"], gmax)
    assert np.all((r["x"] >= 0) & (r["x"] <= 1))
    assert np.all((r["index"] >= 0) & (r["index"] < S))
    v, gr = ps.eval(r["x"], np.arange(nd))
    assert np.array_equal(_bits(v), _bits(r["value"]))
    # projected gradient (maximisation in [0,1]^D): components pushing out of the box at a bound do not count
    x = r["x"]
    pg = np.where((x <= 0) & (gr < 0), 0.0, np.where((x >= 1) & (gr > 0), 0.0, gr))
    scale = a / theta[1:].min()
    assert np.abs(pg).max() <= 1e-4 * scale, (np.abs(pg).max(), scale)
    ps.close()
    gp.close()


def test_full_size_maximizer(m, ctx):
    D, N, F, nd, S, n_local = 64, 8192, 2048, 64, 1024, 50
    X, y, theta = problem(D, N, seed=3, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, 0.01, ph.SE)
    ps = m.PathSamples(gp, nd, F, seed=2024)
    rng = np.random.default_rng(5)
    starts = rng.uniform(0, 1, (D, nd * S))
    r = ps.maximize(starts, n_local)
    assert np.all(np.isfinite(r["value"])) and np.all(np.isfinite(r["x"]))
    v0 = ps.eval(starts, np.repeat(np.arange(nd), S), want_grad=False).reshape(nd, S)
    assert np.all(r["value"] >= v0.max(axis=1))
    ps.close()
    gp.close()


def test_errors_leave_the_context_usable(m, ctx):
    D, N = 3, 40
    X, y, theta = problem(D, N, seed=6)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.SE)
    L = m.lib()
    h = C.c_void_p()
    for nd, F in ((0, 10), (4097, 10), (2, 0), (2, 16385), (-1, 5)):
        rc = L.sls_path_create(gp.h, nd, F, C.c_ulonglong(1), C.byref(h))
        assert rc == -1 and not h.value, (nd, F)
    assert L.sls_path_create(None, 2, 10, C.c_ulonglong(1), C.byref(h)) == -1
    assert L.sls_path_create(gp.h, 2, 10, C.c_ulonglong(1), None) == -1
    ps = m.PathSamples(gp, 2, 64, seed=1)
    xs = np.full((D, 2), 0.5, order="F")
    xp = xs.ctypes.data_as(C.POINTER(C.c_double))
    val = np.empty(4)
    vp = val.ctypes.data_as(C.POINTER(C.c_double))
    bad = np.array([0, 2], dtype=np.int32)
    assert L.sls_path_eval(ps.h, xp, 2, bad.ctypes.data_as(C.POINTER(C.c_int)), vp, None) == -1
    assert L.sls_path_eval(ps.h, xp, 2, None, vp, vp) == -1          # every-draw form has no gradient
    assert L.sls_path_eval(None, xp, 2, None, vp, None) == -1
    assert L.sls_path_eval(ps.h, None, 2, None, vp, None) == -1
    assert L.sls_path_maximize(ps.h, None, 1, 5, None, None, None, None) == -1
    assert L.sls_path_maximize(ps.h, xp, 1, 0, None, None, None, None) == -1
    v_before = ps.eval_all(xs)
    gp.append_point(np.full(D, 0.3), 0.1)
    with pytest.raises(m.SlsError, match="refitted or grown"):
        ps.eval_all(xs)
    with pytest.raises(m.SlsError, match="refitted or grown"):
        ps.maximize(np.full((D, 2), 0.5), 3)
    ps.close()
    # the context and the handle still work: a new object on the grown handle
    ps2 = m.PathSamples(gp, 2, 64, seed=1)
    v_after = ps2.eval_all(xs)
    assert np.all(np.isfinite(v_after)) and v_before.shape == v_after.shape
    ps2.close()
    gp.close()
