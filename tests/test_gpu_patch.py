"""Gallery EUBO, the expected utility of the best cell of a qs x qt grid on a bilinear patch, on the MI355X (sls_patch_eval /
sls_patch_maximize): agreement with the numpy restatement (tests/patch_ref.py), the bit contract with the set routes (value and wins
of sls_qeubo_eval / sls_qnei_eval at the expanded set, the gradient its stated fold; column, other patches, patches per pass,
SLS_COMPACT=0), both mirror symmetries and the degenerate rows against sls_line_eval, the guard, central differences of the device
values, the maximiser held start by start to the restated L-BFGS (tests/lbfgs_ref.py on the device's own patch_eval; cases in
tests/patch_cases.py), a deterministic usefulness check against the best slider, and argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maximize_cases as mc
import patch_cases as pc
import patch_ref as pr
import path_ref as ph
from test_gpu_qeubo import tolerances
from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, F, ND, B = 60, 64, 8, 0.05


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


def setup(m, ctx, D, kernel=ph.MATERN52):
    """The shared fixture shape: N = 60, F = 64, 8 draws, b = 0.05, maximize_cases.problem data."""
    X, y, theta = mc.problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, B, kernel)
    ps = m.PathSamples(gp, ND, F, seed=1234 + D)
    return gp, ps, X, y, theta


# ---- 1. restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(pc.RESTATED)))
def test_agrees_with_the_restatement(m, ctx, k):
    case = pc.RestatedCase(k)
    qs, qt, q = case.qs, case.qt, case.qs * case.qt
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    ref = ph.PathRef(case.X, case.y, case.theta, case.b, case.kernel, case.n_draws, case.F, seed=case.path_seed)
    tol_v, tol_g = tolerances(ref)
    for wb in case.with_baseline:
        t = ps.max_over_points(case.X)[0] if wb else None
        rv, rg, rw, gap = pr.patch(ref, case.patches, qs, qt, case.anchor, baseline=t)
        val, grad, wins = ps.patch_eval(case.patches, qs, qt, anchor=case.anchor, baseline=t, want_wins=True)
        cmp = gap >= tol_v                                  # elsewhere a winner may differ between the two sides
        err_v, err_g = np.abs(val - rv).max(), np.abs(grad - rg).max()
        print(f"case {k}{' with baseline' if wb else ''}: value error {err_v:.3g} (tol {tol_v:.3g}), gradient error {err_g:.3g} "
              f"(tol {tol_g:.3g}), wins compared at {cmp.sum()} of {case.M} patches, smallest gap {gap.min():.3g}")
        assert (~cmp).mean() <= 0.05
        assert grad.shape == rg.shape == case.patches.shape and wins.shape == (q, case.M)
        assert np.array_equal(wins[:, cmp], rw[:, cmp])
        assert np.all(wins.sum(axis=0) <= case.n_draws) if wb else np.array_equal(wins.sum(axis=0), np.full(case.M, case.n_draws))
        assert err_v <= tol_v, (err_v, tol_v)
        assert err_g <= tol_g, (err_g, tol_g)
        # every output is optional and does not change the others
        kw = dict(anchor=case.anchor, baseline=t)
        assert same(ps.patch_eval(case.patches, qs, qt, want_grad=False, **kw), val)
        v2, w2 = ps.patch_eval(case.patches, qs, qt, want_grad=False, want_wins=True, **kw)
        assert same(v2, val) and np.array_equal(w2, wins)
        v3, g3 = ps.patch_eval(case.patches, qs, qt, **kw)
        assert same(v3, val) and same(g3, grad)
    ps.close()
    gp.close()


# ---- 2. bit contract --------------------------------------------------------------------------------------------------------------------
def set_route(ps, sets, q, t):
    return ps.qeubo_eval(sets, q, want_wins=True) if t is None else ps.qnei_eval(sets, q, t, want_wins=True)


@pytest.mark.parametrize("anchored", [False, True], ids=["free", "anchored"])
@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_bits_are_those_of_the_set_routes(m, ctx, anchored, with_base):
    D, qs, qt, M = 5, 3, 3, 300
    q = qs * qt
    gp, ps, X, y, _ = setup(m, ctx, D)
    rng = np.random.default_rng(3)
    anchor = rng.uniform(0, 1, D) if anchored else None
    patches = rng.uniform(0, 1, ((3 if anchored else 4) * D, M))
    t = ps.max_over_points(X)[0] if with_base else None
    kw = dict(anchor=anchor, baseline=t, want_wins=True)
    val, grad, wins = ps.patch_eval(patches, qs, qt, **kw)
    sets = pr.expand(patches, qs, qt, D, anchor)
    sv, sg, sw = set_route(ps, sets, q, t)
    assert same(val, sv) and np.array_equal(wins, sw)
    assert same(grad, pr.fold(sg, qs, qt, D, anchored=anchored))
    assert np.any(grad != 0.0)
    if with_base:
        assert np.any(val > 0.0)
    # a patch alone, and among others at another column
    v1, g1, w1 = ps.patch_eval(patches[:, 17:18], qs, qt, **kw)
    assert _bits(v1)[0] == _bits(val)[17] and same(g1[:, 0], grad[:, 17]) and np.array_equal(w1[:, 0], wins[:, 17])
    perm = rng.permutation(M)
    vp, gp_, wp = ps.patch_eval(patches[:, perm], qs, qt, **kw)
    assert same(vp, val[perm]) and same(gp_, grad[:, perm]) and np.array_equal(wp, wins[:, perm])
    # 128 q POINTS per pass = 128 patches: three passes instead of one
    ctx.set_candidate_chunk(128 * q)
    try:
        vc, gc, wc = ps.patch_eval(patches, qs, qt, **kw)
    finally:
        ctx.set_candidate_chunk(16384)
    assert same(vc, val) and same(gc, grad) and np.array_equal(wc, wins)
    ps.close()
    gp.close()


COMPACT_SCRIPT = r"""
import sys, importlib, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
m = importlib.import_module('sequential-line-search_amd')
rng = np.random.default_rng(12)
D, N, qs, qt = 3, 200, 3, 2
X = rng.uniform(0, 1, (D, N)); y = np.sin(X.sum(0)); theta = np.concatenate([[0.6], np.full(D, 0.4)])
ctx = m.Context(0)
gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
ps = m.PathSamples(gp, 24, 300, seed=8)
out = {}
for name, anchor, rows in (('free', None, 4 * D), ('anch', X[:, int(np.argmax(y))], 3 * D)):
    r = ps.patch_maximize(rng.uniform(0, 1, (rows, 300)), qs, qt, 25, anchor=anchor, opts=m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6))
    st = gp.last_stats()
    out.update({name + '_' + k: r[k] for k in ('x', 'value', 'index', 'x_stars', 'y_stars')})
    out[name + '_issued'], out[name + '_cap'] = st['evals_issued'], st['evals_cap']
np.savez(sys.argv[2], **out)
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
    for form in ("free", "anch"):
        for k in ("x", "value", "x_stars", "y_stars"):
            assert same(out["1"][f"{form}_{k}"], out["0"][f"{form}_{k}"]), (form, k)
        assert out["1"][f"{form}_index"] == out["0"][f"{form}_index"]
        assert out["1"][f"{form}_issued"] < out["1"][f"{form}_cap"]      # starts did leave the batch: the two schedules differed


# ---- 3. mirrors and degenerate rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qs,qt", [(3, 5), (8, 2), (4, 4)])
@pytest.mark.parametrize("axis", ["s", "t"])
@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_mirror_symmetry(m, ctx, qs, qt, axis, with_base):
    """Mirrored corners: the value's bits, wins reversed along the axis, gradient blocks swapped the same way -- bit for bit (the
    folds with the rising weights run down their axis, the mirror image of the order of those with the falling weights)."""
    D, M, q = 5, 200, qs * qt
    gp, ps, X, y, _ = setup(m, ctx, D)
    t = ps.max_over_points(X)[0] - 0.3 if with_base else None
    patches = np.random.default_rng(4).uniform(0, 1, (4 * D, M))
    mirrored = pr.mirror(patches, D, axis)
    perm = pr.mirror_cells(qs, qt, axis)
    v, g, w = ps.patch_eval(patches, qs, qt, baseline=t, want_wins=True)
    vm, gm, wm = ps.patch_eval(mirrored, qs, qt, baseline=t, want_wins=True)
    sets = pr.expand(patches, qs, qt, D)
    V = np.stack([ps.eval_all(sets[k * D:(k + 1) * D]) for k in range(q)])      # q x M x nd
    top = np.sort(V, axis=0)
    tie_free = (top[-1] - top[-2]).min(axis=1) > 0.0                            # a tie goes to the lowest index on either side
    assert tie_free.mean() >= 0.95
    assert same(vm, v)
    assert np.array_equal(wm[:, tie_free], w[perm][:, tie_free])
    assert same(gm[:, tie_free], pr.mirror(g, D, axis)[:, tie_free])
    assert np.any(g != 0.0)
    ps.close()
    gp.close()


@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_degenerate_rows_are_the_line(m, ctx, with_base):
    """qt = 2, c01 = c00, c11 = c10: both rows are the line's positions bit for bit; a tie goes to the lower index, i.e. to row 0."""
    D, M = 5, 130
    gp, ps, X, y, _ = setup(m, ctx, D)
    t = ps.max_over_points(X)[0] - 0.3 if with_base else None
    rng = np.random.default_rng(6)
    for qs in (2, 3, 8):
        lines = rng.uniform(0, 1, (2 * D, M))
        patches = np.concatenate([lines, lines], axis=0)
        lv, lg, lw = ps.line_eval(lines, qs, baseline=t, want_wins=True)
        v, g, w = ps.patch_eval(patches, qs, 2, baseline=t, want_wins=True)
        assert same(v, lv) and np.array_equal(w[:qs], lw) and np.all(w[qs:] == 0)
        assert same(g[:2 * D], lg) and np.all(g[2 * D:] == 0.0)
        # anchored at c00: the gradient of c10 is the anchored line's
        va, ga = ps.patch_eval(np.concatenate([lines[D:, :1], lines[:D, :1], lines[D:, :1]]), qs, 2, anchor=lines[:D, 0], baseline=t)
        la, lga = ps.line_eval(lines[D:, :1], qs, anchor=lines[:D, 0], baseline=t)
        assert same(va, la) and same(ga[:D], lga) and np.all(ga[D:] == 0.0)
    ps.close()
    gp.close()


# ---- 4. guard -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_guard_on_the_device(m, ctx, with_base):
    D, qs, qt = 3, 2, 3
    gp, ps, X, y, _ = setup(m, ctx, D)
    t = ps.max_over_points(X)[0] - 0.3 if with_base else None
    floor = 0.0 if with_base else -1.0e300
    for M, bad in ((3, [1]), (300, [0, 130, 131, 299])):
        patches = np.random.default_rng(5).uniform(0, 1, (4 * D, M))
        val, grad, wins = ps.patch_eval(patches, qs, qt, baseline=t, want_wins=True)
        hit = patches.copy()
        for k, n in enumerate(bad):
            hit[(k % 4) * D + 1, n] = np.nan                       # each corner in turn
        v, g, w = ps.patch_eval(hit, qs, qt, baseline=t, want_wins=True)
        good = np.setdiff1d(np.arange(M), bad)
        assert np.all(v[bad] == floor) and np.all(g[:, bad] == 0.0)
        assert same(v[good], val[good]) and same(g[:, good], grad[:, good]) and np.array_equal(w[:, good], wins[:, good])
        assert np.all(np.isfinite(v[good])) and np.all(np.isfinite(g[:, good]))
        assert same(ps.patch_eval(hit, qs, qt, baseline=t, want_grad=False), v)
    ps.close()
    gp.close()


# ---- 5. central differences ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qs,qt,D,anchored", [(3, 3, 5, False), (2, 4, 3, True)])
def test_central_differences_of_device_values(m, ctx, qs, qt, D, anchored):
    M = 48
    gp, ps, X, y, theta = setup(m, ctx, D)
    a = theta[0]
    ref = ph.PathRef(X, y, theta, B, ph.MATERN52, ND, F, seed=1234 + D)
    anchor = X[:, int(np.argmax(y))] if anchored else None
    rows = (3 if anchored else 4) * D
    patches = np.random.default_rng(11).uniform(0.05, 0.95, (rows, M))
    gap = pr.patch(ref, patches, qs, qt, anchor)[3]
    ok = gap >= 1e-4 * a                               # no winner changes inside the stencil
    assert ok.sum() >= 8, ok.sum()
    val, grad = ps.patch_eval(patches, qs, qt, anchor=anchor)
    h, worst = 1e-6, 0.0
    for r in range(rows):
        E = np.zeros((rows, M))
        E[r] = h
        fd = (ps.patch_eval(patches + E, qs, qt, anchor=anchor, want_grad=False)
              - ps.patch_eval(patches - E, qs, qt, anchor=anchor, want_grad=False)) / (2 * h)
        worst = max(worst, np.abs(fd - grad[r])[ok].max())
    bound = 1e-6 * (a + np.abs(grad[:, ok]).max())
    print(f"{qs} x {qt}, D = {D}: {ok.sum()} of {M} patches, worst error {worst:.3g} (bound {bound:.3g})")
    assert worst <= bound
    ps.close()
    gp.close()


# ---- 6. the maximiser, start by start ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.case_ids(), ids=pc.case_name)
def test_maximiser_held_to_the_restated_lbfgs(m, ctx, c):
    i, variant = c
    case = pc.PatchCase(i)
    qs, qt, anchor = case.qs, case.qt, case.anchor
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    kw = mc.VARIANTS[variant]
    rg = ps.patch_maximize(case.starts, qs, qt, mc.N_LOCAL, anchor=anchor, opts=m.LbfgsOpts(**kw) if kw else None)
    st = gp.last_stats()
    rr = mc.restated(lambda T: ps.patch_eval(T, qs, qt, anchor=anchor), case, kw)
    mc.hold_to_restatement(rg, rr, pc.case_name(c), stats=st)
    assert rg["x_stars"].shape == (case.nvar, case.S) and rg["x"].shape == (case.nvar,)
    at_start = ps.patch_eval(np.clip(case.starts, 0.0, 1.0), qs, qt, anchor=anchor, want_grad=False)
    assert np.all(rg["y_stars"] >= at_start)
    again = ps.patch_eval(rg["x"][:, None], qs, qt, anchor=anchor, want_grad=False)[0]
    assert abs(again - rg["value"]) <= 1e-12 * max(1.0, abs(rg["value"]))
    ps.close()
    gp.close()


def test_maximiser_with_a_baseline(m, ctx):
    """The qNEI form through the maximiser: the baseline reaches every round (the winner's value is patch_eval's with it)."""
    case = pc.PatchCase(0)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    t = ps.max_over_points(case.X)[0] - 0.3
    r = ps.patch_maximize(case.starts, case.qs, case.qt, mc.N_LOCAL, baseline=t)
    rr = mc.restated(lambda T: ps.patch_eval(T, case.qs, case.qt, baseline=t), case, {})
    mc.hold_to_restatement(r, rr, "patch-baseline", stats=gp.last_stats())
    again = ps.patch_eval(r["x"][:, None], case.qs, case.qt, baseline=t, want_grad=False)[0]
    assert r["value"] > 0.0 and abs(again - r["value"]) <= 1e-12 * max(1.0, abs(r["value"]))
    ps.close()
    gp.close()


# ---- 7. usefulness ----------------------------------------------------------------------------------------------------------------------
def test_no_worse_than_the_best_slider(m, ctx):
    """Anchored at the best data point, an 8 x 2 grid, with the degenerate patch of the best 8-position slider among the starts: its
    utility is that slider's (the degenerate-rows identity) and a start never ends below where it began, so the returned gallery's
    utility is at least the slider's."""
    D, qs, qt, S = 5, 8, 2, 129
    gp, ps, X, y, _ = setup(m, ctx, D)
    anchor = X[:, int(np.argmax(y))]
    line = ps.line_maximize(mc.box_starts(D, S, 77), qs, 50, anchor=anchor)
    starts = mc.box_starts(3 * D, S, 78)
    starts[:, 5] = np.concatenate([line["x"], anchor, line["x"]])           # c10 = b, c01 = c00 = anchor, c11 = b
    u_line = ps.patch_eval(starts[:, 5:6], qs, qt, anchor=anchor, want_grad=False)[0]
    assert _bits(u_line) == _bits(ps.line_eval(line["x"][:, None], qs, anchor=anchor, want_grad=False)[0])
    r = ps.patch_maximize(starts, qs, qt, 50, anchor=anchor)
    print(f"utility of the returned gallery {r['value']:.12g}, of the best slider {line['value']:.12g}")
    assert r["value"] >= line["value"]
    assert r["y_stars"][5] >= line["value"]
    assert np.all((r["x"] >= 0.0) & (r["x"] <= 1.0)) and np.all((anchor >= 0.0) & (anchor <= 1.0))
    ps.close()
    gp.close()


# ---- 8. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(m, ctx):
    import ctypes as C
    D, qs, qt = 3, 2, 3
    X, y, theta = mc.problem(D, 40, seed=6)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.SE)
    ps = m.PathSamples(gp, 4, 64, seed=1)
    patches = np.random.default_rng(1).uniform(0, 1, (4 * D, 3))
    anchor, t = np.full(D, 0.5), np.zeros(4)
    for grid in ((1, 4), (4, 1), (5, 4), (0, 2)):
        with pytest.raises(m.SlsError):
            ps.patch_eval(patches, *grid)
        with pytest.raises(m.SlsError):
            ps.patch_maximize(patches, *grid, 5)
    with pytest.raises(m.SlsError, match="4D x M"):
        ps.patch_eval(patches[:D], qs, qt)                           # a wrong row count
    with pytest.raises(m.SlsError, match="3D x M"):
        ps.patch_eval(patches, qs, qt, anchor=anchor)
    bad_anchor, bad_t = anchor.copy(), t.copy()
    bad_anchor[1], bad_t[2] = np.nan, np.nan
    for kw in (dict(anchor=bad_anchor), dict(anchor=anchor, baseline=bad_t)):
        with pytest.raises(m.SlsError, match="not finite"):
            ps.patch_eval(patches[D:], qs, qt, **kw)
        with pytest.raises(m.SlsError, match="not finite"):
            ps.patch_maximize(patches[D:], qs, qt, 5, **kw)
    # the C ABI itself
    lib, dp = m.lib(), C.POINTER(C.c_double)
    Pf = np.asfortranarray(patches)
    p = lambda a: a.ctypes.data_as(dp)
    val, x, v, idx = np.empty(3), np.empty(4 * D), C.c_double(), C.c_long()

    def ev(h, gs, gt, Pp, M):
        return lib.sls_patch_eval(h, gs, gt, None, None, Pp, M, p(val), None, None)

    def mx(h, gs, gt, sp, S=3, n_local=5):
        return lib.sls_patch_maximize(h, gs, gt, None, None, sp, S, n_local, None, C.c_long(0), p(x), C.byref(v), C.byref(idx), None,
                                      None)

    for gs, gt in ((1, 4), (4, 1), (5, 4), (0, 2), (2, 0), (-1, -16), (17, 1), (2, 9), (65536, 65536)):
        assert ev(ps.h, gs, gt, p(Pf), 3) == -1 and mx(ps.h, gs, gt, p(Pf)) == -1, (gs, gt)
    assert ev(None, qs, qt, p(Pf), 3) == -1 and ev(ps.h, qs, qt, None, 3) == -1 and ev(ps.h, qs, qt, p(Pf), -1) == -1
    assert mx(None, qs, qt, p(Pf)) == -1 and mx(ps.h, qs, qt, None) == -1
    assert mx(ps.h, qs, qt, p(Pf), S=0) == -1 and mx(ps.h, qs, qt, p(Pf), n_local=0) == -1
    assert ev(ps.h, qs, qt, p(Pf), 0) == 0                          # M = 0: nothing to do
    assert lib.sls_patch_eval(ps.h, qs, qt, None, None, p(Pf), 3, None, None, None) == 0      # every output may be NULL
    # after every refusal a valid call succeeds
    assert np.all(np.isfinite(ps.patch_eval(patches, qs, qt, want_grad=False)))
    assert np.isfinite(ps.patch_maximize(patches[D:], qs, qt, 5, anchor=anchor, baseline=t)["value"])
    gp.append_point(np.full(D, 0.3), 0.1)                           # the path is stale now
    with pytest.raises(m.SlsError, match="refitted or grown"):
        ps.patch_eval(patches, qs, qt)
    with pytest.raises(m.SlsError, match="refitted or grown"):
        ps.patch_maximize(patches, qs, qt, 5)
    assert ev(ps.h, qs, qt, p(Pf), 3) == -1                         # SLS_ERR_INVALID
    ps.close()
    ps2 = m.PathSamples(gp, 4, 64, seed=1)                          # the context and the handle still work
    assert np.all(np.isfinite(ps2.patch_eval(patches, qs, qt, want_grad=False)))
    ps2.close()
    gp.close()
