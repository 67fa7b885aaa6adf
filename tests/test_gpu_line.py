"""Line EUBO, the expected utility of the best of q grid positions on a slider, on the MI355X (sls_line_eval / sls_line_maximize):
agreement with the numpy restatement (tests/line_ref.py), the bit contract with the set routes (value and wins of sls_qeubo_eval /
sls_qnei_eval at the expanded set, the gradient its stated fold; column, other lines, lines per pass, SLS_COMPACT=0), mirror symmetry,
the degenerate line and the guard, central differences of the device values, the maximiser held start by start to the restated
L-BFGS (tests/lbfgs_ref.py on the device's own line_eval; cases in tests/line_cases.py), a deterministic usefulness check against the
line to the EI maximiser, and argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import line_cases as lc
import line_ref as lr
import maximize_cases as mc
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
@pytest.mark.parametrize("k", range(len(lc.RESTATED)))
def test_agrees_with_the_restatement(m, ctx, k):
    case = lc.RestatedCase(k)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    ref = ph.PathRef(case.X, case.y, case.theta, case.b, case.kernel, case.n_draws, case.F, seed=case.path_seed)
    tol_v, tol_g = tolerances(ref)
    for wb in case.with_baseline:
        t = ps.max_over_points(case.X)[0] if wb else None
        rv, rg, rw, gap = lr.line(ref, case.lines, case.q, case.anchor, baseline=t)
        val, grad, wins = ps.line_eval(case.lines, case.q, anchor=case.anchor, baseline=t, want_wins=True)
        cmp = gap >= tol_v                                  # elsewhere a winner may differ between the two sides
        err_v, err_g = np.abs(val - rv).max(), np.abs(grad - rg).max()
        print(f"case {k}{' with baseline' if wb else ''}: value error {err_v:.3g} (tol {tol_v:.3g}), gradient error {err_g:.3g} "
              f"(tol {tol_g:.3g}), wins compared at {cmp.sum()} of {case.M} lines, smallest gap {gap.min():.3g}")
        assert (~cmp).mean() <= 0.05
        assert grad.shape == rg.shape and wins.shape == (case.q, case.M)
        assert np.array_equal(wins[:, cmp], rw[:, cmp])
        assert np.all(wins.sum(axis=0) <= case.n_draws) if wb else np.array_equal(wins.sum(axis=0), np.full(case.M, case.n_draws))
        assert err_v <= tol_v, (err_v, tol_v)
        assert err_g <= tol_g, (err_g, tol_g)
        # every output is optional and does not change the others
        assert same(ps.line_eval(case.lines, case.q, anchor=case.anchor, baseline=t, want_grad=False), val)
    ps.close()
    gp.close()


# ---- 2. bit contract --------------------------------------------------------------------------------------------------------------------
def set_route(ps, sets, q, t):
    return ps.qeubo_eval(sets, q, want_wins=True) if t is None else ps.qnei_eval(sets, q, t, want_wins=True)


@pytest.mark.parametrize("anchored", [False, True], ids=["free", "anchored"])
@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_bits_are_those_of_the_set_routes(m, ctx, anchored, with_base):
    D, q, M = 5, 4, 300
    gp, ps, X, y, _ = setup(m, ctx, D)
    rng = np.random.default_rng(3)
    anchor = rng.uniform(0, 1, D) if anchored else None
    lines = rng.uniform(0, 1, (D if anchored else 2 * D, M))
    t = ps.max_over_points(X)[0] if with_base else None
    val, grad, wins = ps.line_eval(lines, q, anchor=anchor, baseline=t, want_wins=True)
    sets = lr.expand(lines, q, D, anchor)
    sv, sg, sw = set_route(ps, sets, q, t)
    assert same(val, sv) and np.array_equal(wins, sw)
    assert same(grad, lr.fold(sg, q, D, anchored=anchored))
    if with_base:
        assert np.any(val > 0.0)
    # a line alone, and among others at another column
    v1, g1, w1 = ps.line_eval(lines[:, 17:18], q, anchor=anchor, baseline=t, want_wins=True)
    assert _bits(v1)[0] == _bits(val)[17] and same(g1[:, 0], grad[:, 17]) and np.array_equal(w1[:, 0], wins[:, 17])
    perm = rng.permutation(M)
    vp, gp_, wp = ps.line_eval(lines[:, perm], q, anchor=anchor, baseline=t, want_wins=True)
    assert same(vp, val[perm]) and same(gp_, grad[:, perm]) and np.array_equal(wp, wins[:, perm])
    # 128 q POINTS per pass = 128 lines: three passes instead of one
    ctx.set_candidate_chunk(128 * q)
    try:
        vc, gc, wc = ps.line_eval(lines, q, anchor=anchor, baseline=t, want_wins=True)
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
D, N, q = 3, 200, 5
X = rng.uniform(0, 1, (D, N)); y = np.sin(X.sum(0)); theta = np.concatenate([[0.6], np.full(D, 0.4)])
ctx = m.Context(0)
gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
ps = m.PathSamples(gp, 24, 300, seed=8)
out = {}
for name, anchor, rows in (('free', None, 2 * D), ('anch', X[:, int(np.argmax(y))], D)):
    r = ps.line_maximize(rng.uniform(0, 1, (rows, 300)), q, 25, anchor=anchor, opts=m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6))
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


# ---- 3. mirror ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [3, 7, 16])
@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_mirror_symmetry(m, ctx, q, with_base):
    """Swapped ends: the value's bits, reversed wins, swapped gradient blocks -- bit for bit (the fold of the second end runs in
    decreasing i, the mirror image of the first end's order)."""
    D, M = 5, 200
    gp, ps, X, y, _ = setup(m, ctx, D)
    t = ps.max_over_points(X)[0] - 0.3 if with_base else None
    lines = np.random.default_rng(4).uniform(0, 1, (2 * D, M))
    swapped = np.concatenate([lines[D:], lines[:D]], axis=0)
    v, g, w = ps.line_eval(lines, q, baseline=t, want_wins=True)
    vs, gs, ws = ps.line_eval(swapped, q, baseline=t, want_wins=True)
    sets = lr.expand(lines, q, D)
    V = np.stack([ps.eval_all(sets[i * D:(i + 1) * D]) for i in range(q)])      # q x M x nd
    top = np.sort(V, axis=0)
    tie_free = (top[-1] - top[-2]).min(axis=1) > 0.0                            # a tie goes to the lowest index on either side
    assert tie_free.mean() >= 0.95
    assert same(vs, v)
    assert np.array_equal(ws[:, tie_free], w[::-1][:, tie_free])
    assert same(gs[:D, tie_free], g[D:, tie_free]) and same(gs[D:, tie_free], g[:D, tie_free])
    ps.close()
    gp.close()


# ---- 4. degenerate line and guard -----------------------------------------------------------------------------------------------------
def test_degenerate_line(m, ctx):
    """a = b where the expansion reproduces a at every position (q = 2, 3 always; q = 9 at coordinates that are multiples of 2^-10)."""
    D = 5
    gp, ps, X, y, _ = setup(m, ctx, D)
    rng = np.random.default_rng(6)
    for q, a in ((2, rng.uniform(0, 1, (D, 130))), (3, rng.uniform(0, 1, (D, 130))), (9, rng.integers(0, 1025, (D, 130)) / 1024.0)):
        lines = np.concatenate([a, a], axis=0)
        val, grad, wins = ps.line_eval(lines, q, want_wins=True)
        assert np.all(wins[0] == ND) and np.all(wins[1:] == 0)
        assert np.all(grad[D:] == 0.0)
        sg = ps.qeubo_eval(lr.expand(lines, q, D), q)[1]
        assert same(grad[:D], sg[:D])
        # anchored at the same point: grad_b alone
        gb = ps.line_eval(a[:, :1], q, anchor=a[:, 0])[1]
        assert np.all(gb == 0.0)
    ps.close()
    gp.close()


@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_guard_on_the_device(m, ctx, with_base):
    D, q = 3, 4
    gp, ps, X, y, _ = setup(m, ctx, D)
    t = ps.max_over_points(X)[0] - 0.3 if with_base else None
    floor = 0.0 if with_base else -1.0e300
    for M, bad in ((3, [1]), (300, [0, 130, 299])):
        lines = np.random.default_rng(5).uniform(0, 1, (2 * D, M))
        val, grad, wins = ps.line_eval(lines, q, baseline=t, want_wins=True)
        hit = lines.copy()
        for k, n in enumerate(bad):
            hit[(k % 2) * D + 1, n] = np.nan                       # a, then b
        v, g, w = ps.line_eval(hit, q, baseline=t, want_wins=True)
        good = np.setdiff1d(np.arange(M), bad)
        assert np.all(v[bad] == floor) and np.all(g[:, bad] == 0.0)
        assert same(v[good], val[good]) and same(g[:, good], grad[:, good]) and np.array_equal(w[:, good], wins[:, good])
        assert same(ps.line_eval(hit, q, baseline=t, want_grad=False), v)
    ps.close()
    gp.close()


# ---- 5. central differences ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,D,anchored", [(3, 5, False), (16, 3, True)])
def test_central_differences_of_device_values(m, ctx, q, D, anchored):
    M = 64
    gp, ps, X, y, theta = setup(m, ctx, D)
    a = theta[0]
    ref = ph.PathRef(X, y, theta, B, ph.MATERN52, ND, F, seed=1234 + D)
    rng = np.random.default_rng(7)
    anchor = rng.uniform(0.05, 0.95, D) if anchored else None
    rows = D if anchored else 2 * D
    lines = rng.uniform(0.05, 0.95, (rows, M))
    gap = lr.line(ref, lines, q, anchor)[3]
    ok = gap >= 1e-4 * a                               # no winner changes inside the stencil
    assert ok.sum() >= 8, ok.sum()
    val, grad = ps.line_eval(lines, q, anchor=anchor)
    h = 1e-6
    for r in range(rows):
        E = np.zeros((rows, M))
        E[r] = h
        fd = (ps.line_eval(lines + E, q, anchor=anchor, want_grad=False) - ps.line_eval(lines - E, q, anchor=anchor, want_grad=False)) / (2 * h)
        assert np.abs(fd - grad[r])[ok].max() <= 1e-6 * (a + np.abs(grad[:, ok]).max())
    ps.close()
    gp.close()


# ---- 6. the maximiser, start by start ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", lc.case_ids(), ids=lc.case_name)
def test_maximiser_held_to_the_restated_lbfgs(m, ctx, c):
    i, variant = c
    case = lc.LineCase(i)
    q, anchor = case.q, case.anchor
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    kw = mc.VARIANTS[variant]
    rg = ps.line_maximize(case.starts, q, mc.N_LOCAL, anchor=anchor, opts=m.LbfgsOpts(**kw) if kw else None)
    st = gp.last_stats()
    rr = mc.restated(lambda T: ps.line_eval(T, q, anchor=anchor), case, kw)
    mc.hold_to_restatement(rg, rr, lc.case_name(c), stats=st)
    assert rg["x_stars"].shape == (case.nvar, case.S) and rg["x"].shape == (case.nvar,)
    at_start = ps.line_eval(np.clip(case.starts, 0.0, 1.0), q, anchor=anchor, want_grad=False)
    assert np.all(rg["y_stars"] >= at_start)
    again = ps.line_eval(rg["x"][:, None], q, anchor=anchor, want_grad=False)[0]
    assert abs(again - rg["value"]) <= 1e-12 * max(1.0, abs(rg["value"]))
    ps.close()
    gp.close()


def test_maximiser_with_a_baseline(m, ctx):
    """The qNEI form through the maximiser: the baseline reaches every round (the winner's value is line_eval's with it)."""
    case = lc.LineCase(0)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    t = ps.max_over_points(case.X)[0] - 0.3
    r = ps.line_maximize(case.starts, case.q, mc.N_LOCAL, baseline=t)
    rr = mc.restated(lambda T: ps.line_eval(T, case.q, baseline=t), case, {})
    mc.hold_to_restatement(r, rr, "line-baseline", stats=gp.last_stats())
    again = ps.line_eval(r["x"][:, None], case.q, baseline=t, want_grad=False)[0]
    assert r["value"] > 0.0 and abs(again - r["value"]) <= 1e-12 * max(1.0, abs(r["value"]))
    ps.close()
    gp.close()


# ---- 7. usefulness ----------------------------------------------------------------------------------------------------------------------
def test_no_worse_than_the_line_to_the_ei_maximiser(m, ctx):
    """Anchored at the best data point, q = 9, with the EI maximiser of the same handle among the starts: a start never ends below
    where it began, so the returned slider's utility is at least that of the slider SubmitFeedbackData would show."""
    D, q, S = 5, 9, 129
    gp, ps, X, y, _ = setup(m, ctx, D)
    anchor = X[:, int(np.argmax(y))]
    starts = mc.box_starts(D, S, 77)
    x_ei = gp.acq_maximize(np.clip(starts, 0.0, 1.0), 50)["x"]
    starts[:, 5] = x_ei
    u_ei = ps.line_eval(x_ei[:, None], q, anchor=anchor, want_grad=False)[0]
    r = ps.line_maximize(starts, q, 50, anchor=anchor)
    print(f"utility of the returned slider {r['value']:.12g}, of the slider to the EI maximiser {u_ei:.12g}")
    assert r["value"] >= u_ei
    assert r["y_stars"][5] >= u_ei
    assert np.all((r["x"] >= 0.0) & (r["x"] <= 1.0)) and np.all((anchor >= 0.0) & (anchor <= 1.0))
    # the free form from the same slider
    free = np.concatenate([np.repeat(anchor[:, None], S, axis=1), starts], axis=0)
    rf = ps.line_maximize(free, q, 50)
    assert rf["value"] >= u_ei and np.all((rf["x"] >= 0.0) & (rf["x"] <= 1.0))
    ps.close()
    gp.close()


# ---- 8. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(m, ctx):
    import ctypes as C
    D, q = 3, 3
    X, y, theta = mc.problem(D, 40, seed=6)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.SE)
    ps = m.PathSamples(gp, 4, 64, seed=1)
    lines = np.random.default_rng(1).uniform(0, 1, (2 * D, 3))
    anchor, t = np.full(D, 0.5), np.zeros(4)
    for qq in (1, 17):
        with pytest.raises(m.SlsError):
            ps.line_eval(lines, qq)
        with pytest.raises(m.SlsError):
            ps.line_maximize(lines, qq, 5)
    with pytest.raises(m.SlsError, match="2D x M"):
        ps.line_eval(lines[:D], q)                                  # a wrong row count
    with pytest.raises(m.SlsError, match="D x M"):
        ps.line_eval(lines, q, anchor=anchor)
    bad_anchor, bad_t = anchor.copy(), t.copy()
    bad_anchor[1], bad_t[2] = np.nan, np.nan
    for kw in (dict(anchor=bad_anchor), dict(anchor=anchor, baseline=bad_t)):
        with pytest.raises(m.SlsError, match="not finite"):
            ps.line_eval(lines[D:], q, **kw)
        with pytest.raises(m.SlsError, match="not finite"):
            ps.line_maximize(lines[D:], q, 5, **kw)
    # the C ABI itself
    lib, dp = m.lib(), C.POINTER(C.c_double)
    Lf = np.asfortranarray(lines)
    p = lambda a: a.ctypes.data_as(dp)
    val, x, v, idx = np.empty(3), np.empty(2 * D), C.c_double(), C.c_long()

    def ev(h, qq, Lp, M):
        return lib.sls_line_eval(h, qq, None, None, Lp, M, p(val), None, None)

    def mx(h, qq, sp, S=3, n_local=5):
        return lib.sls_line_maximize(h, qq, None, None, sp, S, n_local, None, C.c_long(0), p(x), C.byref(v), C.byref(idx), None, None)

    for qq in (1, 17, 0, -1):
        assert ev(ps.h, qq, p(Lf), 3) == -1 and mx(ps.h, qq, p(Lf)) == -1, qq
    assert ev(None, q, p(Lf), 3) == -1 and ev(ps.h, q, None, 3) == -1 and ev(ps.h, q, p(Lf), -1) == -1
    assert mx(None, q, p(Lf)) == -1 and mx(ps.h, q, None) == -1 and mx(ps.h, q, p(Lf), S=0) == -1 and mx(ps.h, q, p(Lf), n_local=0) == -1
    assert ev(ps.h, q, p(Lf), 0) == 0                               # M = 0: nothing to do
    assert lib.sls_line_eval(ps.h, q, None, None, p(Lf), 3, None, None, None) == 0      # every output may be NULL
    # after every refusal a valid call succeeds
    assert np.all(np.isfinite(ps.line_eval(lines, q, want_grad=False)))
    assert np.isfinite(ps.line_maximize(lines[D:], q, 5, anchor=anchor, baseline=t)["value"])
    gp.append_point(np.full(D, 0.3), 0.1)                           # the path is stale now
    with pytest.raises(m.SlsError, match="refitted or grown"):
        ps.line_eval(lines, q)
    with pytest.raises(m.SlsError, match="refitted or grown"):
        ps.line_maximize(lines, q, 5)
    ps.close()
    ps2 = m.PathSamples(gp, 4, 64, seed=1)                          # the context and the handle still work
    assert np.all(np.isfinite(ps2.line_eval(lines, q, want_grad=False)))
    ps2.close()
    gp.close()
