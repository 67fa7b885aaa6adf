"""Line EUBO without a GPU: the numpy restatement (tests/line_ref.py) -- its fold against central differences of its value, mirror
symmetry to the bit, the degenerate line --, the order sensitivity of the maximiser cases (tests/line_cases.py), the C ABI's
declarations and exports, and the Python wrapper's argument checks."""
import os
import re

import numpy as np
import pytest

import lbfgs_ref
import line_cases as lc
import line_ref as lr
import maximize_cases as mc
import path_ref as ph
import qeubo_ref as qr
import qnei_ref as nr
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, F, S, B = 60, 64, 8, 0.05


def make_ref(D):
    X, y, theta = mc.problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    return ph.PathRef(X, y, theta, B, ph.MATERN52, S, F, seed=1234 + D), X, y


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def test_weights_mirror_and_ends():
    for q in range(2, 17):
        u, t = lr.weights(q)
        assert np.array_equal(_bits(u), _bits(t[::-1]))
        assert u[0] == 1.0 and t[0] == 0.0 and u[-1] == 0.0 and t[-1] == 1.0
    lines = np.random.default_rng(0).uniform(0, 1, (6, 7))
    sets = lr.expand(lines, 5, 3)
    assert np.array_equal(sets[:3], lines[:3]) and np.array_equal(sets[-3:], lines[3:])     # x_0 = a, x_{q-1} = b


@pytest.mark.parametrize("q,D", [(3, 5), (16, 3)])
@pytest.mark.parametrize("anchored", [False, True], ids=["free", "anchored"])
def test_fold_against_central_differences(q, D, anchored):
    """The gap of a line bounds how far its values may move before a winner changes: the stencil stays far inside it."""
    ref, X, y = make_ref(D)
    a = ref.a
    anchor = X[:, int(np.argmax(y))] if anchored else None
    rows = D if anchored else 2 * D
    lines = np.random.default_rng(11).uniform(0.05, 0.95, (rows, 48))
    val, grad, wins, gap = lr.line(ref, lines, q, anchor)
    ok = gap >= 1e-4 * a
    print(f"q = {q}, D = {D}, {'anchored' if anchored else 'free'}: {ok.sum()} of 48 lines with a gap of at least 1e-4 a")
    assert ok.sum() >= 8, ok.sum()
    h = 1e-6
    for r in range(rows):
        E = np.zeros((rows, 48))
        E[r] = h
        fd = (lr.line(ref, lines + E, q, anchor)[0] - lr.line(ref, lines - E, q, anchor)[0]) / (2 * h)
        assert np.abs(fd - grad[r])[ok].max() <= 1e-6 * (a + np.abs(grad[:, ok]).max())


@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_mirror_symmetry_to_the_bit(with_base):
    D, q = 5, 7
    ref, X, y = make_ref(D)
    t = nr.max_over_points(ref, X)[0] - 0.3 if with_base else None
    lines = np.random.default_rng(4).uniform(0, 1, (2 * D, 40))
    swapped = np.concatenate([lines[D:], lines[:D]], axis=0)
    sets, sw = lr.expand(lines, q, D), lr.expand(swapped, q, D)
    rev = np.concatenate([np.arange(i * D, (i + 1) * D) for i in range(q - 1, -1, -1)])
    assert np.array_equal(_bits(sw), _bits(sets[rev]))                  # the reversed set, bit for bit
    v, g, w, _ = lr.line(ref, lines, q, baseline=t)
    vs, gs, ws, _ = lr.line(ref, swapped, q, baseline=t)
    tie_free = (lr.line(ref, lines, q, baseline=t)[3] > 0.0)
    assert tie_free.all()                                               # no ties: reversing the options reverses the winners
    assert np.array_equal(_bits(vs), _bits(v)) and np.array_equal(ws, w[::-1])
    assert np.array_equal(_bits(gs[:D]), _bits(g[D:])) and np.array_equal(_bits(gs[D:]), _bits(g[:D]))


def test_degenerate_line():
    """a = b where the expansion reproduces a at every position (q = 3 always; q = 9 at coordinates with few mantissa bits): every
    option ties, position 0 wins every draw, grad_b is exactly zero and grad_a is the set gradient's first block."""
    D = 5
    ref, X, y = make_ref(D)
    rng = np.random.default_rng(6)
    for q, a in ((2, rng.uniform(0, 1, (D, 9))), (3, rng.uniform(0, 1, (D, 9))), (9, rng.integers(0, 1025, (D, 9)) / 1024.0)):
        lines = np.concatenate([a, a], axis=0)
        sets = lr.expand(lines, q, D)
        assert all(np.array_equal(sets[i * D:(i + 1) * D], a) for i in range(q))
        val, grad, wins, gap = lr.line(ref, lines, q)
        assert np.all(wins[0] == S) and np.all(wins[1:] == 0) and np.all(gap == 0.0)
        assert np.all(grad[D:] == 0.0)
        assert np.array_equal(grad[:D], qr.qeubo(ref, sets, q)[1][:D])


def test_guarded_line_folds_to_zero():
    D, q = 3, 4
    ref, X, y = make_ref(D)
    lines = np.random.default_rng(8).uniform(0, 1, (2 * D, 5))
    lines[D + 1, 2] = np.nan
    with np.errstate(all="ignore"):
        val, grad, wins, _ = lr.line(ref, lines, q)
        vb, gb, _, _ = lr.line(ref, lines, q, baseline=np.zeros(S))
    assert val[2] == -1.0e300 and vb[2] == 0.0 and np.all(grad[:, 2] == 0.0) and np.all(gb[:, 2] == 0.0)
    assert np.all(np.isfinite(val[[0, 1, 3, 4]])) and np.all(np.isfinite(grad[:, [0, 1, 3, 4]]))


@pytest.fixture(scope="module")
def runs():
    """(shape, variant) -> (case, lanes run, sequential run) on the CPU objective; each computed once."""
    out = {}
    for i in range(len(lc.LINES)):
        case = lc.LineCase(i)
        ref = ph.PathRef(case.X, case.y, case.theta, case.b, case.kernel, case.n_draws, case.F, case.path_seed)
        evaluate = lambda T, ref=ref, case=case: lr.line(ref, T, case.q, case.anchor)[:2]
        for v in mc.VARIANTS:
            out[i, v] = (case,) + tuple(lbfgs_ref.run(evaluate, case.starts, mc.N_LOCAL, order=o, **mc.VARIANTS[v])
                                        for o in ("lanes", "sequential"))
    return out


@pytest.mark.parametrize("c", lc.case_ids(), ids=lc.case_name)
def test_at_most_two_percent_of_the_starts_depend_on_the_summation_order(runs, c):
    case, a, b = runs[c]
    scale = np.abs(b["y_stars"]).max()
    apart = np.abs(a["y_stars"] - b["y_stars"]) > 1e-6 * scale
    print(f"{lc.case_name(c)}: {apart.sum()} of {case.S} starts ({apart.mean():.2%}) end more than 1e-6 apart between the two orders; "
          f"evaluations {a['evals_issued']}, live at the end {a['live_at_end']}, ring {a['ring_max'].max()}, "
          f"smallest Armijo margin {a['armijo_margin'].min():.2e}")
    assert apart.mean() <= 0.02
    assert np.all(a["y_stars"] > 0.1 * mc.FLOOR)                        # no start of a case sits at the guard's floor


@pytest.mark.parametrize("k", range(len(lc.RESTATED)))
def test_inputs_of_the_restatement_test_keep_their_winners(k):
    """tests/test_gpu_line.py compares win counts wherever the restated gap is at least the value tolerance (test_gpu_qeubo.py's):
    at most 5 % of a case's lines may be closer than that."""
    from test_gpu_qeubo import tolerances
    case = lc.RestatedCase(k)
    ref = ph.PathRef(case.X, case.y, case.theta, case.b, case.kernel, case.n_draws, case.F, case.path_seed)
    tol_v, _ = tolerances(ref)
    for wb in case.with_baseline:
        t = nr.max_over_points(ref, case.X)[0] if wb else None
        val, grad, wins, gap = lr.line(ref, case.lines, case.q, case.anchor, baseline=t)
        close = gap < tol_v
        print(f"case {k}{' with baseline' if wb else ''}: {close.sum()} of {case.M} lines with a gap inside {tol_v:.3g}, smallest {gap.min():.3g}")
        assert close.mean() <= 0.05
        if wb:
            assert np.any(val > 0.0)


def test_header_declares_library_exports_and_binding_checks():
    import __graft_entry__ as g
    g.build()
    txt = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = sls()
    lib = m.lib()
    for name in ("sls_line_eval", "sls_line_maximize"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in m.EXPORTS
        assert hasattr(lib, name), f"libsls_hip.so does not export {name}"
    assert re.search(r"#define\s+SLS_LINE_MIN_POSITIONS\s+2\b", code) and m.LINE_MIN_POSITIONS == 2
    assert '"line"' in txt
    ps = m.PathSamples.__new__(m.PathSamples)            # refused before anything is allocated or called
    ps.D, ps.n_draws, ps.h = 2, 4, None
    for q in (1, 17, 0, -1):
        with pytest.raises(m.SlsError, match="2 .. 16"):
            ps.line_eval(np.zeros((4, 1)), q)
        with pytest.raises(m.SlsError, match="2 .. 16"):
            ps.line_maximize(np.zeros((4, 1)), q, 3)
    with pytest.raises(m.SlsError, match="2D x M"):
        ps.line_eval(np.zeros((2, 1)), 3)
    with pytest.raises(m.SlsError, match="D x M = 2 x M"):
        ps.line_eval(np.zeros((4, 1)), 3, anchor=np.zeros(2))
    with pytest.raises(m.SlsError, match="2D x M"):
        ps.line_maximize(np.zeros((3, 1)), 3, 5)
    with pytest.raises(m.SlsError, match="anchor must hold D = 2"):
        ps.line_eval(np.zeros((2, 1)), 3, anchor=np.zeros(3))
    with pytest.raises(m.SlsError, match="n_draws = 4"):
        ps.line_eval(np.zeros((4, 1)), 3, baseline=np.zeros(5))
    with pytest.raises(m.SlsError, match="n_draws = 4"):
        ps.line_maximize(np.zeros((2, 1)), 3, 5, anchor=np.zeros(2), baseline=np.zeros(3))
