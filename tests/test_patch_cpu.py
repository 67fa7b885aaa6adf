"""Gallery EUBO without a GPU: the numpy restatement (tests/patch_ref.py) -- corners and weights, its fold against central differences
of its value, both mirror symmetries to the bit, the transposition to rounding, the degenerate rows against tests/line_ref.py, the
guard --, the two caps on the shared cases (tests/patch_cases.py: winners kept, order sensitivity of the maximiser cases), the C
ABI's declarations and exports, and the Python wrapper's argument checks."""
import os
import re

import numpy as np
import pytest

import lbfgs_ref
import line_ref as lr
import maximize_cases as mc
import patch_cases as pc
import patch_ref as pr
import path_ref as ph
import qnei_ref as nr
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, F, S, B = 60, 64, 8, 0.05
GRIDS = [(qs, qt) for qs in range(2, 9) for qt in range(2, 9) if qs * qt <= 16]


def make_ref(D):
    X, y, theta = mc.problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
    return ph.PathRef(X, y, theta, B, ph.MATERN52, S, F, seed=1234 + D), X, y


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_corner_cells_are_the_corners_exactly():
    D = 3
    rng = np.random.default_rng(0)
    anchor = rng.uniform(0, 1, D)
    for qs, qt in GRIDS:
        for a in (None, anchor):
            patches = rng.uniform(0, 1, ((4 if a is None else 3) * D, 7))
            c = pr.split(patches, D, a)
            sets = pr.expand(patches, qs, qt, D, a)
            cell = lambda i, j: sets[(i + qs * j) * D:(i + qs * j + 1) * D]
            assert sets.shape == (qs * qt * D, 7)
            assert same(cell(0, 0), c[0]) and same(cell(qs - 1, 0), c[1])
            assert same(cell(0, qt - 1), c[2]) and same(cell(qs - 1, qt - 1), c[3])
            lo, hi = np.minimum.reduce(c), np.maximum.reduce(c)           # a convex combination of the corners, up to its roundings
            for k in range(qs * qt):
                x = sets[k * D:(k + 1) * D]
                assert np.all(x >= lo - 4e-16) and np.all(x <= hi + 4e-16)


@pytest.mark.parametrize("qs,qt,D", [(3, 3, 5), (2, 4, 3)])
@pytest.mark.parametrize("anchored", [False, True], ids=["free", "anchored"])
def test_fold_against_central_differences(qs, qt, D, anchored):
    """The gap of a patch bounds how far its values may move before a winner changes: the stencil stays far inside it."""
    ref, X, y = make_ref(D)
    a = ref.a
    anchor = X[:, int(np.argmax(y))] if anchored else None
    rows = (3 if anchored else 4) * D
    patches = np.random.default_rng(11).uniform(0.05, 0.95, (rows, 48))
    val, grad, wins, gap = pr.patch(ref, patches, qs, qt, anchor)
    ok = gap >= 1e-4 * a
    assert ok.sum() >= 8, ok.sum()
    h, worst = 1e-6, 0.0
    for r in range(rows):
        E = np.zeros((rows, 48))
        E[r] = h
        fd = (pr.patch(ref, patches + E, qs, qt, anchor)[0] - pr.patch(ref, patches - E, qs, qt, anchor)[0]) / (2 * h)
        worst = max(worst, np.abs(fd - grad[r])[ok].max())
    bound = 1e-6 * (a + np.abs(grad[:, ok]).max())
    print(f"{qs} x {qt}, D = {D}, {'anchored' if anchored else 'free'}: {ok.sum()} of 48 patches with a gap of at least 1e-4 a, "
          f"worst error {worst:.3g} (bound {bound:.3g})")
    assert worst <= bound


@pytest.mark.parametrize("axis", ["s", "t"])
@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_mirror_symmetry_to_the_bit(axis, with_base):
    D, qs, qt = 5, 3, 5
    ref, X, y = make_ref(D)
    t = nr.max_over_points(ref, X)[0] - 0.3 if with_base else None
    patches = np.random.default_rng(4).uniform(0, 1, (4 * D, 40))
    mirrored = pr.mirror(patches, D, axis)
    perm = pr.mirror_cells(qs, qt, axis)
    rows = np.concatenate([np.arange(k * D, (k + 1) * D) for k in perm])
    assert same(pr.expand(mirrored, qs, qt, D), pr.expand(patches, qs, qt, D)[rows])       # the permuted set, bit for bit
    v, g, w, gap = pr.patch(ref, patches, qs, qt, baseline=t)
    vm, gm, wm, _ = pr.patch(ref, mirrored, qs, qt, baseline=t)
    assert np.all(gap > 0.0)                                            # no ties: permuting the options permutes the winners
    assert same(vm, v) and np.array_equal(wm, w[perm])
    assert same(gm, pr.mirror(g, D, axis))
    assert np.any(g != 0.0)


def test_transposition_to_rounding_only():
    """c10 <-> c01 with qs <-> qt names the same cells, but the two nestings of the expansion round differently: the cells agree to
    a few units in the last place of a coordinate in [0,1], and values and gradients to the tolerances the device is held to."""
    from test_gpu_qeubo import tolerances
    D, qs, qt = 5, 3, 5
    ref, X, y = make_ref(D)
    tol_v, tol_g = tolerances(ref)
    patches = np.random.default_rng(4).uniform(0, 1, (4 * D, 40))
    tr = np.concatenate([patches[c * D:(c + 1) * D] for c in (0, 2, 1, 3)], axis=0)
    cells = np.array([j + qt * i for j in range(qt) for i in range(qs)])     # cell (i, j) of the patch is cell (j, i) of the transposed
    rows = np.concatenate([np.arange(k * D, (k + 1) * D) for k in cells])
    e, et = pr.expand(patches, qs, qt, D), pr.expand(tr, qt, qs, D)[rows]
    # the same bilinear form of the same rounded weights on both sides; each side rounds 9 times on the way (lo, hi: three each, then
    # three more), of which 6 reach a cell with weight at most one: at most 2^-54 each for numbers in [0,1]
    assert np.abs(e - et).max() <= 12 * 2.0 ** -54 and not same(e, et)
    v, g, w, gap = pr.patch(ref, patches, qs, qt)
    vt, gt, wt, _ = pr.patch(ref, tr, qt, qs)
    print(f"transposition: largest value difference {np.abs(v - vt).max():.3g}, {(_bits(v) != _bits(vt)).sum()} of 40 values differ in bits")
    assert np.abs(v - vt).max() <= tol_v and np.array_equal(wt[cells], w)
    assert np.abs(gt - np.concatenate([g[c * D:(c + 1) * D] for c in (0, 2, 1, 3)], axis=0)).max() <= tol_g


@pytest.mark.parametrize("with_base", [False, True], ids=["eubo", "nei"])
def test_degenerate_rows_are_the_line(with_base):
    """qt = 2, c01 = c00, c11 = c10: the weights along t are exactly 0 and 1, both grid rows are the line's positions bit for bit, a
    tie goes to the lower index, i.e. to row 0."""
    D = 5
    ref, X, y = make_ref(D)
    t = nr.max_over_points(ref, X)[0] - 0.3 if with_base else None
    rng = np.random.default_rng(6)
    for qs in (2, 3, 8):
        lines = rng.uniform(0, 1, (2 * D, 9))
        patches = np.concatenate([lines, lines], axis=0)
        sets = pr.expand(patches, qs, 2, D)
        assert same(sets[:qs * D], lr.expand(lines, qs, D)) and same(sets[qs * D:], sets[:qs * D])
        lv, lg, lw, _ = lr.line(ref, lines, qs, baseline=t)
        v, g, w, _ = pr.patch(ref, patches, qs, 2, baseline=t)
        assert same(v, lv) and np.array_equal(w[:qs], lw) and np.all(w[qs:] == 0)
        assert same(g[:2 * D], lg) and np.all(g[2 * D:] == 0.0)


def test_guarded_patch_folds_to_zero():
    D, qs, qt = 3, 2, 3
    ref, X, y = make_ref(D)
    patches = np.random.default_rng(8).uniform(0, 1, (4 * D, 5))
    patches[2 * D + 1, 2] = np.nan
    with np.errstate(all="ignore"):
        val, grad, wins, _ = pr.patch(ref, patches, qs, qt)
        vb, gb, _, _ = pr.patch(ref, patches, qs, qt, baseline=np.zeros(S))
    assert val[2] == -1.0e300 and vb[2] == 0.0 and np.all(grad[:, 2] == 0.0) and np.all(gb[:, 2] == 0.0)
    assert np.all(np.isfinite(val[[0, 1, 3, 4]])) and np.all(np.isfinite(grad[:, [0, 1, 3, 4]]))


@pytest.fixture(scope="module")
def runs():
    """(shape, variant) -> (case, lanes run, sequential run) on the CPU objective; each computed once."""
    out = {}
    for i in range(len(pc.PATCHES)):
        case = pc.PatchCase(i)
        ref = ph.PathRef(case.X, case.y, case.theta, case.b, case.kernel, case.n_draws, case.F, case.path_seed)
        evaluate = lambda T, ref=ref, case=case: pr.patch(ref, T, case.qs, case.qt, case.anchor)[:2]
        for v in mc.VARIANTS:
            out[i, v] = (case,) + tuple(lbfgs_ref.run(evaluate, case.starts, mc.N_LOCAL, order=o, **mc.VARIANTS[v])
                                        for o in ("lanes", "sequential"))
    return out


@pytest.mark.parametrize("c", pc.case_ids(), ids=pc.case_name)
def test_at_most_two_percent_of_the_starts_depend_on_the_summation_order(runs, c):
    case, a, b = runs[c]
    scale = np.abs(b["y_stars"]).max()
    apart = np.abs(a["y_stars"] - b["y_stars"]) > 1e-6 * scale
    print(f"{pc.case_name(c)}: {apart.sum()} of {case.S} starts ({apart.mean():.2%}) end more than 1e-6 apart between the two orders; "
          f"evaluations {a['evals_issued']}, live at the end {a['live_at_end']}, ring {a['ring_max'].max()}, "
          f"smallest Armijo margin {a['armijo_margin'].min():.2e}")
    assert apart.mean() <= 0.02
    assert np.all(a["y_stars"] > 0.1 * mc.FLOOR)                        # no start of a case sits at the guard's floor


@pytest.mark.parametrize("k", range(len(pc.RESTATED)))
def test_inputs_of_the_restatement_test_keep_their_winners(k):
    """tests/test_gpu_patch.py compares win counts wherever the restated gap is at least the value tolerance (test_gpu_qeubo.py's):
    at most 5 % of a case's patches may be closer than that."""
    from test_gpu_qeubo import tolerances
    case = pc.RestatedCase(k)
    ref = ph.PathRef(case.X, case.y, case.theta, case.b, case.kernel, case.n_draws, case.F, case.path_seed)
    tol_v, _ = tolerances(ref)
    for wb in case.with_baseline:
        t = nr.max_over_points(ref, case.X)[0] if wb else None
        val, grad, wins, gap = pr.patch(ref, case.patches, case.qs, case.qt, case.anchor, baseline=t)
        close = gap < tol_v
        print(f"case {k}{' with baseline' if wb else ''}: {close.sum()} of {case.M} patches with a gap inside {tol_v:.3g}, "
              f"smallest {gap.min():.3g}")
        assert close.mean() <= 0.05
        assert grad.shape == case.patches.shape and wins.shape == (case.qs * case.qt, case.M)
        if wb:
            assert np.any(val > 0.0)


def test_header_declares_library_exports_and_binding_checks():
    import __graft_entry__ as g
    g.build()
    txt = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = sls()
    lib = m.lib()
    for name in ("sls_patch_eval", "sls_patch_maximize"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in m.EXPORTS
        assert hasattr(lib, name), f"libsls_hip.so does not export {name}"
    assert re.search(r"#define\s+SLS_PATCH_MIN_POSITIONS\s+2\b", code) and m.PATCH_MIN_POSITIONS == 2
    assert re.search(r"#define\s+SLS_QEUBO_MAX_OPTIONS\s+16\b", code) and m.QEUBO_MAX_OPTIONS == 16
    assert '"patch"' in txt
    ps = m.PathSamples.__new__(m.PathSamples)            # refused before anything is allocated or called
    ps.D, ps.n_draws, ps.h = 2, 4, None
    for qs, qt in ((1, 4), (4, 1), (5, 4), (0, 2)):
        with pytest.raises(m.SlsError, match="at most 16 cells"):
            ps.patch_eval(np.zeros((8, 1)), qs, qt)
        with pytest.raises(m.SlsError, match="at most 16 cells"):
            ps.patch_maximize(np.zeros((8, 1)), qs, qt, 3)
    with pytest.raises(m.SlsError, match="4D x M = 8 x M"):
        ps.patch_eval(np.zeros((6, 1)), 2, 2)
    with pytest.raises(m.SlsError, match="3D x M = 6 x M"):
        ps.patch_eval(np.zeros((8, 1)), 2, 2, anchor=np.zeros(2))
    with pytest.raises(m.SlsError, match="4D x M"):
        ps.patch_maximize(np.zeros((4, 1)), 2, 2, 5)
    with pytest.raises(m.SlsError, match="3D x M"):
        ps.patch_maximize(np.zeros((8, 1)), 2, 2, 5, anchor=np.zeros(2))
    with pytest.raises(m.SlsError, match="anchor must hold D = 2"):
        ps.patch_eval(np.zeros((6, 1)), 2, 2, anchor=np.zeros(3))
    with pytest.raises(m.SlsError, match="n_draws = 4"):
        ps.patch_eval(np.zeros((8, 1)), 2, 2, baseline=np.zeros(5))
    with pytest.raises(m.SlsError, match="n_draws = 4"):
        ps.patch_maximize(np.zeros((6, 1)), 2, 2, 5, anchor=np.zeros(2), baseline=np.zeros(3))
