"""qLogNEI, log-space noisy expected improvement of q points on posterior draws, on the MI355X (sls_qlognei_terms /
sls_qlognei_eval / sls_qlognei_maximize): the scalar terms against 50-digit values, agreement with the numpy restatement
(tests/qlognei_ref.py) in value, gradient and hard win counts, the sandwich against the device's own qNEI at the default
temperatures, the bit-level contract (column, other sets, sets per pass, SLS_COMPACT), a set no draw improves, the guard and the
refusals, the neighbours' bits before and after, the maximiser start by start against tests/lbfgs_ref.py, and the maximiser leaving
starts where qNEI is exactly 0 (tests/qlognei_cases.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import maximize_cases as mc
import path_ref as ph
import qlognei_cases as qc
import qlognei_ref as lr
from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
TAU = (0.05, 0.05)
DEFAULT = (1e-6, 1e-2)


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
    """tests/test_gpu_qeubo.py's bounds on one value f_s(x) and one gradient component of it (B_v, B_g)."""
    ev = np.linalg.eigvalsh(ref.Ky)
    cond = ev[-1] / ev[0]
    vs = np.abs(ref.v).max()
    tol_v = 1e-10 * ref.a + 4 * cond * EPS * vs * ref.a * np.sqrt(ref.N)
    tol_g = 1e-9 * ref.a + 4 * cond * EPS * vs * ref.a * np.sqrt(ref.N) / ref.ell.min()
    return tol_v, tol_g


def bounds(ref, out, tau0, taum):
    """Per set: the value moves by at most sum c B_v = A B_v with the values (c = d value / d v); a gradient component is sum c df: the
    df move by B_g (A B_g), and c = omega pi rho moves, to first order and relative to itself, by at most 2 rho_max B_v (omega), (2 /
    taum) rho_max B_v (pi) and (2 / tau0) B_v (rho: |R'/R| <= 2) -- times G = sum c |df|.  64 eps for the arithmetic of either side."""
    B_v, B_g = tolerances(ref)
    tol_val = B_v * out["A"] + 64 * EPS * (1 + np.abs(out["val"]))
    tol_grad = B_g * out["A"] + out["G"] * B_v * (out["rho_max"] * (2 + 2 / taum) + 2 / tau0) + 64 * EPS * out["G"]
    return tol_val, tol_grad


def setup(m, ctx, kernel, N, D, F, nd, b=0.05):
    X, y, theta = problem(D, N, seed=N + D + F, ell=0.3 * np.sqrt(D))
    gp = m.GP(ctx, X, y, theta, b, kernel)
    ps = m.PathSamples(gp, nd, F, seed=1234 + D)
    ref = ph.PathRef(X, y, theta, b, kernel, nd, F, seed=1234 + D)
    return gp, ps, ref


def test_scalar_terms_against_50_digit_values(ctx):
    """16 eps: three library calls of at most 2 ulp each and a log of a quantity that carries 3 eps."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "qlognei_terms.npz"))
    a, L, R = z["a"], z["L"], z["R"]
    assert a.size % 256 != 0
    gL, gR = ctx.qlognei_terms(a)
    eL, eR = np.abs(gL - L) / (EPS * (1 + np.abs(L))), np.abs(gR - R) / (EPS * R)
    print(f"L within {eL.max():.3g} eps (1 + |L|) at a = {a[np.argmax(eL)]!r}, R within {eR.max():.3g} eps at a = {a[np.argmax(eR)]!r}")
    assert np.all(np.isfinite(gL)) and np.all(gR > 0)
    assert eL.max() <= 16 and eR.max() <= 16
    for n in (1, 257):                                   # one element; one element into the second block
        l1, r1 = ctx.qlognei_terms(a[:n])
        assert np.array_equal(_bits(l1), _bits(gL[:n])) and np.array_equal(_bits(r1), _bits(gR[:n]))
    lib, dp = sls().lib(), C.POINTER(C.c_double)         # either output may be NULL
    only = np.empty(a.size)
    assert lib.sls_qlognei_terms(ctx.h, a.ctypes.data_as(dp), C.c_long(a.size), None, only.ctypes.data_as(dp)) == 0
    assert np.array_equal(_bits(only), _bits(gR))


# tests/test_gpu_qeubo.py's four cases, then 16 points on one draw and one point on 130 draws
CASES = [(ph.SE, 90, 2, 100, 3, 64), (ph.MATERN52, 90, 16, 1024, 4, 64), (ph.SE, 300, 96, 700, 2, 37), (ph.MATERN52, 700, 7, 300, 5, 130),
         (ph.SE, 90, 2, 100, 16, 1), (ph.MATERN52, 90, 2, 100, 16, 1), (ph.SE, 90, 2, 100, 1, 130), (ph.MATERN52, 90, 2, 100, 1, 130),
         # D > 128 (tests/test_gpu_qeubo.py's two): the only check of this criterion's gradient above 128 columns
         (ph.SE, 90, 129, 100, 2, 37), (ph.MATERN52, 130, 257, 300, 4, 37)]


@pytest.mark.parametrize("kernel,N,D,F,q,nd", CASES)
def test_agrees_with_the_restatement(m, ctx, kernel, N, D, F, q, nd):
    gp, ps, ref = setup(m, ctx, kernel, N, D, F, nd)
    B_v, _ = tolerances(ref)
    t, _ = ps.max_over_points(ref.X)                     # the baseline the device formed, on both sides
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 300))
    out = lr.qlognei(ref, sets, q, t, *TAU)
    tol_val, tol_grad = bounds(ref, out, *TAU)
    val, grad, wins = ps.qlognei_eval(sets, q, t, *TAU, want_wins=True)
    nv, nw = ps.qnei_eval(sets, q, t, want_grad=False, want_wins=True)
    assert np.array_equal(wins, nw)                      # the hard wins, bit for bit
    err_v, err_g = np.abs(val - out["val"]), np.abs(grad - out["grad"]).max(axis=0)
    print(f"value error {err_v.max():.3g} = {(err_v / tol_val).max():.3g} of its bound (bounds {tol_val.min():.3g} .. {tol_val.max():.3g}), "
          f"gradient error {err_g.max():.3g} = {(err_g / tol_grad).max():.3g} of its bound ({tol_grad.min():.3g} .. {tol_grad.max():.3g}); "
          f"B_v {B_v:.3g}, A {out['A'].min():.3g} .. {out['A'].max():.3g}, rho_max {out['rho_max'].max():.3g}")
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    assert np.all(err_v <= tol_val), (err_v / tol_val).max()
    assert np.all(err_g <= tol_grad), (err_g / tol_grad).max()
    assert np.array_equal(_bits(ps.qlognei_eval(sets, q, t, *TAU, want_grad=False)), _bits(val))
    # the default temperatures: finite, and between the bounds the device's own qNEI gives.  Both sides are functions of the same
    # values, qNEI with Lipschitz constant 1 and exp(value) with q^taum in the maximum norm, and each side's values carry B_v.
    dv, dg = ps.qlognei_eval(sets, q, t)
    assert np.all(np.isfinite(dv)) and np.all(np.isfinite(dg)) and np.all(np.abs(dg).max(axis=0) > 0)
    tau0, taum = DEFAULT
    ev, hi = np.exp(dv), q ** taum * (nv + tau0 * math.log(2.0))
    slack = 2 * q ** taum * B_v
    print(f"default temperatures: {np.mean(nv == 0.0):.2f} of the sets have qNEI 0; exp(value) - qNEI >= {(ev - nv).min():.3g}, "
          f"upper bound - exp(value) >= {(hi - ev).min():.3g}, slack {slack:.3g}")
    assert np.all(ev >= nv * (1 - 1e-12) - slack) and np.all(ev <= hi * (1 + 1e-12) + slack)
    ps.close()
    gp.close()


def test_bit_contract(m, ctx, monkeypatch):
    D, N, F, q, nd, M = 3, 120, 300, 4, 37, 300
    X, y, theta = problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    t, _ = ps.max_over_points(X)
    rng = np.random.default_rng(3)
    sets = rng.uniform(0, 1, (q * D, M))
    for taus in (TAU, DEFAULT):
        val, grad, wins = ps.qlognei_eval(sets, q, t, *taus, want_wins=True)
        v2, g2, w2 = ps.qlognei_eval(sets, q, t, *taus, want_wins=True)
        assert np.array_equal(_bits(val), _bits(v2)) and np.array_equal(_bits(grad), _bits(g2)) and np.array_equal(wins, w2)
        # a set alone (M = 1), in a block one column into the second tile (M = 129), among others at another column
        v1, g1, w1 = ps.qlognei_eval(sets[:, 17:18], q, t, *taus, want_wins=True)
        assert _bits(v1)[0] == _bits(val)[17] and np.array_equal(_bits(g1[:, 0]), _bits(grad[:, 17])) and np.array_equal(w1[:, 0], wins[:, 17])
        va, ga, wa = ps.qlognei_eval(sets[:, 100:229], q, t, *taus, want_wins=True)
        assert np.array_equal(_bits(va), _bits(val[100:229])) and np.array_equal(_bits(ga), _bits(grad[:, 100:229]))
        assert np.array_equal(wa, wins[:, 100:229])
        perm = rng.permutation(M)
        vp, gp_, wp = ps.qlognei_eval(sets[:, perm], q, t, *taus, want_wins=True)
        assert np.array_equal(_bits(vp), _bits(val[perm])) and np.array_equal(_bits(gp_), _bits(grad[:, perm]))
        assert np.array_equal(wp, wins[:, perm])
        # 256 POINTS per pass = 64 sets, rounded to the 128-set minimum: three passes instead of one
        ctx.set_candidate_chunk(256)
        try:
            vc, gc, wc = ps.qlognei_eval(sets, q, t, *taus, want_wins=True)
        finally:
            ctx.set_candidate_chunk(16384)
        assert np.array_equal(_bits(vc), _bits(val)) and np.array_equal(_bits(gc), _bits(grad)) and np.array_equal(wc, wins)
        # options permuted: wins and gradient blocks move with their options exactly, the value to rounding
        order = np.array([2, 0, 3, 1])
        rows = np.concatenate([np.arange(i * D, (i + 1) * D) for i in order])
        vo, go, wo = ps.qlognei_eval(sets[rows], q, t, *taus, want_wins=True)
        assert np.array_equal(wo, wins[order]) and np.array_equal(_bits(go), _bits(grad[rows]))
        assert np.all(np.abs(vo - val) <= 8 * EPS * (1 + np.abs(val)))
    # the maximiser with and without compaction of the live columns: a set meets other neighbours, the bits stay
    starts = rng.uniform(0, 1, (q * D, 150))
    res = {}
    val, grad = ps.qlognei_eval(sets, q, t, *TAU)
    for flag in ("1", "0"):
        monkeypatch.setenv("SLS_COMPACT", flag)
        vf, gf = ps.qlognei_eval(sets, q, t, *TAU)
        assert np.array_equal(_bits(vf), _bits(val)) and np.array_equal(_bits(gf), _bits(grad)), flag
        res[flag] = ps.qlognei_maximize(starts, q, 12, t, *TAU, opts=m.LbfgsOpts(ftol_rel=1e-3, xtol_rel=1e-3))
        res[flag]["stats"] = gp.last_stats()
    monkeypatch.delenv("SLS_COMPACT")
    for k in ("x", "x_stars", "y_stars"):
        assert np.array_equal(_bits(res["1"][k]), _bits(res["0"][k])), k
    assert res["1"]["index"] == res["0"]["index"] and res["1"]["value"] == res["0"]["value"]
    assert res["1"]["stats"]["evals_issued"] < res["1"]["stats"]["evals_cap"]     # starts did leave the batch
    ps.close()
    gp.close()


def test_a_set_no_draw_improves(m, ctx):
    kernel, N, D, F, q, nd = CASES[0]
    gp, ps, ref = setup(m, ctx, kernel, N, D, F, nd)
    B_v, _ = tolerances(ref)
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 300))
    t, _ = ps.max_over_points(ref.X)
    high = np.full(nd, 1.0e3)
    nv, ng, nw = ps.qnei_eval(sets, q, high, want_wins=True)
    assert np.all(nv == 0.0) and not np.any(np.signbit(nv)) and np.all(ng == 0.0) and np.all(nw == 0)
    for taus in (TAU, DEFAULT):
        out = lr.qlognei(ref, sets, q, high, *taus)
        tol_val, tol_grad = bounds(ref, out, *taus)
        val, grad, wins = ps.qlognei_eval(sets, q, high, *taus, want_wins=True)
        err_v, err_g = np.abs(val - out["val"]), np.abs(grad - out["grad"]).max(axis=0)
        print(f"taus {taus}: value {val.min():.6g} .. {val.max():.6g}, error {(err_v / tol_val).max():.3g} of its bound, gradient error "
              f"{(err_g / tol_grad).max():.3g} of its bound")
        assert np.all(np.isfinite(val)) and np.all(wins == 0)
        assert np.all(err_v <= tol_val) and np.all(err_g <= tol_grad)
        # every point's block is nonzero wherever its weights are (in double the weights of a point far below the set's best
        # underflow: the restatement says where)
        alive = out["c"].sum(axis=2) > 0                                         # q x M
        blocks = np.abs(grad.reshape(q, D, -1)).max(axis=1) > 0
        assert np.all(blocks.any(axis=0)) and np.all(blocks[alive])
        if taus == TAU:
            assert np.all(blocks)
    # a baseline far below every value: within the sandwich of qNEI's
    low = t - 1.0e3
    nv = ps.qnei_eval(sets, q, low, want_grad=False)
    for tau0, taum in (TAU, DEFAULT):
        ev = np.exp(ps.qlognei_eval(sets, q, low, tau0, taum, want_grad=False))
        hi = q ** taum * (nv + tau0 * math.log(2.0))
        slack = 2 * q ** taum * B_v
        assert np.all(ev >= nv * (1 - 1e-12) - slack) and np.all(ev <= hi * (1 + 1e-12) + slack)
    ps.close()
    gp.close()


def test_guard_and_refusals(m, ctx):
    D, N, F, q, nd = 3, 120, 300, 3, 20
    X, y, theta = problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    t, _ = ps.max_over_points(X)
    for M, bad in ((3, [1]), (300, [0, 130, 299])):
        sets = np.random.default_rng(5).uniform(0, 1, (q * D, M))
        val, grad, wins = ps.qlognei_eval(sets, q, t, *TAU, want_wins=True)
        hit = sets.copy()
        for k, n in enumerate(bad):
            hit[(k % q) * D + 1, n] = np.nan                       # another option each time
        v, g, w = ps.qlognei_eval(hit, q, t, *TAU, want_wins=True)
        good = np.setdiff1d(np.arange(M), bad)
        assert np.all(v[bad] == m.QEUBO_FLOOR) and np.all(g[:, bad] == 0.0)
        assert np.array_equal(_bits(v[good]), _bits(val[good])) and np.array_equal(_bits(g[:, good]), _bits(grad[:, good]))
        assert np.array_equal(w[:, good], wins[:, good])
        assert np.array_equal(_bits(ps.qlognei_eval(hit, q, t, *TAU, want_grad=False)), _bits(v))
    sets = np.random.default_rng(5).uniform(0, 1, (q * D, 3))
    want = ps.qlognei_eval(sets, q, t, *TAU, want_grad=False)
    lib, dp = m.lib(), C.POINTER(C.c_double)
    F_sets, val3 = np.asfortranarray(sets), np.empty(3)
    x, v1, idx = np.empty(q * D), C.c_double(), C.c_long()
    p = lambda a: a.ctypes.data_as(dp)

    def ev(tb, t0, tm, M=3):
        return lib.sls_qlognei_eval(ps.h, q, p(tb), C.c_double(t0), C.c_double(tm), p(F_sets), M, p(val3), None, None)

    def mx(tb, t0, tm):
        return lib.sls_qlognei_maximize(ps.h, q, p(tb), C.c_double(t0), C.c_double(tm), p(F_sets), 3, 4, None, C.c_long(0), p(x),
                                        C.byref(v1), C.byref(idx), None, None)

    for bad in (float("nan"), 0.0, -1.0, float("inf")):
        assert ev(t, bad, 0.05) == -1 and "tau_relu" in lib.sls_last_error().decode()
        assert ev(t, 0.05, bad) == -1 and "tau_max" in lib.sls_last_error().decode()
        assert mx(t, bad, 0.05) == -1 and mx(t, 0.05, bad) == -1
    for poison in (np.nan, np.inf, -np.inf):
        tb = t.copy()
        tb[nd - 1] = poison
        assert ev(tb, 0.05, 0.05) == -1 and "not finite" in lib.sls_last_error().decode()
        assert mx(tb, 0.05, 0.05) == -1
    val3[:] = 7.0
    assert ev(t, 0.05, 0.05, M=0) == 0 and np.all(val3 == 7.0)        # M = 0: nothing to do
    assert ev(t, 0.05, 0.05) == 0 and np.array_equal(_bits(val3), _bits(want))   # the context stays usable
    assert mx(t, 0.05, 0.05) == 0 and np.isfinite(v1.value)
    ps.close()
    gp.close()


def test_neighbours_keep_their_bits(m, ctx):
    """qEUBO and qNEI on a path handle before and after a qLogNEI evaluation on it."""
    D, N, F, q, nd, M = 3, 120, 300, 4, 37, 200
    X, y, theta = problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    t, _ = ps.max_over_points(X)
    sets = np.random.default_rng(9).uniform(0, 1, (q * D, M))
    before = ps.qeubo_eval(sets, q, want_wins=True) + ps.qnei_eval(sets, q, t, want_wins=True)
    ps.qlognei_eval(sets, q, t, *TAU, want_wins=True)
    ps.qlognei_eval(sets, q, t)
    after = ps.qeubo_eval(sets, q, want_wins=True) + ps.qnei_eval(sets, q, t, want_wins=True)
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes(order="F") == b.tobytes(order="F")
    ps.close()
    gp.close()


@pytest.mark.parametrize("variant", list(mc.VARIANTS))
def test_maximiser_against_the_restated_lbfgs(m, ctx, variant):
    """tests/test_gpu_maximize_restated.py's smallest qNEI shape (q = 3, D = 5), its starts and its comparison rule, with the device's
    own sls_qlognei_eval as the restated run's objective."""
    case = mc.Case("qnei", 0)
    q = case.shape["q"]
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    t, _ = ps.max_over_points(case.X)
    kw = mc.VARIANTS[variant]
    rg = ps.qlognei_maximize(case.starts, q, mc.N_LOCAL, t, *TAU, opts=m.LbfgsOpts(**kw) if kw else None)
    st = gp.last_stats()
    rr = mc.restated(lambda T: ps.qlognei_eval(T, q, t, *TAU), case, kw)
    mc.hold_to_restatement(rg, rr, f"qlognei-q{q}-D{case.D}-{variant}", stats=st)
    assert (rr["evals"][case.dead] > 1).all()            # the starts qNEI leaves at once move here
    ps.close()
    gp.close()


def test_maximiser_leaves_starts_where_qnei_is_zero(m, ctx):
    """tests/qlognei_cases.py: the starts ESC_ASSERTED have qNEI exactly 0 (every value 1e-3 or more below the baseline).
    sls_qnei_maximize returns them unmoved with the value 0; sls_qlognei_maximize at the default temperatures ends them where the
    device's qNEI is positive."""
    e = qc.escape_case()
    q, starts, t, idx = qc.ESC_Q, e["starts"], e["t"], qc.ESC_ASSERTED
    gp = m.GP(ctx, e["X"], e["y"], e["theta"], e["b"], e["kernel"])
    ps = m.PathSamples(gp, qc.ESC_DRAWS, qc.ESC_F, seed=qc.ESC_PATH_SEED)
    v0, g0 = ps.qnei_eval(starts[:, idx], q, t)
    assert np.all(v0 == 0.0) and np.all(g0 == 0.0)
    rn = ps.qnei_maximize(starts, q, qc.ESC_N_LOCAL, t)
    assert np.array_equal(rn["x_stars"][:, idx], starts[:, idx]) and np.all(rn["y_stars"][idx] == 0.0)
    rl = ps.qlognei_maximize(starts, q, qc.ESC_N_LOCAL, t, *qc.ESC_TAUS)
    after = ps.qnei_eval(rl["x_stars"], q, t, want_grad=False)
    print("qNEI at the ends of the asserted starts:", after[idx])
    assert np.all(after[idx] > 0.0)
    assert np.all(after[idx] >= qc.ESC_MARGIN)           # the CPU run's 6.28e-3, not a revived rounding error
    assert np.all((rl["x_stars"] >= 0.0) & (rl["x_stars"] <= 1.0))
    ps.close()
    gp.close()
