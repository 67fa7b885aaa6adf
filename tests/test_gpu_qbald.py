"""qBALD, the information gain of a q-option choice query on posterior draws, on the MI355X (sls_qbald_eval / sls_qbald_maximize):
agreement with the numpy restatement (tests/qbald_ref.py) in value, gradient, predicted choice probabilities and hard win counts, the
limits of the BTL scale, the bit-level contract (column, other sets, sets per pass, SLS_COMPACT, permuted options), the guard and the
refusals, the neighbours' bits before and after, and the maximiser start by start against tests/lbfgs_ref.py.

The bounds of the agreement test.  Each side forms the values v = f_s(x_i) within B_v of the exact ones and every component of
grad f_s(x_i) within B_g (tests/test_gpu_qlognei.py's tolerances).  With u = B_v / tau and eps = 2 u:
  log p_i = v_i / tau - log sum_j exp(v_j / tau) moves by at most |dv_i| / tau + sum_j p_j |dv_j| / tau <= 2 u = eps, and so does
  log pbar_i (pbar is an average of the p); the bound is stated with the looser d log p <= 2 eps, d log pbar <= 2 eps, d l <= 4 eps;
  KL_s <= ln S (p / pbar <= S), and sum_i p_i |l_i| = KL_s + 2 sum_{l_i < 0} p_i ln(pbar_i / p_i) <= ln S + 2 (ln x <= x - 1), so
  d KL_s = sum_i (dp_i l_i + p_i dl_i), with |dp_i| <= eps p_i, is at most eps (ln S + 2) + 2 eps; the bound allows
  eps (6 + 2 ln S + 2 / e) for it;
  c = p (l - KL) / (S tau):  dc = dp (l - KL) / (S tau) + p (dl - dKL) / (S tau), at most eps |c| + eps (6 + ln S) p / (S tau) to
  first order by the above, and the bound allows 2 eps |c| + eps (10 + 2 ln max(S, 2)) p / (S tau).
Value: sum c dv, at most B_v A with A = sum |c|, and kappa (1 + |value|) for the arithmetic of either side, kappa = (64 + 4 q (1 +
ln max(S, 2))) eps: 64 eps as the other set criteria allow, and 4 eps for each of the q terms of a sum whose terms reach 1 + ln S.
Gradient component: sum c df; the df move by B_g (B_g A), the c as above times |df| <= |grad f|_inf: eps (2 G + (10 + 2 ln max(S, 2))
P) with G = sum |c| |grad f|_inf and P = sum p |grad f|_inf / (S tau); kappa (G + P) for the arithmetic.
prob = pbar: within 2 eps relative, so within 2 eps + kappa absolutely."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import maximize_cases as mc
import path_ref as ph
import qbald_ref as br
import test_gpu_qlognei as ql
from util import sls

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
TAU = 0.05
SCALES = (0.05, 0.01)
CASES = ql.CASES


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def kappa(q, S):
    return (64 + 4 * q * (1 + math.log(max(S, 2)))) * EPS


def bounds(ref, out, q, tau):
    """(value, gradient, prob) bounds per set, as derived in the module's docstring."""
    B_v, B_g = ql.tolerances(ref)
    S = ref.n_draws
    eps, kap = 2 * B_v / tau, kappa(q, S)
    tol_val = B_v * out["A"] + kap * (1 + np.abs(out["val"]))
    tol_grad = B_g * out["A"] + eps * (2 * out["G"] + (10 + 2 * math.log(max(S, 2))) * out["P"]) + kap * (out["G"] + out["P"])
    return tol_val, tol_grad, 2 * eps + kap


def entropy(f):
    with np.errstate(all="ignore"):
        return -np.where(f > 0, f * np.log(f), 0.0).sum(axis=0)


@pytest.mark.parametrize("kernel,N,D,F,q,nd", CASES)
def test_agrees_with_the_restatement(m, ctx, kernel, N, D, F, q, nd):
    gp, ps, ref = ql.setup(m, ctx, kernel, N, D, F, nd)
    B_v, _ = ql.tolerances(ref)
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 300))
    gabs = br.draw_gradient_norms(ref, sets, q)          # once for both scales
    _, qw = ps.qeubo_eval(sets, q, want_grad=False, want_wins=True)
    for tau in SCALES:
        out = br.qbald(ref, sets, q, tau, gabs=gabs)
        tol_val, tol_grad, tol_prob = bounds(ref, out, q, tau)
        val, grad, prob, wins = ps.qbald_eval(sets, q, tau, want_prob=True, want_wins=True)
        assert np.array_equal(wins, qw)                  # the hard wins, bit for bit
        err_v, err_g, err_p = np.abs(val - out["val"]), np.abs(grad - out["grad"]).max(axis=0), np.abs(prob - out["prob"]).max(axis=0)
        print(f"tau {tau}: value error {err_v.max():.3g} = {(err_v / tol_val).max():.3g} of its bound, gradient error {err_g.max():.3g} = "
              f"{(err_g / tol_grad).max():.3g} of its bound ({tol_grad.min():.3g} .. {tol_grad.max():.3g}), prob error {err_p.max():.3g} = "
              f"{err_p.max() / tol_prob:.3g} of its bound; B_v {B_v:.3g}, A {out['A'].min():.3g} .. {out['A'].max():.3g}, value "
              f"{val.min():.3g} .. {val.max():.3g}, |sum prob - 1| <= {np.abs(prob.sum(axis=0) - 1).max() / EPS:.3g} eps")
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
        assert np.all(err_v <= tol_val), (err_v / tol_val).max()
        assert np.all(err_g <= tol_grad), (err_g / tol_grad).max()
        assert np.all(err_p <= tol_prob), err_p.max() / tol_prob
        kap = kappa(q, nd)
        assert np.all(val >= -kap) and np.all(val <= math.log(q) + kap)
        assert np.all(np.abs(prob.sum(axis=0) - 1.0) <= q * EPS)
        if q == 1:
            assert np.all(val == 0.0) and np.all(grad == 0.0) and np.all(prob == 1.0)
        if nd == 1:
            assert np.all(val == 0.0) and np.all(grad == 0.0)
        assert np.array_equal(_bits(ps.qbald_eval(sets, q, tau, want_grad=False)), _bits(val))
    ps.close()
    gp.close()


@pytest.mark.parametrize("case", [0, 3])
def test_limits_of_the_scale(m, ctx, case):
    kernel, N, D, F, q, nd = CASES[case]
    gp, ps, ref = ql.setup(m, ctx, kernel, N, D, F, nd)
    B_v, _ = ql.tolerances(ref)
    sets = np.random.default_rng(1).uniform(0, 1, (q * D, 300))
    kap = kappa(q, nd)
    # a near-deterministic user: one-hot probabilities under every draw.  Premise: the two largest values of every (set, draw) are
    # further apart than both sides' error and than 745 tau, where exp underflows to 0
    gap = br.qbald(ref, sets, q, 1e-9, want_G=False)["gap"].min()
    print(f"smallest gap between the two largest values {gap:.3g}, B_v {B_v:.3g}")
    assert gap > 2 * B_v + 745e-9
    val, grad, prob, wins = ps.qbald_eval(sets, q, 1e-9, want_prob=True, want_wins=True)
    f = wins / nd
    print(f"tau 1e-9: |value - H(wins / S)| <= {np.abs(val - entropy(f)).max():.3g}, |prob - wins / S| <= {np.abs(prob - f).max():.3g}")
    assert np.all(np.abs(val - entropy(f)) <= kap * (1 + math.log(q)))
    assert np.all(np.abs(prob - f) <= 2 * EPS)
    assert np.all(grad == 0.0)
    # a user who answers at random: nothing to learn
    val, prob = ps.qbald_eval(sets, q, 1e6, want_grad=False, want_prob=True)
    print(f"tau 1e6: |value| <= {np.abs(val).max():.3g}, |prob - 1/q| <= {np.abs(prob - 1.0 / q).max():.3g}")
    assert np.all(np.abs(val) <= 1e-12) and np.all(np.abs(prob - 1.0 / q) <= 1e-6)
    # every option the same point
    same = np.tile(sets[:D], (q, 1))
    val, grad, prob = ps.qbald_eval(same, q, TAU, want_prob=True)
    print(f"equal options: |value| <= {np.abs(val).max():.3g}, |prob - 1/q| <= {np.abs(prob - 1.0 / q).max():.3g}, kappa {kap:.3g}")
    assert np.all(np.abs(val) <= kap) and np.all(np.abs(prob - 1.0 / q) <= kap)
    ps.close()
    gp.close()


def test_bit_contract(m, ctx, monkeypatch):
    D, N, F, q, nd, M = 3, 120, 300, 4, 37, 300
    X, y, theta = ql.problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    ref = ph.PathRef(X, y, theta, 0.01, ph.MATERN52, nd, F, seed=42)
    rng = np.random.default_rng(3)
    sets = rng.uniform(0, 1, (q * D, M))
    gabs = br.draw_gradient_norms(ref, sets, q)
    kap = kappa(q, nd)
    ev = lambda s, tau: ps.qbald_eval(s, q, tau, want_prob=True, want_wins=True)

    def same(a, b):
        return all(np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))

    for tau in SCALES:
        full = ev(sets, tau)
        val, grad, prob, wins = full
        assert same(ev(sets, tau), full)
        # a set alone (M = 1), in a block one column into the second tile (M = 129), among others at another column
        assert same(ev(sets[:, 17:18], tau), [a[..., 17:18] for a in full])
        assert same(ev(sets[:, 100:229], tau), [a[..., 100:229] for a in full])
        perm = rng.permutation(M)
        assert same(ev(sets[:, perm], tau), [a[..., perm] for a in full])
        # 256 POINTS per pass = 64 sets, rounded to the 128-set minimum: three passes instead of one
        ctx.set_candidate_chunk(256)
        try:
            chunked = ev(sets, tau)
        finally:
            ctx.set_candidate_chunk(16384)
        assert same(chunked, full)
        # options permuted: wins and prob move with their options exactly; KL_s is a signed sum in index order, so the value and the
        # gradient only to rounding
        order = np.array([2, 0, 3, 1])
        rows = np.concatenate([np.arange(i * D, (i + 1) * D) for i in order])
        vo, go, po, wo = ev(sets[rows], tau)
        out = br.qbald(ref, sets, q, tau, gabs=gabs)
        dv, dg = np.abs(vo - val) / (kap * (1 + np.abs(val))), np.abs(go - grad[rows]).max(axis=0) / (kap * (out["G"] + out["P"]))
        print(f"tau {tau}, permuted options: value moves by {dv.max():.3g} of its bound, gradient by {dg.max():.3g}")
        assert np.array_equal(wo, wins[order]) and np.array_equal(_bits(po), _bits(prob[order]))
        assert np.all(dv <= 1.0) and np.all(dg <= 1.0)
    # the maximiser with and without compaction of the live columns: a set meets other neighbours, the bits stay
    starts = rng.uniform(0, 1, (q * D, 150))
    res = {}
    val, grad = ps.qbald_eval(sets, q, TAU)
    for flag in ("1", "0"):
        monkeypatch.setenv("SLS_COMPACT", flag)
        vf, gf = ps.qbald_eval(sets, q, TAU)
        assert np.array_equal(_bits(vf), _bits(val)) and np.array_equal(_bits(gf), _bits(grad)), flag
        res[flag] = ps.qbald_maximize(starts, q, 12, TAU, opts=m.LbfgsOpts(ftol_rel=1e-3, xtol_rel=1e-3))
        res[flag]["stats"] = gp.last_stats()
    monkeypatch.delenv("SLS_COMPACT")
    for k in ("x", "x_stars", "y_stars"):
        assert np.array_equal(_bits(res["1"][k]), _bits(res["0"][k])), k
    assert res["1"]["index"] == res["0"]["index"] and res["1"]["value"] == res["0"]["value"]
    assert res["1"]["stats"]["evals_issued"] < res["1"]["stats"]["evals_cap"]     # starts did leave the batch
    ps.close()
    gp.close()


def test_guard_and_refusals(m, ctx):
    D, N, F, q, nd = 3, 120, 300, 3, 20
    X, y, theta = ql.problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    for M, bad in ((3, [1]), (300, [0, 130, 299])):
        sets = np.random.default_rng(5).uniform(0, 1, (q * D, M))
        val, grad, prob, wins = ps.qbald_eval(sets, q, TAU, want_prob=True, want_wins=True)
        hit = sets.copy()
        for k, n in enumerate(bad):
            hit[(k % q) * D + 1, n] = np.nan                       # another option each time
        v, g, p, w = ps.qbald_eval(hit, q, TAU, want_prob=True, want_wins=True)
        _, qw = ps.qeubo_eval(hit, q, want_grad=False, want_wins=True)
        good = np.setdiff1d(np.arange(M), bad)
        assert np.all(v[bad] == m.QEUBO_FLOOR) and np.all(g[:, bad] == 0.0) and np.all(p[:, bad] == 0.0)
        assert np.array_equal(w, qw)                               # wins as sls_qeubo_eval reports them, the hit sets included
        assert np.array_equal(_bits(v[good]), _bits(val[good])) and np.array_equal(_bits(g[:, good]), _bits(grad[:, good]))
        assert np.array_equal(_bits(p[:, good]), _bits(prob[:, good])) and np.array_equal(w[:, good], wins[:, good])
        assert np.array_equal(_bits(ps.qbald_eval(hit, q, TAU, want_grad=False)), _bits(v))
    M = 3
    sets = np.random.default_rng(5).uniform(0, 1, (q * D, M))
    full = ps.qbald_eval(sets, q, TAU, want_prob=True, want_wins=True)
    lib, dp, ip = m.lib(), C.POINTER(C.c_double), C.POINTER(C.c_int)
    F_sets, val3 = np.asfortranarray(sets), np.empty(M)
    x, v1, idx = np.empty(q * D), C.c_double(), C.c_long()
    p = lambda a: a.ctypes.data_as(dp)

    def ev(scale, M=M):
        return lib.sls_qbald_eval(ps.h, q, C.c_double(scale), p(F_sets), M, p(val3), None, None, None)

    def mx(scale):
        return lib.sls_qbald_maximize(ps.h, q, C.c_double(scale), p(F_sets), M, 4, None, C.c_long(0), p(x), C.byref(v1), C.byref(idx), None,
                                      None)

    for bad in (float("nan"), 0.0, -1.0, float("inf"), 5e-324):
        assert ev(bad) == -1 and "scale" in lib.sls_last_error().decode()
        assert mx(bad) == -1 and "scale" in lib.sls_last_error().decode()
    val3[:] = 7.0
    assert ev(TAU, M=0) == 0 and np.all(val3 == 7.0)                  # M = 0: nothing to do
    assert ev(TAU) == 0 and np.array_equal(_bits(val3), _bits(full[0]))   # the context stays usable
    assert mx(TAU) == 0 and np.isfinite(v1.value)
    # every subset of NULL outputs: the outputs that remain keep their bits
    for keep in itertools.product((False, True), repeat=4):
        bufs = [np.empty(M), np.empty((q * D, M), order="F"), np.empty((q, M), order="F"), np.zeros((q, M), dtype=np.int32, order="F")]
        args = [(b.ctypes.data_as(ip) if b.dtype == np.int32 else p(b)) if k else None for b, k in zip(bufs, keep)]
        assert lib.sls_qbald_eval(ps.h, q, C.c_double(TAU), p(F_sets), M, *args) == 0
        for b, k, want in zip(bufs, keep, full):
            assert not k or b.tobytes(order="F") == want.tobytes(order="F"), keep
    ps.close()
    gp.close()


def test_neighbours_keep_their_bits(m, ctx):
    """qEUBO, qNEI and qLogNEI on a path handle before and after qBALD calls on it."""
    D, N, F, q, nd, M = 3, 120, 300, 4, 37, 200
    X, y, theta = ql.problem(D, N, seed=31)
    gp = m.GP(ctx, X, y, theta, 0.01, ph.MATERN52)
    ps = m.PathSamples(gp, nd, F, seed=42)
    t, _ = ps.max_over_points(X)
    sets = np.random.default_rng(9).uniform(0, 1, (q * D, M))
    others = lambda: (ps.qeubo_eval(sets, q, want_wins=True) + ps.qnei_eval(sets, q, t, want_wins=True) +
                      ps.qlognei_eval(sets, q, t, *ql.TAU, want_wins=True))
    before = others()
    ps.qbald_eval(sets, q, TAU, want_prob=True, want_wins=True)
    ps.qbald_eval(sets, q)
    ps.qbald_maximize(sets[:, :20], q, 3, TAU)
    after = others()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes(order="F") == b.tobytes(order="F")
    ps.close()
    gp.close()


@pytest.mark.parametrize("variant", list(mc.VARIANTS))
def test_maximiser_against_the_restated_lbfgs(m, ctx, variant):
    """tests/test_gpu_maximize_restated.py's smallest qNEI shape (q = 3, D = 5), its starts and its comparison rule, with the device's
    own sls_qbald_eval as the restated run's objective."""
    case = mc.Case("qnei", 0)
    q = case.shape["q"]
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    kw = mc.VARIANTS[variant]
    rg = ps.qbald_maximize(case.starts, q, mc.N_LOCAL, TAU, opts=m.LbfgsOpts(**kw) if kw else None)
    st = gp.last_stats()
    rr = mc.restated(lambda T: ps.qbald_eval(T, q, TAU), case, kw)
    mc.hold_to_restatement(rg, rr, f"qbald-q{q}-D{case.D}-{variant}", stats=st)
    assert (rr["evals"] > 1).all()                       # at this scale no start is stationary
    ps.close()
    gp.close()


def test_maximiser_above_128_columns(m, ctx):
    """maximize_cases.WIDE's set case, q = 2 and D = 129: 258 variables."""
    i = len(mc.ROUTES["qeubo"]) - 1
    case = mc.Case("qeubo", i)
    assert case.shape == mc.WIDE["qeubo"][0] and case.nvar > 128
    q = case.shape["q"]
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    rg = ps.qbald_maximize(case.starts, q, mc.N_LOCAL, TAU)
    st = gp.last_stats()
    rr = mc.restated(lambda T: ps.qbald_eval(T, q, TAU), case, {})
    mc.hold_to_restatement(rg, rr, f"qbald-q{q}-D{case.D}-default", stats=st)
    ps.close()
    gp.close()
