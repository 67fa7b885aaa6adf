"""The search over affine subspaces (sls_*_sub; include/sls_hip.h "maximisation over affine subspaces") on the device.

A column with map k stands for the point x = c_k + A_k z; two kernels (csrc/kernels_sub.hip) expand z into x in front of the
unchanged evaluation and fold its gradient back onto z.  So everything here is stated in BITS against the plain calls and the numpy
restatement of the two kernels (tests/subspace_ref.py), and the maximisers are held, start by start, to tests/lbfgs_ref.py driven
by the device's own *_eval_sub (tests/maximize_cases.py: hold_to_restatement with z_stars in the place of x_stars).  The cases and
the CPU check that they are not sensitive to the summation order are in tests/subspace_cases.py / tests/test_subspace_cpu.py.
The _sub routes always take the tiled evaluation: wherever a plain call is the comparison, SLS_WAVE_PATH=0 makes it take it too."""
import numpy as np
import pytest

import maximize_cases as mc
import subspace_cases as sc
import subspace_ref as sr
from util import sls

pytestmark = pytest.mark.gpu
N_LOCAL = mc.N_LOCAL
M_EVAL = 300
N_DRAWS, PER_DRAW, N_FREQ = 3, 50, 256


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def opts_of(m, variant):
    kw = mc.VARIANTS[variant]
    return m.LbfgsOpts(**kw) if kw else None


def y_star_of(case):
    return case.y.max() + np.array([0.1, 0.25, 0.6])


class Routes:
    """The five evaluation routes of one handle, each as (plain eval at X, eval_sub at (maps, Z), maximize_sub at (maps, starts))."""

    def __init__(self, m, ctx, case, with_path=True):
        self.m, self.case = m, case
        self.gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
        self.ps = m.PathSamples(self.gp, N_DRAWS, N_FREQ, seed=1234 + case.D) if with_path else None
        self.y_star = y_star_of(case)

    def close(self):
        if self.ps is not None:
            self.ps.close()
        self.gp.close()

    def plain(self, route, X, draws=None, want_grad=True):
        gp = self.gp
        if route == "mes":
            return gp.mes_eval(self.y_star, X, want_grad=want_grad)
        if route == "path":
            return self.ps.eval(X, draws, want_grad=want_grad)
        return gp.acq_eval(X, dict(ei=mc.EI, ucb=mc.UCB, logei=mc.LOG_EI)[route], mc.UCB_H, want_grad=want_grad)

    def sub(self, route, maps, Z, draws=None, **kw):
        gp = self.gp
        if route == "mes":
            return gp.mes_eval_sub(self.y_star, maps, Z, **kw)
        if route == "path":
            return self.ps.eval_sub(maps, Z, draws, **kw)
        return gp.acq_eval_sub(maps, Z, dict(ei=mc.EI, ucb=mc.UCB, logei=mc.LOG_EI)[route], mc.UCB_H, **kw)

    def maximize_sub(self, route, maps, starts, **kw):
        gp = self.gp
        if route == "mes":
            return gp.mes_maximize_sub(self.y_star, maps, starts, N_LOCAL, **kw)
        return gp.acq_maximize_sub(maps, starts, N_LOCAL, dict(ei=mc.EI, ucb=mc.UCB, logei=mc.LOG_EI)[route], mc.UCB_H, **kw)


HANDLE_ROUTES = ("ei", "ucb", "logei", "mes")
EVAL_ROUTES = HANDLE_ROUTES + ("path",)


# ---- 1. evaluation: bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", (0, 3, 5, 6), ids=sc.shape_name)
def test_eval_sub_is_the_plain_evaluation_between_the_restated_expand_and_fold(m, ctx, monkeypatch, i):
    monkeypatch.setenv("SLS_WAVE_PATH", "0")
    case = sc.SubCase(i)
    Z, k = case.eval_points(M_EVAL, 20 + i)
    draws = np.random.default_rng(30 + i).integers(0, N_DRAWS, M_EVAL)
    maps = m.SubMaps(case.A, case.c, k)
    X_ref = sr.expand(case.A, case.c, k, Z)
    r = Routes(m, ctx, case)
    for route in EVAL_ROUTES:
        val, gz, X = r.sub(route, maps, Z, draws, want_x=True)
        assert same_bits(X, X_ref), f"{route}: X_out is not the contract's expand"
        pv, pg = r.plain(route, X, draws)
        assert same_bits(val, pv), f"{route}: {np.count_nonzero(bits(val) != bits(pv))} of {M_EVAL} values differ from the plain call at X_out"
        assert same_bits(gz, sr.fold(case.A, case.c, k, pg)), f"{route}: grad_z is not the contract's fold of the plain gradient"
        assert np.isfinite(val).all() and np.isfinite(gz).all()
        # without a gradient: the plain call's value-only evaluation (it may take another contraction than the one with a gradient)
        assert same_bits(r.sub(route, maps, Z, draws, want_grad=False), r.plain(route, X, draws, want_grad=False)), f"{route}: value only"
    r.close()


# ---- 2. column independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", (3, 6), ids=sc.shape_name)
def test_a_points_bits_depend_on_its_own_variables_and_its_own_map_alone(m, ctx, i):
    case = sc.SubCase(i)
    Z, k = case.eval_points(M_EVAL, 20 + i)
    draws = np.random.default_rng(30 + i).integers(0, N_DRAWS, M_EVAL)
    r = Routes(m, ctx, case)
    perm = np.random.default_rng(70 + i).permutation(M_EVAL)
    for route in EVAL_ROUTES:
        val, gz, X = r.sub(route, m.SubMaps(case.A, case.c, k), Z, draws, want_x=True)
        # another column, other neighbours
        v2, g2, X2 = r.sub(route, m.SubMaps(case.A, case.c, k[perm]), Z[:, perm], draws[perm], want_x=True)
        assert same_bits(v2, val[perm]) and same_bits(g2, gz[:, perm]) and same_bits(X2, X[:, perm]), route
        # alone, with its own map as the only map of the call
        for j in (0, 127, 128, M_EVAL - 1):
            v1, g1, X1 = r.sub(route, m.SubMaps(case.A[k[j]], case.c[k[j]]), Z[:, j:j + 1], draws[j:j + 1], want_x=True)
            assert same_bits(v1, val[j:j + 1]) and same_bits(g1, gz[:, j:j + 1]) and same_bits(X1, X[:, j:j + 1]), (route, j)
    r.close()


@pytest.mark.parametrize("i", (1, 7), ids=sc.shape_name)
def test_compaction_does_not_change_a_bit(m, ctx, monkeypatch, i):
    case = sc.SubCase(i)
    maps = m.SubMaps(case.A, case.c, case.map_of_start)
    r = Routes(m, ctx, case, with_path=False)
    route = "ei" if case.acq == mc.EI else "ucb"
    out = {}
    for compact in ("1", "0"):
        monkeypatch.setenv("SLS_COMPACT", compact)
        out[compact] = r.maximize_sub(route, maps, case.starts)
    for key in ("z_stars", "y_stars", "x_stars", "z", "x"):
        assert same_bits(out["0"][key], out["1"][key]), key
    assert out["0"]["index"] == out["1"]["index"] and out["0"]["value"] == out["1"]["value"]
    r.close()


# ---- 3. the identity map ------------------------------------------------------------------------------------------------------------------
def identity_maps(m, D, kind):
    if kind == "identity":
        return m.SubMaps(np.eye(D), np.zeros(D))
    A, c = sc.box_maps(np.full((D, 1), 0.5), 1, half=1.0)   # Box(0, 1): lo = 0, hi = 1
    assert np.array_equal(A[0], np.eye(D)) and not c.any()
    return m.SubMaps(A, c, np.zeros(129, dtype=np.int32))


@pytest.mark.parametrize("kind", ("identity", "box01"))
@pytest.mark.parametrize("route", HANDLE_ROUTES)
def test_identity_map_is_the_plain_maximiser(m, ctx, monkeypatch, route, kind):
    """d = D, A = I, c = 0 on the harness shape (N = 600, D = 5, tiled evaluation): the same y_stars to the bit, the same points (only
    the sign of a zero may differ: x = 0 + 1 z), the same statistics."""
    monkeypatch.setenv("SLS_WAVE_PATH", "0")
    case = mc.Case("harness", 0)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    y_star = y_star_of(case)
    acq = dict(ei=mc.EI, ucb=mc.UCB, logei=mc.LOG_EI).get(route)
    maps = identity_maps(m, case.D, kind)
    for variant in ("default", "tol1e-2"):
        o = opts_of(m, variant)
        if route == "mes":
            rp = gp.mes_maximize(y_star, case.starts, N_LOCAL, opts=o)
        else:
            rp = gp.acq_maximize(case.starts, N_LOCAL, acq, mc.UCB_H, opts=o)
        sp = gp.last_stats()
        if route == "mes":
            rs = gp.mes_maximize_sub(y_star, maps, case.starts, N_LOCAL, opts=o)
        else:
            rs = gp.acq_maximize_sub(maps, case.starts, N_LOCAL, acq, mc.UCB_H, opts=o)
        ss = gp.last_stats()
        assert same_bits(rs["y_stars"], rp["y_stars"]), f"{np.count_nonzero(bits(rs['y_stars']) != bits(rp['y_stars']))} of {case.S} end values differ"
        assert np.array_equal(rs["x_stars"], rp["x_stars"]) and np.array_equal(rs["z_stars"], rp["x_stars"])
        assert rs["index"] == rp["index"] and rs["value"] == rp["value"] and np.array_equal(rs["x"], rp["x"]) and np.array_equal(rs["z"], rp["x"])
        assert ss == sp, (ss, sp)
    gp.close()


@pytest.mark.parametrize("kind", ("identity", "box01"))
def test_identity_map_is_the_plain_maximiser_of_the_draws(m, ctx, kind):
    case = mc.Case("path", 1)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, case.n_draws, case.F, seed=case.path_seed)
    maps = m.SubMaps(np.eye(case.D), np.zeros(case.D), None if kind == "identity" else np.zeros(case.S, dtype=np.int32))
    rp = ps.maximize(case.starts, N_LOCAL)
    rs = ps.maximize_sub(maps, case.starts, N_LOCAL)
    assert same_bits(rs["value"], rp["value"]) and np.array_equal(rs["index"], rp["index"])
    assert np.array_equal(rs["x"], rp["x"]) and np.array_equal(rs["z"], rp["x"])
    ps.close()
    gp.close()


# ---- 4. the maximisers against the restated bounded L-BFGS ----------------------------------------------------------------------------
def restated_cases():
    out = [("acq", i, v) for i, v in sc.case_ids()]
    out += [("logei", i, v) for i, v in sc.case_ids((0, 7))]
    out += [("mes", i, v) for i, v in sc.case_ids((3, 7))]
    return out


def check_winner(rg, case, maps, offset):
    j = rg["index"] - offset
    assert 0 <= j < rg["y_stars"].size
    assert rg["value"] == rg["y_stars"][j] and rg["value"] == rg["y_stars"].max() and j == int(np.argmax(rg["y_stars"]))
    assert same_bits(rg["z"], rg["z_stars"][:, j]) and same_bits(rg["x"], rg["x_stars"][:, j])


@pytest.mark.parametrize("c", restated_cases(), ids=lambda c: f"{c[0]}-{sc.case_name(c[1:])}")
def test_maximize_sub_against_the_restatement(m, ctx, c):
    kind, i, variant = c
    case = sc.SubCase(i)
    route = kind if kind != "acq" else ("ei" if case.acq == mc.EI else "ucb")
    label = f"{kind}-{sc.case_name((i, variant))}"
    maps = m.SubMaps(case.A, case.c, case.map_of_start)
    r = Routes(m, ctx, case, with_path=False)
    offset = 1000 if variant == "history3" else 0
    rg = r.maximize_sub(route, maps, case.starts, opts=opts_of(m, variant), offset=offset)
    stats = r.gp.last_stats()
    rr = mc.restated(lambda T, live: r.sub(route, maps.subset(live), T), case, mc.VARIANTS[variant], with_live=True)
    assert same_bits(rg["x_stars"], sr.expand(case.A, case.c, case.map_of_start, rg["z_stars"])), "x_stars is not the expand of z_stars"
    check_winner(rg, case, maps, offset)
    held = dict(x_stars=rg["z_stars"], y_stars=rg["y_stars"], index=rg["index"] - offset, value=rg["value"], x=rg["z"])
    mc.hold_to_restatement(held, rr, label, stats=stats)
    # without the per-start outputs: the same winner
    r1 = r.maximize_sub(route, maps, case.starts, opts=opts_of(m, variant), offset=offset, want_all=False)
    assert r1["index"] == rg["index"] and r1["value"] == rg["value"] and same_bits(r1["z"], rg["z"]) and same_bits(r1["x"], rg["x"])
    r.close()


@pytest.mark.parametrize("c", sc.case_ids((0, 5, 6)), ids=lambda c: f"path-{sc.case_name(c)}")
def test_path_maximize_sub_against_the_restatement(m, ctx, c):
    """3 draws x 50 starts in one lock-step search: start j maximises draw j / 50 on map 7 j mod n_maps; one winner per draw."""
    i, variant = c
    case = sc.SubCase(i)
    T = N_DRAWS * PER_DRAW
    case.S, case.starts = T, mc.box_starts(case.d, T, sc.SEED + i)
    moc = (7 * np.arange(T)) % case.n_maps
    maps = m.SubMaps(case.A, case.c, moc)
    gp = m.GP(ctx, case.X, case.y, case.theta, case.b, case.kernel)
    ps = m.PathSamples(gp, N_DRAWS, N_FREQ, seed=1234 + case.D)
    r = ps.maximize_sub(maps, case.starts, N_LOCAL, opts=opts_of(m, variant))
    rr = mc.restated(lambda Tz, live: ps.eval_sub(maps.subset(live), Tz, live // PER_DRAW), case, mc.VARIANTS[variant], with_live=True)
    assert r["z"].shape == (case.d, N_DRAWS) and np.all((r["z"] >= 0.0) & (r["z"] <= 1.0))
    cols = np.arange(N_DRAWS) * PER_DRAW + r["index"]
    win = maps.subset(cols)
    assert same_bits(r["x"], sr.expand(case.A, case.c, moc[cols], r["z"])), "x_out is not the expand of z_out"
    at = ps.eval_sub(win, r["z"], np.arange(N_DRAWS), want_grad=False)
    for s in range(N_DRAWS):
        mc.hold_winner_to_restatement(r["value"][s], int(r["index"][s]), rr["y_stars"][s * PER_DRAW:(s + 1) * PER_DRAW], at[s],
                                      f"path-{sc.case_name(c)} draw {s}")
    ps.close()
    gp.close()


# ---- 5. trust regions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", (6, 7), ids=sc.shape_name)
def test_trust_regions_keep_their_starts_inside_and_do_not_see_each_other(m, ctx, i):
    case = sc.SubCase(i)
    assert case.kind == "box"
    maps = m.SubMaps(case.A, case.c, case.map_of_start)
    r = Routes(m, ctx, case, with_path=False)
    route = "ei" if case.acq == mc.EI else "ucb"
    full = r.maximize_sub(route, maps, case.starts)
    lo = case.c[case.map_of_start].T
    hi = (case.c + np.einsum("krr->kr", case.A))[case.map_of_start].T          # lo + (hi - lo) 1, as the expand rounds it
    assert np.all(full["x_stars"] >= lo) and np.all(full["x_stars"] <= hi)
    assert np.all(lo >= 0.0) and np.all(hi <= 1.0 + 2.3e-16)
    for k in range(case.n_maps):
        own = np.nonzero(case.map_of_start == k)[0]
        alone = r.maximize_sub(route, maps.subset(own), case.starts[:, own])
        for key in ("z_stars", "x_stars", "y_stars"):
            assert same_bits(alone[key], full[key][..., own]), (k, key)
        assert alone["value"] == full["y_stars"][own].max() and own[alone["index"]] == own[int(np.argmax(full["y_stars"][own]))]
    r.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_call(m, ctx):
    case = sc.SubCase(3)
    D, d, K = case.D, case.d, case.n_maps
    r = Routes(m, ctx, case)
    gp, ps = r.gp, r.ps
    Z, k = case.eval_points(7, 1)
    draws = np.arange(7) % N_DRAWS
    good = m.SubMaps(case.A, case.c, k)
    nan_A, inf_c = case.A.copy(), case.c.copy()
    nan_A[K - 1, D - 1, d - 1] = np.nan
    inf_c[K - 1, D - 1] = np.inf
    bad_maps = {
        "struct_size 0": good.struct(struct_size=0),
        "struct_size too large": good.struct(struct_size=good.struct().struct_size + 8),
        "d = 0": good.struct(d=0),
        "d = D + 1": good.struct(d=D + 1),
        "n_maps = 0": good.struct(n_maps=0),
        "A NULL": good.struct(A=None),
        "c NULL": good.struct(c=None),
        "NaN in A": m.SubMaps(nan_A, case.c, k),
        "inf in c": m.SubMaps(case.A, inf_c, k),
        "map = n_maps": m.SubMaps(case.A, case.c, np.where(np.arange(7) == 5, K, k)),   # within the 2 N_DRAWS columns of the path call
        "map = -1": m.SubMaps(case.A, case.c, np.where(np.arange(7) == 0, -1, k)),
    }
    before = gp.acq_eval_sub(good, Z)
    for what, bad in bad_maps.items():
        calls = {
            "acq_eval_sub": lambda: gp.acq_eval_sub(bad, Z),
            "acq_maximize_sub": lambda: gp.acq_maximize_sub(bad, Z, 3),
            "mes_eval_sub": lambda: gp.mes_eval_sub(r.y_star, bad, Z),
            "mes_maximize_sub": lambda: gp.mes_maximize_sub(r.y_star, bad, Z, 3),
            "path eval_sub": lambda: ps.eval_sub(bad, Z, draws),
            "path maximize_sub": lambda: ps.maximize_sub(bad, Z[:, :2 * N_DRAWS], 3),
        }
        for name, call in calls.items():
            with pytest.raises(m.SlsError, match="error -1"):
                call()
            print(f"{name} refuses {what}: {m.lib().sls_last_error().decode()}")
    with pytest.raises(m.SlsError, match="draw_of_point is NULL"):
        ps.eval_sub(good, Z, None)
    with pytest.raises(m.SlsError, match="unknown acquisition type"):
        gp.acq_eval_sub(good, Z, acq=7)
    with pytest.raises(m.SlsError, match="unknown acquisition type"):
        gp.acq_maximize_sub(good, Z, 3, acq=7)
    # the handle still works, and an empty call is a no-op
    after = gp.acq_eval_sub(good, Z)
    assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])
    empty = np.zeros((d, 0))
    none = m.SubMaps(case.A, case.c, np.zeros(0, dtype=np.int32))
    assert gp.acq_eval_sub(none, empty)[0].shape == (0,)
    assert gp.mes_eval_sub(r.y_star, none, empty)[0].shape == (0,)
    assert ps.eval_sub(none, empty, np.zeros(0, dtype=np.int32))[0].shape == (0,)
    # a path object of a handle that has changed since is refused
    gp.append_point(np.full(D, 0.3), 0.1)
    with pytest.raises(m.SlsError, match="refitted or grown"):
        ps.eval_sub(good, Z, draws)
    with pytest.raises(m.SlsError, match="refitted or grown"):
        ps.maximize_sub(good, Z[:, :2 * N_DRAWS], 3)
    assert gp.acq_eval_sub(good, Z)[0].shape == (7,)
    r.close()
