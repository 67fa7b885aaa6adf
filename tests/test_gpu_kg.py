"""The knowledge gradient on a discrete set on the MI355X (sls_kg_*): the combiner alone on caller-supplied lines (sls_kg_lines) at
every pad of its sort and on degenerate line sets, the fixed points against sls_gp_predict, the slopes against sls_gp_predict_cov and
the numpy restatement (tests/kg_ref.py), the value and the gradient on the device's own inputs against an mpmath evaluation that uses
neither the sort nor the scan, a real sls_gp_append_point, central differences, noise_var = 0, the guard, the bit-level contract,
stale objects and the argument errors.

Bounds that are measured, not guessed: the device is held to 8 times the error the float64 restatement itself shows against the
mpmath reference on the same float64 inputs (the combiner margin of tests/test_gpu_jes.py: another libm), with a floor of
eps max(1, |value|); both figures are printed.  The posterior covariances c_k(x) of the device are read through a joint-entropy-search
object on the same points: the two criteria share that stage, launch for launch."""
import ctypes as C

import numpy as np
import pytest
import torch      # before libsls_hip.so is loaded (tests/test_gpu_device_entry.py): the library binds to the HIP runtime torch brought

import gram_ref
import jes_ref
import kg_cases
import kg_ref
from util import sls

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SE, MATERN52 = 0, 1
B = 0.05


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.fixture
def same_route(monkeypatch):
    monkeypatch.setenv("SLS_WAVE_PATH", "0")
    monkeypatch.setenv("SLS_TRI_PREDICT", "0")


# ---- the combiner alone ------------------------------------------------------------------------------------------------------------
def on_envelope(a, b):
    on = np.zeros(len(a), dtype=bool)
    on[kg_ref.envelope([float(v) for v in a], [float(v) for v in b])[0]] = True
    return on


def check_lines(ctx, a, Bm, a_self, b_self, mp_rows, label):
    """One sls_kg_lines call against the restatement (every candidate) and the mpmath reference (the rows mp_rows): returns
    (device error, restatement error) of the value, beta and pi."""
    M, K = Bm.shape
    own = a_self is not None
    out = ctx.kg_lines(a, Bm, a_self, b_self)
    val, beta, prob = out[:3]
    rv, rb, rp, ro = kg_ref.lines_batch(a, Bm, a_self, b_self)
    total = prob.sum(axis=1) + (out[3][:, 1] if own else 0.0)
    assert np.all(np.abs(total - 1.0) <= 4 * EPS), (label, np.abs(total - 1.0).max())
    assert np.all(val >= 0.0)
    for mm in range(M):
        al, bl = (np.append(a, a_self[mm]), np.append(Bm[mm], b_self[mm])) if own else (a, Bm[mm])
        on = on_envelope(al, bl)
        assert np.all(beta[mm][~on[:K]] == 0.0) and np.all(prob[mm][~on[:K]] == 0.0), (label, mm)
        if own and not on[K]:
            assert out[3][mm, 0] == 0.0 and out[3][mm, 1] == 0.0
    # every candidate against the restatement: the same operations on the same bits, another libm.  A term (b' - b) f carries at most
    # ~3 eps |b' - b| (exp to 1 ulp, erfc to a few), their sum (b_max - b_min) of that; beta and pi a few eps of phi <= 0.4, Phi <= 1
    spread = Bm.max(axis=1) - Bm.min(axis=1) if not own else np.maximum(Bm.max(axis=1), b_self) - np.minimum(Bm.min(axis=1), b_self)
    assert np.all(np.abs(val - rv) <= 16 * EPS * (spread + np.abs(rv)) + 1e-320), (label, np.abs(val - rv).max())
    assert np.abs(beta - rb).max() <= 8 * EPS and np.abs(prob - rp).max() <= 8 * EPS, label
    if own:
        assert np.abs(out[3] - ro).max() <= 8 * EPS, label
    err = np.zeros((3, 2))
    for mm in mp_rows:
        al, bl = (np.append(a, a_self[mm]), np.append(Bm[mm], b_self[mm])) if own else (a, Bm[mm])
        mv, mb, mpi = kg_ref.lines_mp(al, bl)
        mv += max(0.0, a_self[mm] - a.max()) if own else 0.0
        dev = (val[mm], np.append(beta[mm], out[3][mm, 0]) if own else beta[mm], np.append(prob[mm], out[3][mm, 1]) if own else prob[mm])
        ref = (rv[mm], np.append(rb[mm], ro[mm, 0]) if own else rb[mm], np.append(rp[mm], ro[mm, 1]) if own else rp[mm])
        for q, (d, r, x) in enumerate(zip(dev, ref, (mv, mb, mpi))):
            floor = EPS * max(1.0, abs(mv)) if q == 0 else EPS
            err[q, 0] = max(err[q, 0], np.abs(d - x).max())
            err[q, 1] = max(err[q, 1], np.abs(r - x).max(), floor)
    return err


@pytest.mark.parametrize("own", [False, True], ids=["fixed", "self"])
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 129, 1023, 1024])
def test_combiner_on_random_lines(ctx, K, own):
    rng = np.random.default_rng(100 + 2 * K + own)
    err = np.zeros((3, 2))
    for M in (1, 129, 300):
        a = rng.standard_normal(K)
        Bm = np.asfortranarray(rng.standard_normal((M, K)) * rng.uniform(0.01, 2.0, (M, 1)))
        if K >= 63:
            Bm[:, 5] = Bm[:, 40]                                                   # equal slopes among the random ones
        a_self = rng.standard_normal(M) + np.where(np.arange(M) % 2 == 0, 1.5, -0.5) if own else None   # on both sides of a_max
        b_self = np.abs(rng.standard_normal(M)) if own else None
        rows = np.unique(np.linspace(0, M - 1, 8 if K <= 129 else 3).astype(int))
        err = np.maximum(err, check_lines(ctx, a, Bm, a_self, b_self, rows, (K, M, own)))
    print(f"K {K} {'with' if own else 'without'} the self line: device / float64 restatement error against mpmath: value "
          f"{err[0, 0]:.3g} / {err[0, 1]:.3g}, beta {err[1, 0]:.3g} / {err[1, 1]:.3g}, pi {err[2, 0]:.3g} / {err[2, 1]:.3g}")
    assert np.all(err[:, 0] <= 8 * err[:, 1]), err


DEGENERATE = kg_cases.DEGENERATE


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_combiner_on_degenerate_lines(ctx, name):
    a, b = (np.array(v) for v in DEGENERATE[name])
    K = a.size
    # candidate 0: the set; candidate 1: the set mirrored in z; candidate 2: with a self line that repeats line 0 (a duplicate of it)
    Bm = np.asfortranarray(np.stack([b, -b]))
    err = check_lines(ctx, a, Bm, None, None, [0, 1], name)
    e2 = check_lines(ctx, a, np.asfortranarray(b[None, :]), np.array([a[0]]), np.array([b[0]]), [0], name + " + self")
    err = np.maximum(err, e2)
    print(f"{name}: device / restatement error against mpmath: value {err[0, 0]:.3g} / {err[0, 1]:.3g}, beta {err[1, 0]:.3g} / "
          f"{err[1, 1]:.3g}, pi {err[2, 0]:.3g} / {err[2, 1]:.3g}")
    assert np.all(err[:, 0] <= 8 * err[:, 1]), err
    val, beta, prob = ctx.kg_lines(a, Bm)
    if name in ("all slopes equal", "all b = 0"):
        first = int(np.argmax(a))                                                 # E = 1: exactly 0, beta 0, pi the lowest arg max
        assert np.array_equal(val, np.zeros(2)) and np.array_equal(beta, np.zeros((2, K)))
        assert np.array_equal(prob, np.tile(np.eye(K)[first], (2, 1)))
    if name == "three lines through one point":
        assert beta[0, 1] == 0.0 and prob[0, 1] == 0.0                            # the middle line is popped: t <= the breakpoint
    # the self line that duplicates line 0 loses the tie to the lower index
    so = ctx.kg_lines(a, np.asfortranarray(b[None, :]), np.array([a[0]]), np.array([b[0]]))[3]
    assert so[0, 0] == 0.0 and so[0, 1] == 0.0


def test_lines_arguments(m, ctx):
    lib, dp = m.lib(), C.POINTER(C.c_double)
    p = lambda x: x.ctypes.data_as(dp)
    a, Bm, v = np.array([0.1, 0.2]), np.asfortranarray(np.ones((3, 2))), np.empty(3)

    def refused(rc, word):
        msg = lib.sls_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(lib.sls_kg_lines(None, p(a), p(Bm), None, None, 2, 3, p(v), None, None, None), "ctx is NULL")
    refused(lib.sls_kg_lines(ctx.h, p(a), p(Bm), None, None, 0, 3, p(v), None, None, None), "K = 0")
    refused(lib.sls_kg_lines(ctx.h, p(a), p(Bm), None, None, 1025, 3, p(v), None, None, None), "K = 1025")
    refused(lib.sls_kg_lines(ctx.h, p(a), p(Bm), None, None, 2, -1, p(v), None, None, None), "M = -1")
    refused(lib.sls_kg_lines(ctx.h, None, p(Bm), None, None, 2, 3, p(v), None, None, None), "NULL")
    refused(lib.sls_kg_lines(ctx.h, p(a), p(Bm), p(v), None, 2, 3, p(v), None, None, None), "go together")
    refused(lib.sls_kg_lines(ctx.h, p(a), p(Bm), None, None, 2, 3, None, None, None, None), "val is NULL")
    refused(lib.sls_kg_lines(ctx.h, p(a), p(Bm), None, None, 2, 3, p(v), None, None, p(v)), "self_out")
    bad = Bm.copy(order="F")
    bad[1, 1] = np.nan
    refused(lib.sls_kg_lines(ctx.h, p(a), p(bad), None, None, 2, 3, p(v), None, None, None), "not finite")
    assert lib.sls_kg_lines(ctx.h, None, None, None, None, 2, 0, None, None, None, None) == 0
    only = ctx.kg_lines(a, Bm, want_beta=False, want_prob=False)[0]                # the value alone: the same bits
    assert np.array_equal(only, ctx.kg_lines(a, Bm)[0])


# ---- the whole pass ------------------------------------------------------------------------------------------------------------------
def problem(D, N, seed, ell=0.5, a=0.5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


def ref_points(rng, K, X):
    """x_k uniform with two of them on data points (one for K = 1)."""
    D, N = X.shape
    xs = rng.uniform(0, 1, (D, K))
    xs[:, 0] = X[:, N // 3]
    if K > 2:
        xs[:, K // 2] = X[:, N // 2]
    return np.asfortranarray(xs)


CASES = [(SE, 90, 2), (MATERN52, 700, 16), (SE, 300, 96), (MATERN52, 130, 257)]
_FITS = {}


def case(kernel, N, D):
    """The problem, its float64 fit (computed once, shared, never modified) and cond(K_y): the shapes of tests/test_gpu_jes.py."""
    key = (kernel, N, D)
    if key not in _FITS:
        X, y, theta = problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
        f = jes_ref.fit(X, y, theta[1:], theta[0], B, kernel)
        ev = np.linalg.eigvalsh(f["K"])
        _FITS[key] = (X, y, theta, f, ev[-1] / ev[0])
    return _FITS[key]


def device_cov(gp, xs, Xs):
    """c_k(x_m) as the device forms it: the stage the knowledge gradient shares with joint entropy search."""
    j = gp.jes_create(xs, np.zeros(xs.shape[1]), 1.0)
    cov = j.eval(Xs, B, want_grad=False, want_cov=True)[1]
    j.close()
    return cov


def subset(M, K):
    return np.unique(np.linspace(0, M - 1, 4 if K <= 129 else 2).astype(int))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,N,D", CASES)
def test_points_slopes_value_and_gradient(m, ctx, same_route, kernel, N, D, mode):
    X, y, theta, f, cond = case(kernel, N, D)
    gp = m.GP(ctx, X, y, theta, B, kernel)
    gp.set_sigma_mode(mode)
    rng = np.random.default_rng(5)
    worst = dict(cov=0.0, dev_v=0.0, ref_v=0.0, dev_g=0.0, ref_g=0.0, val=0.0, grad=0.0, lines=0)
    for K in (1, 7, 129, 1024):
        xs = ref_points(rng, K, X)
        kg = gp.kg_create(xs)
        a, a_max, arg = kg.points()
        mu_p, _ = gp.predict(xs)
        assert np.array_equal(a, mu_p) and a_max == a.max() and arg == int(np.argmax(a))       # the same route: bit-equal
        o = kg_ref.points(f, xs)
        for M in (1, 129, 300):
            Xs = rng.uniform(0, 1, (D, M))
            mu, sg = gp.predict(Xs)
            dmu, dsg = gp.predict_grad(Xs)
            s = np.sqrt(sg * sg + B)
            cov = device_cov(gp, xs, Xs)
            ref_cov, dcov = jes_ref.covariances(f, o, Xs, True)
            tol, tol_dc = jes_ref.covariance_bounds(f, o, Xs, cond)
            for own in (True, False):
                val, grad, slope = kg.eval(Xs, B, include_self=own, want_grad=True, want_slopes=True)
                assert slope.shape == (M, K) and np.all(np.isfinite(slope)) and np.all(val >= 0.0)
                # the slopes: the device's covariance over its s (a division), the restatement within the conditioning bound
                assert np.all(np.abs(slope - cov / s[:, None]) <= 4 * EPS * np.abs(slope))
                e_c = np.abs(slope * s[:, None] - ref_cov) / (tol + 4 * EPS * np.abs(ref_cov))
                worst["cov"] = max(worst["cov"], e_c.max())
                assert e_c.max() <= 1.0, (K, M, e_c.max(), cond)
                if own and (M == 300 or K == 7):
                    joint = gp.predict_cov(np.concatenate([Xs, xs], axis=1))[1][:M, M:]
                    tj = tol + 8 * np.sqrt(cond) * EPS * theta[0] * np.sqrt(N)
                    assert np.all(np.abs(slope * s[:, None] - joint) <= tj + 4 * EPS * np.abs(joint)), (K, M)
                rv, rg, info = kg_ref.kg(mu, sg, cov, a, B, own, dmu, dsg, dcov)
                assert not info["bad"].any()
                worst["val"], worst["grad"] = max(worst["val"], val.max()), max(worst["grad"], np.abs(grad).max())
                worst["lines"] = max(worst["lines"], int((info["pi"] > 0).sum(axis=1).max()))
                sb, ds = subset(M, K), np.arange(min(D, 6))
                sd = np.ix_(ds, sb)
                mv, mg = kg_ref.kg_mp(mu[sb], sg[sb], cov[sb], a, B, own, dmu[sd], dsg[sd], dcov[sd])
                floor_v = EPS * np.maximum(1.0, np.abs(mv))
                e_ref = max(np.abs(rv[sb] - mv).max(), floor_v.max())
                e_dev = np.abs(val[sb] - mv).max()
                # gradient: the device's grad c differs from the restatement's by the conditioning of K_y: sum_k |h_k| tol_dc
                cterm = np.einsum("mk,dmk->dm", np.abs(info["H"]), tol_dc)
                floor_g = EPS * max(1.0, np.abs(mg).max())
                g_ref = max(np.abs(rg[sd] - mg).max(), floor_g)
                g_dev = (np.abs(grad[sd] - mg) - cterm[sd]).max()
                for kk, vv in (("dev_v", e_dev / e_ref), ("ref_v", e_ref), ("dev_g", g_dev / g_ref), ("ref_g", g_ref)):
                    worst[kk] = max(worst[kk], vv)
                assert e_dev <= 8 * e_ref, (K, M, own, e_dev, e_ref)
                assert g_dev <= 8 * g_ref, (K, M, own, g_dev, g_ref)
                # every point against the restatement, loosely (the same formula in the same precision on the same inputs)
                assert np.abs(val - rv).max() <= 1e-12 * (1.0 + np.abs(rv).max()), (K, M, own, np.abs(val - rv).max())
                assert np.all(np.abs(grad - rg) <= 1e-10 * (1.0 + np.abs(rg).max()) + cterm), (K, M, own)
                assert np.array_equal(kg.eval(Xs, B, include_self=own), val)                    # val alone
        kg.close()
    print(f"kernel {kernel} N {N} D {D} mode {mode}: cond {cond:.3g}, largest covariance error / bound {worst['cov']:.3g}; float64 "
          f"restatement against mpmath: value {worst['ref_v']:.3g}, gradient {worst['ref_g']:.3g}; device error / restatement error: "
          f"value {worst['dev_v']:.3g}, gradient beyond the conditioning term {worst['dev_g']:.3g}; largest value {worst['val']:.3g}, "
          f"gradient component {worst['grad']:.3g}, lines on an envelope {worst['lines']}")
    assert worst["val"] > 0.0 and worst["grad"] > 0.0 and worst["lines"] >= 2                   # the criterion is not flat here
    gp.close()


@pytest.mark.parametrize("kernel,N,D", [(SE, 90, 2), (MATERN52, 700, 16)])
def test_future_mean_against_a_real_appended_point(m, ctx, kernel, N, D):
    """mu_{n+1}(x_k) = a_k + b_k z after the observation y = mu(x) + s z at x, with noise_var the handle's b: sls_gp_append_point."""
    X, y, theta, f, cond = case(kernel, N, D)
    gp = m.GP(ctx, X, y, theta, B, kernel)
    rng = np.random.default_rng(13)
    K = 7
    xs = ref_points(rng, K, X)
    kg = gp.kg_create(xs)
    a = kg.points()[0]
    x = rng.uniform(0.2, 0.8, (D, 1))
    mu, sg = gp.predict(x)
    _, slope = kg.eval(x, B, want_slopes=True)
    s = np.sqrt(sg[0] ** 2 + B)
    vs = np.abs(gp.matrix(m.GP_ALPHA)).max()
    tol_mu = 1e-10 * theta[0] + 4 * cond * EPS * max(vs, 1.0) * theta[0] * np.sqrt(N)       # the bound of tests/test_gpu_jes.py
    for z in (-1.5, 0.3, 2.0):
        g2 = m.GP(ctx, X, y, theta, B, kernel)
        g2.append_point(x[:, 0], mu[0] + s * z)
        new = g2.predict(xs)[0]
        err = np.abs(new - (a + slope[0] * z)).max()
        print(f"N {N} z {z}: appended point against a_k + b_k z: {err:.3g} (bound {tol_mu:.3g}), largest |b_k z| {np.abs(slope[0] * z).max():.3g}")
        assert err <= tol_mu
        g2.close()
    kg.close()
    gp.close()


@pytest.mark.parametrize("kernel,N,D,mode", [(SE, 90, 2, 0), (MATERN52, 700, 16, 1), (MATERN52, 130, 257, 0)])
def test_gradient_against_central_differences(m, ctx, kernel, N, D, mode):
    X, y, theta, f, cond = case(kernel, N, D)
    gp = m.GP(ctx, X, y, theta, B, kernel)
    gp.set_sigma_mode(mode)
    rng = np.random.default_rng(17)
    kg = gp.kg_create(ref_points(rng, 7, X))
    Xs = rng.uniform(0.05, 0.95, (D, 8))
    h = 1e-6
    for own, nv in ((True, B), (False, B), (True, 0.0)):
        val, grad = kg.eval(Xs, nv, include_self=own, want_grad=True)
        assert np.all(np.isfinite(val)) and np.all(val >= 0.0) and np.abs(grad).max() > 0.0
        for d in range(min(D, 4)):
            E = np.zeros((D, 8))
            E[d] = h
            fd = (kg.eval(Xs + E, nv, include_self=own) - kg.eval(Xs - E, nv, include_self=own)) / (2 * h)
            err = np.abs(fd - grad[d]).max()
            print(f"N {N} D {D} self {own} noise_var {nv}: central differences, d = {d}: {err:.3g} (|grad| max {np.abs(grad).max():.3g})")
            assert err <= 1e-6 * (1.0 + np.abs(grad).max())                     # the bound of the JES test
    kg.close()
    gp.close()


def test_noise_var_zero_against_the_restatement(m, ctx, same_route):
    kernel, N, D = MATERN52, 700, 16
    X, y, theta, f, cond = case(kernel, N, D)
    gp = m.GP(ctx, X, y, theta, B, kernel)
    rng = np.random.default_rng(19)
    xs = ref_points(rng, 7, X)
    kg = gp.kg_create(xs)
    a = kg.points()[0]
    Xs = rng.uniform(0, 1, (D, 129))
    mu, sg = gp.predict(Xs)
    cov = device_cov(gp, xs, Xs)
    val, slope = kg.eval(Xs, 0.0, want_slopes=True)
    assert np.all(np.abs(slope - cov / sg[:, None]) <= 4 * EPS * np.abs(slope))   # s = sigma
    rv = kg_ref.kg(mu, sg, cov, a, 0.0)[0]
    sb = subset(129, 7)
    mv = kg_ref.kg_mp(mu[sb], sg[sb], cov[sb], a, 0.0)[0]
    e_ref = max(np.abs(rv[sb] - mv).max(), EPS * np.maximum(1.0, np.abs(mv)).max())
    print(f"noise_var = 0: float64 restatement {e_ref:.3g}, device {np.abs(val[sb] - mv).max():.3g}")
    assert np.abs(val[sb] - mv).max() <= 8 * e_ref and np.abs(val - rv).max() <= 1e-12 * (1.0 + np.abs(rv).max())
    kg.close()
    gp.close()


def test_beyond_the_gram_guard(m, ctx):
    """l = 3e-3 at (N, D) = (129, 6): the handle forms every Gram route from raw coordinate differences (tests/test_gpu_jes.py)."""
    N, D, K = 129, 6, 7
    r = gram_ref.problem(N, D, 3e-3)
    f = jes_ref.fit(r["X"], r["y"], r["ell"], r["a"], r["b"], MATERN52)
    ev = np.linalg.eigvalsh(f["K"])
    cond = ev[-1] / ev[0]
    gp = m.GP(ctx, r["X"], r["y"], r["theta"], r["b"], MATERN52)
    rng = np.random.default_rng(4)
    xs = np.clip(r["X"][:, 41:41 + 3 * K:3] + r["ell"][:, None] * 0.5 * rng.standard_normal((D, K)) / np.sqrt(D), 0, 1)
    Xs = np.clip(r["X"][:, 40:40 + 3 * 24:3] + r["ell"][:, None] * 0.7 * rng.standard_normal((D, 24)) / np.sqrt(D), 0, 1)
    Xs[:, :K] = xs + r["ell"][:, None] * 0.3 * rng.standard_normal((D, K)) / np.sqrt(D)
    Xs = np.clip(Xs, 0, 1)
    kg = gp.kg_create(xs)
    o = kg_ref.points(f, xs)
    val, grad, slope = kg.eval(Xs, r["b"], want_grad=True, want_slopes=True)
    mu, sg = gp.predict(Xs)
    s = np.sqrt(sg * sg + r["b"])
    ref = jes_ref.covariances(f, o, Xs)
    tol, _ = jes_ref.covariance_bounds(f, o, Xs, cond)
    assert np.abs(ref).max() > 0.05 * r["a"]                                       # the covariances are there
    assert np.all(np.abs(slope * s[:, None] - ref) <= tol + 8 * EPS * np.abs(ref))
    assert np.all(val >= 0.0) and val.max() > 0.0
    h = 1e-9                                                                       # l / 3e6
    sub = np.arange(8)
    for d in range(3):
        E = np.zeros((D, 8))
        E[d] = h
        fd = (kg.eval(Xs[:, sub] + E, r["b"]) - kg.eval(Xs[:, sub] - E, r["b"])) / (2 * h)
        err = np.abs(fd - grad[d, sub]).max()
        print(f"beyond the guard: central differences, d = {d}: {err:.3g} (|grad| max {np.abs(grad[:, sub]).max():.3g})")
        assert err <= 1e-6 * (1.0 + np.abs(grad[:, sub]).max()) + 4 * cond * EPS / h
    kg.close()
    gp.close()


def test_guard(m, ctx, same_route):
    """b = 0, candidates on the data points: wherever the device's sigma is below 1e-10 the value and the gradient are exactly 0;
    everywhere they are finite."""
    D, N = 2, 25
    g = np.linspace(0.05, 0.95, 5)
    X = np.array([[a, c] for a in g for c in g]).T.copy()
    y = np.sin(3 * X[0]) * np.cos(2 * X[1])
    theta = np.array([0.5, 0.15, 0.15])
    gp = m.GP(ctx, X, y, theta, 0.0, MATERN52)
    mid = np.array([[0.1625, 0.1625], [0.3875, 0.6125], [0.8375, 0.3875], [0.6125, 0.8375]]).T      # cell centres: sigma is largest
    Xs = np.concatenate([X, mid + 0.01], axis=1)
    _, sg = gp.predict(Xs)
    guard = sg < 1e-10
    assert guard[:N].sum() >= 1 and not guard[N:].any()
    kg = gp.kg_create(np.concatenate([mid, X[:, [3, 12]]], axis=1))                                  # two of the points on data points
    for nv in (1e-4, 0.0):
        val, grad = kg.eval(Xs, nv, want_grad=True)
        assert np.array_equal(val[guard], np.zeros(guard.sum())) and np.array_equal(grad[:, guard], np.zeros((D, guard.sum())))
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad)) and np.all(val >= 0.0) and np.all(val[N:] > 0.0)
    kg.close()
    gp.close()


def test_bit_contract(m, ctx):
    D, N, M, K = 5, 300, 300, 129
    X, y, theta = problem(D, N, seed=21)
    gp = m.GP(ctx, X, y, theta, B, MATERN52)
    rng = np.random.default_rng(3)
    Xs = rng.uniform(0, 1, (D, M))
    xs = ref_points(rng, K, X)
    kg = gp.kg_create(xs)
    ev = lambda T, **kw: kg.eval(T, B, want_grad=True, want_slopes=True, **kw)
    val, grad, sl = ev(Xs)
    v2, g2, s2 = ev(Xs)
    assert np.array_equal(val, v2) and np.array_equal(grad, g2) and np.array_equal(sl, s2)          # repeated call
    perm = rng.permutation(M)
    vp, gpm, sp = ev(Xs[:, perm])
    assert np.array_equal(vp, val[perm]) and np.array_equal(gpm, grad[:, perm]) and np.array_equal(sp, sl[perm])
    sub = np.array([7, 200, 131])
    vs, gs, ss = ev(Xs[:, sub])
    assert np.array_equal(vs, val[sub]) and np.array_equal(gs, grad[:, sub]) and np.array_equal(ss, sl[sub])
    v1, g1, s1 = ev(Xs[:, 200:201])                                                                  # alone
    assert v1[0] == val[200] and np.array_equal(g1[:, 0], grad[:, 200]) and np.array_equal(s1[0], sl[200])
    ctx.set_candidate_chunk(128)
    vc, gc, sc = ev(Xs)
    ctx.set_candidate_chunk(16384)
    assert np.array_equal(vc, val) and np.array_equal(gc, grad) and np.array_equal(sc, sl)           # nor the candidate chunk
    assert np.array_equal(kg.eval(Xs, B), val)                                                       # val alone
    vg, gg = kg.eval(Xs, B, want_grad=True)
    assert np.array_equal(vg, val) and np.array_equal(gg, grad)                                      # slopes asked for or not
    vn, gn = kg.eval(Xs, B, include_self=False, want_grad=True)
    assert np.array_equal(kg.eval(Xs, B, include_self=False), vn) and not np.array_equal(vn, val)
    # the first K' points of this object against an object of those K' points: the same a_k, the same slopes
    for Kq in (1, 7):
        kq = gp.kg_create(xs[:, :Kq])
        assert np.array_equal(kq.points()[0], kg.points()[0][:Kq])
        assert np.array_equal(kq.eval(Xs, B, want_slopes=True)[1], sl[:, :Kq])
        kq.close()
    kg.close()
    gp.close()


def test_stale_object_and_argument_errors(m, ctx):
    D, N, K = 2, 30, 3
    X, y, theta = problem(D, N, seed=9)
    gp = m.GP(ctx, X, y, theta, B, SE)
    lib, dp = m.lib(), C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    Xs = np.asfortranarray(np.full((D, 3), 0.5))
    val, grad = np.empty(3), np.empty((D, 3), order="F")
    xs = np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (D, K)))
    x, v, idx = np.empty(D), C.c_double(), C.c_long()

    def refused(rc, word):
        msg = lib.sls_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def create(g, xp, Kc):
        h = C.c_void_p()
        rc = lib.sls_kg_create(g, xp, Kc, C.byref(h))
        assert rc == 0 or not h.value
        return rc, h

    ctx.prof_enable(True)
    ctx.prof_reset()
    refused(create(gp.h, p(xs), 0)[0], "K = 0")
    refused(create(gp.h, p(xs), 1025)[0], "K = 1025")
    for bad in (np.nan, np.inf, -np.inf):
        xb = xs.copy(order="F")
        xb[1, 2] = bad
        refused(create(gp.h, p(xb), K)[0], "point 2")
    refused(create(None, p(xs), K)[0], "gp is NULL")
    refused(create(gp.h, None, K)[0], "x_ref is NULL")
    refused(lib.sls_kg_create(gp.h, p(xs), K, None), "out is NULL")
    for name in ("kg_setup", "kg", "jes_cov", "cross_gram"):
        assert ctx.prof_get(name)[1] == 0, name                                   # nothing was launched
    rc, h = create(gp.h, p(xs), K)
    assert rc == 0 and h.value and ctx.prof_get("kg_setup")[1] > 0

    def ev(hh, nv, Xp, M, vp):
        return lib.sls_kg_eval(hh, C.c_double(nv), 1, Xp, M, vp, p(grad), None)

    def mx(hh, nv, sp, opts=None):
        return lib.sls_kg_maximize(hh, C.c_double(nv), 1, sp, 3, 5, opts, C.c_long(0), p(x), C.byref(v), C.byref(idx), None, None)

    ctx.prof_reset()
    for nv in (-1.0, -1e-300, np.inf, np.nan):
        refused(ev(h, nv, p(Xs), 3, p(val)), "noise_var")
        refused(mx(h, nv, p(Xs)), "noise_var")
    refused(ev(None, B, p(Xs), 3, p(val)), "k is NULL")
    refused(ev(h, B, None, 3, p(val)), "Xs is NULL")
    refused(ev(h, B, p(Xs), 3, None), "val is NULL")
    refused(ev(h, B, p(Xs), -1, p(val)), "M = -1")
    refused(mx(None, B, p(Xs)), "k is NULL")
    refused(mx(h, B, None), "starts is NULL")
    opts = m.LbfgsOpts()
    opts.struct_size = 999
    refused(mx(h, B, p(Xs), C.byref(opts)), "struct_size")
    refused(lib.sls_kg_points(None, None, None, None), "k is NULL")
    for name in ("kg", "jes_cov", "cross_gram"):
        assert ctx.prof_get(name)[1] == 0, name
    assert ev(h, B, None, 0, None) == 0                                           # M = 0: nothing to do
    assert ev(h, B, p(Xs), 3, p(val)) == 0 and np.all(np.isfinite(val))
    assert ctx.prof_get("kg")[1] == 2 and ctx.prof_get("jes_cov")[1] == 1 and ctx.prof_get("jes")[1] == 0
    assert mx(h, B, p(Xs)) == 0
    assert lib.sls_kg_points(h, None, None, None) == 0
    # stale: a refit, a sigma-mode switch, an appended point (each changes the generation); no stale state is used, nothing is launched
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda")
    yd = torch.from_numpy(np.ascontiguousarray(y + 0.01)).to("cuda")
    for change in (lambda: gp.refit_dev(Xd.data_ptr(), yd.data_ptr()), lambda: gp.set_sigma_mode(1),
                   lambda: gp.append_point(np.full(D, 0.3), 0.1)):
        change()
        ctx.prof_reset()
        refused(ev(h, B, p(Xs), 3, p(val)), "sls_kg_create")
        refused(mx(h, B, p(Xs)), "sls_kg_create")
        refused(lib.sls_kg_points(h, p(val), None, None), "sls_kg_create")
        assert ctx.prof_get("kg")[1] == 0 and ctx.prof_get("cross_gram")[1] == 0
        assert lib.sls_kg_destroy(h) == 0
        rc, h = create(gp.h, p(xs), K)
        assert rc == 0 and ev(h, B, p(Xs), 3, p(val)) == 0
    ctx.prof_enable(False)
    assert lib.sls_kg_destroy(h) == 0 and lib.sls_kg_destroy(None) == 0
    gp.close()
