"""CPU-side checks of the Laplace posterior for preference data (include/sls_hip.h "Laplace posterior"): the numpy restatement
tests/laplace_ref.py against the project's own BTL objective (oracle.pref_objective), its algebra, and the public surface."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import laplace_ref as lr
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(N, D, seed, kernel, s, b=0.005, n_tuples=None):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (D, N))
    theta = np.full(D + 1, 0.5)
    n_tuples = n_tuples or (2 * N) // 3
    prefs = [tuple(int(i) for i in rng.choice(N, size=int(rng.integers(2, 5)), replace=False)) for _ in range(n_tuples)]
    y = 0.05 * rng.normal(size=N)
    return X, y, theta, b, kernel, prefs, s


@pytest.mark.parametrize("s", [0.01, 1.0])
@pytest.mark.parametrize("kernel", [lr.SE, lr.MATERN52])
@pytest.mark.parametrize("N", [12, 40])
def test_w_is_the_hessian_of_the_projects_btl_term(oracle, N, kernel, s):
    """K_y^-1 + W of the restatement = minus the central finite-difference Jacobian (h = 1e-6) of the oracle's own gradient in y:
    W is the Hessian of THE PROJECT'S Bradley-Terry-Luce term, scale convention included.  Bound: 1e-8 of the largest entry, ten times
    the finite-difference error of these cases (5e-10 .. 6e-10)."""
    X, y, theta, b, kernel, prefs, s = case(N, 3, 100 + N, kernel, s)
    ref = lr.LaplaceRef(X, y, theta, b, kernel, prefs, s)
    h = 1e-6
    J = np.empty((N, N))
    for j in range(N):
        e = np.zeros(N)
        e[j] = h
        gp = oracle.pref_objective(kernel, X, prefs, y + e, a=0.5, r=0.5, b=b, btl_scale=s)[1]
        gm = oracle.pref_objective(kernel, X, prefs, y - e, a=0.5, r=0.5, b=b, btl_scale=s)[1]
        J[:, j] = (gp - gm) / (2 * h)
    want = np.linalg.inv(ref.Ky) + ref.W
    err = np.abs(-J - want).max() / np.abs(want).max()
    print(f"N {N} kernel {kernel} s {s}: |-J - (K_y^-1 + W)| / max = {err:.3e}")
    assert err <= 1e-8, err


@pytest.mark.parametrize("s", [0.01, 1.0])
@pytest.mark.parametrize("kernel", [lr.SE, lr.MATERN52])
def test_algebra_of_the_restatement(kernel, s):
    X, y, theta, b, kernel, prefs, s = case(40, 3, 7, kernel, s)
    prefs = prefs + [prefs[0], (5, 5, 9)]          # a tuple given twice, an index repeated inside a tuple
    ref = lr.LaplaceRef(X, y, theta, b, kernel, prefs, s)
    N = ref.N
    P = np.linalg.inv(ref.Ky) + ref.W
    I = ref.cov_g @ P
    assert np.abs(I - np.eye(N)).max() <= 1e-9 * np.linalg.cond(P), np.abs(I - np.eye(N)).max()
    assert np.array_equal(ref.W, ref.W.T)
    assert np.abs(ref.W.sum(axis=0)).max() <= 1e-9 * np.abs(ref.W).max()             # every H has the ones vector in its null space
    ev = np.linalg.eigvalsh(ref.T)
    assert ev.min() >= -1e-12 and ev.max() < 1.0
    assert np.linalg.eigvalsh(ref.B).min() >= 1.0 - 1e-12
    Xs = np.random.default_rng(3).uniform(0, 1, (3, 50))
    prod, sub, third = ref.sigma_forms(Xs)
    scale = ref.a
    print(f"kernel {kernel} s {s}: forms differ by {np.abs(prod - sub).max() / scale:.2e}, {np.abs(prod - third).max() / scale:.2e}")
    assert np.abs(prod - sub).max() <= 1e-10 * scale and np.abs(prod - third).max() <= 1e-10 * scale
    # the Laplace variance is never below the plain one: M = K_y^-1 - K_y^-1 Sigma_g K_y^-1 and Sigma_g is positive definite
    assert np.all(ref.predict(Xs)[1] >= ref.plain_sigma(Xs) - 1e-10)
    # the joint covariance has sigma^2 on its diagonal; the evidence is what its terms say
    assert np.allclose(np.diag(ref.cov(Xs)), prod, rtol=0, atol=1e-10 * scale)
    dmu, dsg = ref.predict_grad(Xs)
    hh = 1e-6
    for d in range(3):
        E = np.zeros_like(Xs)
        E[d] = hh
        fd = (ref.predict(Xs + E)[1] - ref.predict(Xs - E)[1]) / (2 * hh)
        fm = (ref.predict(Xs + E)[0] - ref.predict(Xs - E)[0]) / (2 * hh)
        assert np.abs(fd - dsg[d]).max() <= 1e-6 * max(np.abs(dsg).max(), 1.0)
        assert np.abs(fm - dmu[d]).max() <= 1e-6 * max(np.abs(dmu).max(), 1.0)


def test_newton_map_is_a_mode():
    X, _, theta, b, kernel, prefs, s = case(40, 3, 11, lr.MATERN52, 1.0)
    y = lr.newton_map(X, theta, b, kernel, prefs, s)
    g = lr.loglik_grad(prefs, y, s, 40) - np.linalg.solve(lr.LaplaceRef(X, y, theta, b, kernel, prefs, s).Ky, y)
    assert np.abs(g).max() <= 1e-6


def test_path_restatement_layout():
    """Draw s takes 2F + 2N numbers in the order w, w', eps, z; the first k draws of an n-draw object are a k-draw object."""
    X, y, theta, b, kernel, prefs, s = case(12, 2, 5, lr.MATERN52, 1.0)
    ref = lr.LaplaceRef(X, y, theta, b, kernel, prefs, s)
    p4, p2 = lr.LaplacePathRef(ref, 4, 8, 42), lr.LaplacePathRef(ref, 2, 8, 42)
    assert np.array_equal(p4.v[:, :2], p2.v) and np.array_equal(p4.W[:, :2], p2.W)
    B0, per = lr.ph.block0(2, 8, kernel), 2 * 8 + 2 * 12
    E1 = lr.ph.normals(42, B0 + per, per)
    assert np.array_equal(p4.eps[:, 1], E1[16:28]) and np.array_equal(p4.z[:, 1], E1[28:40])
    # the sampled goodness vectors have covariance Sigma_g: L L_B^-T (L L_B^-T)^T
    Rm = ref.L @ np.linalg.inv(ref.LB).T
    assert np.allclose(Rm @ Rm.T, ref.cov_g, rtol=1e-9, atol=1e-12)


def test_surface_header_and_binding(tmp_path):
    """The four entry points are declared in a header that still compiles as pedantic C99, and the ctypes handle carries the four
    methods and the selectors."""
    hdr = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    for name in ("sls_gp_set_laplace", "sls_gp_clear_laplace", "sls_gp_laplace_get", "sls_gp_laplace_summary"):
        assert re.search(r"\bint %s\(sls_gp\*" % name, hdr), name
    for name, val in (("SLS_LAPLACE_W", 0), ("SLS_LAPLACE_COV", 1), ("SLS_LAPLACE_M", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name
    for scope in ("laplace_w", "laplace_b", "laplace_potri", "laplace_m"):
        assert '"%s"' % scope in hdr, scope
    src = tmp_path / "lap.c"
    src.write_text('#include "sls_hip.h"\n'
                   'int main(void) {\n'
                   '    unsigned flat[2] = {0u, 1u};\n'
                   '    int off[2] = {0, 2};\n'
                   '    double ll, ld, ev, out[1];\n'
                   '    int rc = sls_gp_set_laplace((sls_gp*)0, flat, off, 1, 0.01);\n'
                   '    rc += sls_gp_clear_laplace((sls_gp*)0);\n'
                   '    rc += sls_gp_laplace_get((sls_gp*)0, SLS_LAPLACE_M, out);\n'
                   '    rc += sls_gp_laplace_summary((sls_gp*)0, &ll, &ld, &ev);\n'
                   '    return rc == 0;\n}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = sls()
    for name in ("set_laplace", "clear_laplace", "laplace_matrix", "laplace_summary"):
        assert callable(getattr(m.GP, name, None)), name
    assert (m.LAPLACE_W, m.LAPLACE_COV, m.LAPLACE_M) == (0, 1, 2)
    for name in ("sls_gp_set_laplace", "sls_gp_clear_laplace", "sls_gp_laplace_get", "sls_gp_laplace_summary"):
        assert name in m.EXPORTS
    assert issubclass(m.Unsupported, m.SlsError)


def test_null_handle_is_refused_without_a_device():
    lib = sls().lib()
    flat = (C.c_uint * 2)(0, 1)
    off = (C.c_int * 2)(0, 2)
    assert lib.sls_gp_set_laplace(None, flat, off, 1, C.c_double(0.01)) == -1
    assert lib.sls_gp_clear_laplace(None) == -1
    assert lib.sls_gp_laplace_get(None, 0, None) == -1
    assert lib.sls_gp_laplace_summary(None, None, None, None) == -1
