"""Leave-one-out cross-validation on the device up a ladder of condition numbers (loo_ref.RUNGS: both kernels, (3, 37) and
(5, 130), b = 1e-8, every length scale of loo_ref.problem multiplied until cond(K_y) is about 1e6, about 1e8 and 1e9 .. 4e9) against
the 50-digit values of tests/golden/loo_illcond.npz.  The LOO quantities are where conditioning bites -- d_i = (K_y^-1)_ii,
mu_-i = y_i - alpha_i / d_i, W = 1/2 (u alpha^T + alpha u^T) - M -- and the LOO fit's box [1e-8, 50] does not keep it out of there.

Tolerance: the bound tests/test_loo_cpu.py holds numpy to on the same rungs (loo_ref.ladder_tolerances, cond from the fixture):
10 cond eps for mu (absolute scale max|y|), var, logp and L (scale sum|logp|), 100 cond eps max|g| for the D + 2 derivatives; never
tighter than the fixed tolerances of tests/test_gpu_loo.py.  Device and numpy are both backward-stable inversions of the same matrix,
so their errors are c cond eps with a modest c, and the c is the one already fixed for the reference.  Every rung is admitted by
tests/test_loo_cpu.py::test_ladder_rung_is_admitted.  The measured errors, as multiples of cond eps, are recorded
(util.record("loo_conditioning", ...); profiles/loo_conditioning.json holds those of the run that added the test)."""
import os

import numpy as np
import pytest

import loo_ref
from test_gpu_loo import same_bits
from util import record, sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.3e-16


@pytest.fixture(scope="module")
def ctx():
    c = sls().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def illcond():
    z = np.load(os.path.join(ROOT, "tests", "golden", "loo_illcond.npz"))
    return {str(n): {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(str(n) + "/")} for n in z["cases"]}


def vector_multiples(f, mu, var, logp):
    """The errors of the three vectors in units of cond eps times the scale the bound gives each: |mu| + max|y|, |var|, |logp| + 1."""
    ce = float(f["cond"]) * EPS
    return dict(mu=float(np.max(np.abs(mu - f["mu"]) / (np.abs(f["mu"]) + np.abs(f["y"]).max())) / ce),
                var=float(np.max(np.abs(var - f["var"]) / np.abs(f["var"])) / ce),
                logp=float(np.max(np.abs(logp - f["logp"]) / (np.abs(f["logp"]) + 1.0)) / ce))


def check_vectors(f, mu, var, logp):
    tol, _ = loo_ref.ladder_tolerances(float(f["cond"]))
    ymax = np.abs(f["y"]).max()
    rtol = max(tol, 1e-7)
    np.testing.assert_allclose(mu, f["mu"], rtol=rtol, atol=max(tol * ymax, 1e-9 * max(np.abs(f["mu"]).max(), ymax)))
    np.testing.assert_allclose(var, f["var"], rtol=rtol, atol=1e-9 * np.abs(f["var"]).max())
    np.testing.assert_allclose(logp, f["logp"], rtol=rtol, atol=max(tol, 1e-9 * np.abs(f["logp"]).max()))


@pytest.mark.parametrize("kernel,D,N,s,b", loo_ref.RUNGS)
def test_rung(ctx, illcond, kernel, D, N, s, b):
    name = loo_ref.rung_name(kernel, D, N, s, b)
    f = illcond[name]
    X, y, theta = f["X"], f["y"], f["theta"]
    cond = float(f["cond"])
    tol, gtol = loo_ref.ladder_tolerances(cond)
    h = sls().Nll(ctx, X, kernel)
    try:
        r = h.loo(y, theta, b)
        r2 = h.loo(y, theta, b)
        rv = h.loo(y, theta, b, want_grad=False)
    finally:
        h.close()
    gps = {}
    for mode in (sls().SIGMA_EXPLICIT_INVERSE, sls().SIGMA_CHOLESKY_SOLVE):
        gp = sls().GP(ctx, X, y, theta, b, kernel)
        try:
            gp.set_sigma_mode(mode)
            gps[mode] = gp.loo()
        finally:
            gp.close()
    # measured first, asserted after: the record holds every figure of a rung that fails
    want_g = np.concatenate([f["grad_theta"], [float(f["grad_b"])]])
    got_g = np.concatenate([r["grad_theta"], [r["grad_b"]]])
    gscale = np.abs(want_g).max()
    sum_abs = float(np.sum(np.abs(f["logp"])))
    mult = vector_multiples(f, r["mu"], r["var"], r["logp"])
    mult["L"] = abs(r["value"] - float(f["L"])) / (cond * EPS * sum_abs)
    mult["grad"] = float(np.max(np.abs(got_g - want_g)) / (cond * EPS * gscale))
    gp_mult = {("explicit_inverse" if mode == sls().SIGMA_EXPLICIT_INVERSE else "cholesky_solve"): vector_multiples(f, *g)
               for mode, g in gps.items()}
    record("loo_conditioning", rung=name, kernel=kernel, D=D, N=N, s=s, b=b, cond=cond, bound_multiples=dict(vectors=10, L=10, grad=100),
           nll_loo=mult, gp_loo=gp_mult)
    print(name, "cond %.3g" % cond, "multiples of cond eps:", mult, gp_mult)
    check_vectors(f, r["mu"], r["var"], r["logp"])
    assert abs(r["value"] - float(f["L"])) <= max(tol * sum_abs, 1e-9 * abs(float(f["L"])))
    assert np.all(np.abs(got_g - want_g) <= np.maximum(gtol * gscale, 1e-6 * np.abs(want_g) + 1e-6 * gscale)), (got_g, want_g)
    assert same_bits(r, r2) and same_bits(r, rv, grad=False)
    for g in gps.values():
        check_vectors(f, *g)
