"""The reference of the short-length-scale GPU tests (gram_ref.py) is its own proof: its fp64 form stays within the tests'
tolerances of its longdouble form on every case those tests use, and an fp64 emulation of the norm expansion -- the arithmetic
form of the matrix-core Gram kernels -- violates them at l <= 1e-5 on the same cases, so the cases can fail."""
import numpy as np
import pytest

import gram_ref as gr

CASES = [(N, D, case) for (N, D) in gr.SIZES for case in gr.ELL_CASES]


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case", CASES)
def test_fp64_direct_differences_agree_with_longdouble_and_the_expansion_does_not(oracle, N, D, case, kernel):
    r64 = gr.reference(N, D, case, kernel)
    y_max = float(np.abs(r64["y"]).max())
    q64 = gr.quantities(r64)
    qld = gr.quantities(gr.reference(N, D, case, kernel, np.longdouble))
    gr._CACHE.pop((N, D, case, kernel, np.longdouble, False))      # 72 longdouble records would be ~100 MB
    gr.check(q64, qld, D, y_max)
    # the table of the issue: with a = 0.7, b = 5e-3 the fp64 form is within 1e-13 of longdouble on K, alpha and log|K_y|
    e = gr.errors(q64, qld)
    assert e["K"]["max_abs"] <= 1e-13 * gr.A and e["alpha"]["max_abs"] <= 1e-13 * e["alpha"]["scale"]
    assert e["logdet"]["max_abs"] <= 1e-13 * max(1.0, e["logdet"]["scale"])
    # the oracle's MAP objective forms differences too: the same value and gradient
    vo, go = oracle.gp_map_objective(kernel, r64["X"], r64["y"], r64["hyp"])
    gr.check(dict(map_value=vo, map_grad=go), qld, D, y_max)
    if case in (1e-5, 1e-8, "ard"):
        qex = gr.quantities(gr.reference(N, D, case, kernel, expansion=True))
        gr._CACHE.pop((N, D, case, kernel, np.float64, True))
        for key in ("K", "Ks", "alpha", "logdet"):
            with pytest.raises(AssertionError):
                gr.check({key: qex[key]}, qld, D, y_max)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,D,case", gr.WIDE_CASES)
def test_wide_cases_fp64_agrees_with_longdouble(oracle, N, D, case, kernel):
    """D > 128 (gram_ref.WIDE_CASES): the fp64 form within every tolerance of check() of its longdouble form, the gradients of mean
    and deviation included, and the oracle's MAP objective with it; beyond the guard the emulated expansion fails on K_y."""
    r64 = gr.reference(N, D, case, kernel)
    y_max = float(np.abs(r64["y"]).max())
    q64 = gr.quantities(r64)
    qld = gr.quantities(gr.reference(N, D, case, kernel, np.longdouble))
    gr.check(q64, qld, D, y_max)
    for k in ("dmean", "ddev", "ucb_grad", "ei_grad"):           # every gradient row, 128 and up included, is live at some candidate
        rows = np.abs(qld[k]).max(axis=1)
        assert rows.min() > (1e-3 * rows.max() if (N, D, case) in gr.WIDE_DENSE else 0.0), k
    assert np.abs(qld["map_grad"][2:]).min() > 0
    vo, go = oracle.gp_map_objective(kernel, r64["X"], r64["y"], r64["hyp"])
    gr.check(dict(map_value=vo, map_grad=go), qld, D, y_max)
    if (N, D, case) not in gr.WIDE_DENSE:
        qex = gr.quantities(gr.reference(N, D, case, kernel, expansion=True))
        gr._CACHE.pop((N, D, case, kernel, np.float64, True))
        with pytest.raises(AssertionError):
            gr.check(dict(K=qex["K"]), qld, D, y_max)
