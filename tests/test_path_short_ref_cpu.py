"""The reference of the path, set-criterion and EUBO tests beyond the Gram guard (tests/path_short_ref.py) is its own proof, the way
tests/test_gram_ref_cpu.py argues for gram_ref: inside the guard it is the restatement the path tests already use; beyond it that
restatement's kernel misses the near-duplicate entries this one gets right; its float64 form stays within a finite, recorded band of
its longdouble form on every case of tests/test_gpu_short_length_scales_paths.py; and on every case at most 10 % of the sets lose
their place in the comparison of winners to a margin below 100 value tolerances."""
import numpy as np
import pytest

import eubo_ref
import gram_ref as gr
import line_ref as lr
import path_ref as ph
import path_short_ref as sr
import qeubo_ref as qr

KERNELS = [0, 1]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N,D", sr.SIZES)
def test_inside_the_guard_it_is_the_restatement_of_the_path_tests(N, D, kernel):
    inside_the_guard(N, D, 0.3, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N,D,case", gr.WIDE_DENSE)
def test_wide_dense_cases_are_the_restatement_of_the_path_tests(N, D, case, kernel):
    """D = 129, 192, 257 at l = 0.3 sqrt(D): inside the guard, the same assertions."""
    inside_the_guard(N, D, case, kernel)


def inside_the_guard(N, D, case, kernel):
    """l = 0.3 (0.3 sqrt(D) at D > 128): values to the 1e-8 and gradients to the 1e-6 (1 + |g|max) of tests/test_path_sample_cpu.py, against
    path_ref.PathRef; qEUBO, a line and the EUBO pairs against qeubo_ref / line_ref on that PathRef and eubo_ref.eubo."""
    r = sr.reference(N, D, case, kernel)
    assert not sr.beyond_guard(r["ell"], D)
    ref, q64, Xs = r["ref64"], r["q64"], r["Xs"]
    old = ph.PathRef(r["X"], r["y"], r["theta"], r["b"], kernel, r["nd"], sr.F, seed=r["seed"])
    dr = sr.draws_of_points(Xs.shape[1], r["nd"])
    ov, og = old.eval(Xs, dr)
    assert np.abs(ref.v - old.v).max() <= 1e-8 * max(1.0, np.abs(old.v).max())
    assert np.abs(q64["val"] - ov).max() <= 1e-8 and np.abs(q64["all"] - old.eval_all(Xs)).max() <= 1e-8
    assert np.abs(q64["grad"] - og).max() <= 1e-6 * (1 + np.abs(og).max())
    assert np.abs(q64["val_prior"] + q64["val_data"] - q64["val"]).max() <= 1e-14
    sets = sr.sets_of(Xs, 5)
    oq = qr.qeubo(old, sets, 5)
    assert np.abs(q64["qeubo5_val"] - oq[0]).max() <= 1e-8 and np.array_equal(q64["qeubo5_wins"], oq[2])
    assert np.abs(q64["qeubo5_grad"] - oq[1]).max() <= 1e-6 * (1 + np.abs(oq[1]).max())
    for anchored in (False, True):
        lines, anchor = sr.lines_of(Xs, anchored)
        new_l, old_l = lr.line(ref, lines, sr.LINE_Q, anchor), lr.line(old, lines, sr.LINE_Q, anchor)
        assert np.abs(new_l[0] - old_l[0]).max() <= 1e-8 and np.array_equal(new_l[2], old_l[2])
        assert np.abs(new_l[1] - old_l[1]).max() <= 1e-6 * (1 + np.abs(old_l[1]).max())
    e = sr.eubo_reference(N, D, case, kernel)
    rv, rg, info = eubo_ref.eubo(r["X"], r["y"], r["theta"], r["b"], kernel, e["pairs"])
    assert not info["bad"].any() and not e["e64"][2]["bad"].any()
    assert np.abs(e["e64"][0] - rv).max() <= 1e-8 and np.abs(e["e64"][1] - rg).max() <= 1e-6 * (1 + np.abs(rg).max())


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N,D", sr.SIZES)
def test_beyond_the_guard_the_old_kernel_misses_the_near_duplicate_entries(N, D, kernel):
    """l = 1e-5: the ten candidates at q ~ 0.5 from a training point.  path_ref.kernel_c (norm expansion) violates the
    4 (D + 8) eps a of gram_ref on exactly those entries; the new float64 form holds it against longdouble."""
    r = sr.reference(N, D, 1e-5, kernel)
    assert sr.beyond_guard(r["ell"], D)
    near = list(gr.CAND_NEAR)
    rows = [41 + 3 * k for k in range(len(near))]
    k80, c80 = r["ref80"].kc(r["Xs"])
    assert np.all((k80[near, rows] > 0.3 * gr.A) & (k80[near, rows] < 0.99 * gr.A))          # neither 0 nor a
    tol = gr.gram_tolerance(D)
    for which, exact in ((0, k80), (1, c80)):
        new = r["ref64"].kc(r["Xs"])[which]
        old = ph.kernel_c(r["Xs"], r["X"], r["theta"], kernel)[which]
        assert np.abs(new - exact).max() <= tol
        assert np.abs(old - exact)[near, rows].min() > tol


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N,D,case,nd", sr.CASES)
def test_band_is_finite_and_the_winner_margins_keep_nine_sets_in_ten(N, D, case, nd, kernel):
    r = sr.reference(N, D, case, kernel, nd)
    band = sr.band(N, D, case, kernel, nd)
    for k in ("val", "grad", "all", "v", "t", "val_prior", "val_data", "grad_prior", "grad_data"):
        assert k in band
    for q in sr.QS:
        for name in ("qeubo", "qnei"):
            assert f"{name}{q}_val" in band and f"{name}{q}_grad" in band
    assert all(np.isfinite(b) for b in band.values()), band
    assert all(np.isfinite(t) and t > 0 for t in r["tol"].values())
    # a band is rounding, not disagreement: within 1e-6 of the quantity's own size
    for k, b in band.items():
        assert b <= 1e-6 * max(1.0, float(np.abs(r["q80"][k]).max())), (k, b)
    # the identity at the data on the reference itself, to its own band
    ref = r["ref80"]
    assert np.abs(ref.eval_all(r["X"]) - ref.data_identity()).max() <= 1e-6
    for k, kept in r["kept"].items():
        assert (~kept).mean() <= sr.MAX_DROPPED, (k, float((~kept).mean()), r["margin"])
    if nd == 5:
        e = sr.eubo_reference(N, D, case, kernel)
        assert np.isfinite(e["band"]["val"]).all() and np.isfinite(e["band"]["grad"]).all()
        assert not e["e80"][2]["bad"].any() and e["e80"][2]["s"].min() >= 1e-3
