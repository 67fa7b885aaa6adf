"""Which code a handle runs on either side of D = 128, asserted from the context's launch counters, and the MAP fits just above it.

WAVE_PATH_MAX_D = NLL_SMALL_MAX_D = 128 (csrc/kernels.hpp): at D = 129 a small handle (N = 90) takes the tiled pipeline even for one
point or one start, every gradient goes through the 128-column tiles of grad_gemm (two of them), and the single-launch MAP fits
refuse, so that the host layer runs its own optimiser on sls_gp_nll_batch / sls_gp_nll_grad / sls_pref_objective.  The wide cases
of the other modules rest on these premises; here they are checked, so that a change of a limit cannot silently move those cases
back onto the code the D <= 128 tests already run."""
import ctypes as C
import os

import numpy as np
import pytest

import gram_ref as gr
from test_gpu_short_length_scales import random_prefs
from util import env_switch, record, sls, synth_clustered_ard_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ELL = 90, 3.4                                        # 0.3 sqrt(129): a dense problem on both sides of the limit
EI = 0
COUNTERS = ("acq_wave", "grad_gemm")


def calls(gp, r):
    """name -> call, for the five evaluation shapes whose route depends on D."""
    return {"predict": lambda: gp.predict(r["Xs"]),
            "predict_grad": lambda: gp.predict_grad(r["Xs"]),
            "ei_value_and_gradient": lambda: gp.acq_eval(r["Xs"], EI),
            "ei_value_only": lambda: (gp.acq_eval(r["Xs"], EI, want_grad=False),),
            "maximize_3_starts": lambda: tuple(gp.acq_maximize(r["Xs"][:, :3], 5)[k] for k in ("index", "x", "value", "x_stars", "y_stars"))}


def launch_counts(m, r, kernel):
    c = m.Context(0)
    c.prof_enable(True)
    gp = m.GP(c, r["X"], r["y"], r["theta"], r["b"], kernel)
    out = {}
    try:
        for name, call in calls(gp, r).items():
            c.prof_reset()
            call()
            out[name] = {k: c.prof_get(k)[1] for k in COUNTERS}
    finally:
        gp.close()
        c.close()
    return out


@pytest.mark.parametrize("kernel", [0, 1])
def test_d128_takes_the_wave_route_and_d129_does_not(kernel):
    """N = 90: every evaluation shape launches the one-wavefront kernels at D = 128 and none of them at D = 129, where each call
    that returns a gradient launches the tiled contraction instead."""
    m = sls()
    at128 = launch_counts(m, gr.reference(N, 128, ELL, kernel), kernel)
    at129 = launch_counts(m, gr.reference(N, 129, ELL, kernel), kernel)
    record("wide_routes", kernel=kernel, launches_at_128=at128, launches_at_129=at129)
    for name in at128:
        assert at128[name]["acq_wave"] > 0, (name, at128[name])
        assert at129[name]["acq_wave"] == 0, (name, at129[name])
    for name in ("predict_grad", "ei_value_and_gradient", "maximize_3_starts"):
        assert at129[name]["grad_gemm"] > 0, (name, at129[name])


@pytest.mark.parametrize("kernel", [0, 1])
def test_wave_switch_is_inert_at_d129(kernel):
    """SLS_WAVE_PATH = 0 and 1 give the same bits at D = 129: there is one route."""
    m = sls()
    r = gr.reference(N, 129, ELL, kernel)
    c = m.Context(0)
    res = {}
    try:
        for v in (0, 1):
            with env_switch("SLS_WAVE_PATH", v):
                gp = m.GP(c, r["X"], r["y"], r["theta"], r["b"], kernel)
                res[v] = {name: call() for name, call in calls(gp, r).items()}
                gp.close()
    finally:
        c.close()
    for name in res[0]:
        for a, b in zip(res[0][name], res[1][name]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), name


# ---- the MAP fits at N = 30, D = 129 --------------------------------------------------------------------------------------------------
N_FIT, D_FIT = 30, 129


def fit_problem(oracle):
    """Clustered points (util.synth_clustered_ard_problem): at the prior's length scale K_y has off-diagonal structure in 129
    dimensions, so that the likelihood's gradient is there in every row."""
    X, y, _ = synth_clustered_ard_problem(oracle, D_FIT, N_FIT)
    return np.asfortranarray(X), np.ascontiguousarray(y), random_prefs(np.random.default_rng(N_FIT + D_FIT), N_FIT, N_FIT // 2)


@pytest.fixture(scope="module")
def ctx():
    c = sls().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    sls().lib()
    lib = C.CDLL(os.path.join(ROOT, "sequential-line-search_amd", "libsequential-line-search.so"))
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint)
    lib.slsh_gp_map_fit.argtypes = [dp, C.c_int, C.c_int, dp, C.c_int, dp, dp]
    lib.slsh_pref_map_fit.argtypes = [dp, C.c_int, C.c_int, up, ip, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_uint, C.c_int, dp, dp, dp]
    lib.slsh_last_error.restype = C.c_char_p
    return lib


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def test_single_launch_map_fits_refuse_d129(ctx, oracle):
    """sls_pref_map_fit and sls_gp_map_fit at (N = 30, D = 129): SLS_ERR_UNSUPPORTED, by D alone."""
    m = sls()
    X, y, prefs = fit_problem(oracle)
    n = N_FIT + D_FIT + 2
    h = m.Nll(ctx, X, 1)
    try:
        with pytest.raises(m.Unsupported):
            h.pref_map_fit(prefs, np.zeros(n), np.full(n, -10.0), np.full(n, 2.0), 10, use_map=True)
        with pytest.raises(m.Unsupported):
            h.pref_map_fit(prefs, np.zeros(N_FIT), np.full(N_FIT, -10.0), np.full(N_FIT, 10.0), 10)
        with pytest.raises(m.Unsupported):
            h.gp_map_fit(y, np.zeros(D_FIT + 2), np.full(D_FIT + 2, -18.0), np.full(D_FIT + 2, 3.9), 10)
    finally:
        h.close()


@pytest.mark.parametrize("kernel", [0, 1])
def test_host_gp_map_fit_falls_back_to_the_tiled_objective(ctx, host, oracle, kernel):
    """GaussianProcessRegressor(X, y, kernel) at N = 30, D = 129: DIRECT on sls_gp_nll_batch and the local phase on sls_gp_nll_grad,
    both on the tiled pipeline at Np = 128 with two column tiles.  The fit completes, does not end below the prior medians it starts
    from (the oracle's objective there), and sls_gp_nll_grad at the returned point is the oracle's objective and gradient to the
    tolerance of test_gp_map_objective_and_gradient."""
    X, y, _ = fit_problem(oracle)
    x, st = np.zeros(D_FIT + 2), np.zeros(8)
    rc = host.slsh_gp_map_fit(_p(X), D_FIT, N_FIT, _p(np.ascontiguousarray(y)), kernel, _p(x), _p(st))
    assert rc == 0, host.slsh_last_error()
    assert np.all(np.isfinite(x)) and np.all(x > 0)
    start = np.concatenate([[0.5, 1e-4], np.full(D_FIT, 0.5)])
    v0, _ = oracle.gp_map_objective(kernel, X, y, start)
    vo, go = oracle.gp_map_objective(kernel, X, y, x)
    h = sls().Nll(ctx, X, kernel)
    v, g = h.gp_objective(y, x)
    h.close()
    record("wide_routes", route="host_gp_map_fit", kernel=kernel, start=float(v0), final=float(st[0]), oracle_final=float(vo),
           evals_direct=int(st[3]), evals_local=int(st[4]), seconds=float(st[5]),
           errors=gr.errors(dict(map_value=v, map_grad=g), dict(map_value=vo, map_grad=go)))
    assert vo >= v0 and st[0] >= v0 - 1e-8 * max(1.0, abs(v0)), (v0, vo, st[0])
    gr.check(dict(map_value=v, map_grad=g), dict(map_value=vo, map_grad=go), D_FIT, 1.0)
    gr.check(dict(map_value=st[0]), dict(map_value=vo), D_FIT, 1.0)


@pytest.mark.parametrize("kernel", [0, 1])
def test_host_preference_map_fit_falls_back_to_the_tiled_objective(ctx, host, oracle, kernel):
    """PreferenceRegressor with MAP hyper-parameters at M = 30, D = 129 (the reference's 100 evaluations): the host optimiser on
    sls_pref_objective.  The fit completes, does not end below its start (y = 0 at the default hyper-parameters), and
    sls_pref_objective at the returned point is the oracle's objective and gradient."""
    X, _, prefs = fit_problem(oracle)
    flat = np.array([i for p in prefs for i in p], dtype=np.uint32)
    offs = np.zeros(len(prefs) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(p) for p in prefs])
    yv, hyp, obj = np.zeros(N_FIT), np.zeros(D_FIT + 2), C.c_double(0.0)
    rc = host.slsh_pref_map_fit(_p(X), D_FIT, N_FIT, _p(flat, C.c_uint), _p(offs, C.c_int), len(prefs), 1, 0.5, 0.5, 0.005, 0.25, 0.01,
                                100, kernel, _p(yv), _p(hyp), C.byref(obj))
    assert rc == 0, host.slsh_last_error()
    assert np.all(np.isfinite(yv)) and np.all(np.isfinite(hyp)) and np.all(hyp > 0)
    start = np.concatenate([np.zeros(N_FIT), [0.5, 0.005], np.full(D_FIT, 0.5)])
    x = np.concatenate([yv, hyp])
    v0, _ = oracle.pref_objective(kernel, X, prefs, start, use_map=True)
    vo, go = oracle.pref_objective(kernel, X, prefs, x, use_map=True)
    h = sls().Nll(ctx, X, kernel)
    v, g = h.pref_objective(prefs, x, use_map=True)
    h.close()
    record("wide_routes", route="host_pref_map_fit", kernel=kernel, start=float(v0), final=float(obj.value), oracle_final=float(vo),
           errors=gr.errors(dict(map_value=v, map_grad=g), dict(map_value=vo, map_grad=go)))
    assert vo >= v0 and obj.value >= v0 - 1e-8 * max(1.0, abs(v0)), (v0, vo, obj.value)
    gr.check(dict(map_value=v, map_grad=g), dict(map_value=vo, map_grad=go), D_FIT, 1.0)
    gr.check(dict(map_value=obj.value), dict(map_value=vo), D_FIT, 1.0)
