"""Where a predict / acquisition call changes route (csrc/capi.hip: eval_entry).

A call of sls_gp_predict, sls_gp_predict_grad or sls_acq_eval takes one of four routes: a slot of the context (<= 64 points, no
context lock), the zero-copy block (value-only acquisition), the one-wavefront kernels behind a staged or pageable upload
(Np <= 512, <= 4096 points), or the tiled pipeline.  The first three run the SAME kernel on the same points, so at equal M their
results are equal bit for bit whatever the switches say; the tiled pipeline agrees to rounding.  The cases sit on the limits:
M = 64 / 65 (slot), 4096 / 4097 (wave path), Np = 512 -> 640 (a handle that leaves the wave path while in use), omitted outputs,
M = 0.  (src/acquisition-function.cpp:125-165: Predict* / the acquisition value of one regressor, point by point and in batches.)"""
import contextlib

import numpy as np
import pytest

from util import env_switch, sls, synth_candidates, synth_problem

pytestmark = pytest.mark.gpu

D, N = 5, 90
UCB_H = 2.0
TOL = dict(rtol=1e-6, atol=1e-9)      # test_gpu_concurrency.py: device against the oracle's batched predict


@contextlib.contextmanager
def switches(**kv):
    with contextlib.ExitStack() as st:
        for k, v in kv.items():
            st.enter_context(env_switch(k, v))
        yield


def all_calls(gp, Q):
    """Every form of the three entry points the Python binding can make, as a dict of tuples of arrays."""
    m = sls()
    return {
        "predict": gp.predict(Q),
        "predict_grad": gp.predict_grad(Q),
        "ei": gp.acq_eval(Q, m.ACQ_EI),
        "ucb": gp.acq_eval(Q, m.ACQ_UCB, UCB_H),
        "ei_value": (gp.acq_eval(Q, m.ACQ_EI, want_grad=False),),
        "ucb_value": (gp.acq_eval(Q, m.ACQ_UCB, UCB_H, want_grad=False),),
    }


def assert_same_bits(a, b, label):
    assert a.keys() == b.keys()
    for name in a:
        assert len(a[name]) == len(b[name])
        for k, (u, v) in enumerate(zip(a[name], b[name])):
            assert u.shape == v.shape and np.array_equal(u, v), f"{label}: {name}[{k}] differs"


@pytest.fixture(scope="module")
def ctx():
    c = sls().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def problem(oracle):
    X, y, theta, b = synth_problem(oracle, D, N)
    return X, y, theta, b, synth_candidates(oracle, D, 4097)


@pytest.fixture(scope="module")
def handles(ctx, oracle, problem):
    """sigma mode -> (device handle, oracle regressor of the same class, 4097 query points)"""
    X, y, theta, b, Q = problem
    out = {}
    for mode in (0, 1):
        gp = sls().GP(ctx, X, y, theta, b, sls().KERNEL_MATERN52)
        gp.set_sigma_mode(mode)
        out[mode] = (gp, oracle.Regressor(X, y, theta, b, kernel=oracle.KERNEL_MATERN52, reg_type=mode), Q)
    yield out
    for gp, _, _ in out.values():
        gp.close()


@pytest.fixture(params=[0, 1], ids=["explicit_inverse", "cholesky_solve"])
def handle(request, handles):
    return handles[request.param]


@pytest.mark.parametrize("M", [1, 64, 65])
def test_slot_limit_same_bits_on_every_route(handle, M):
    """M = 64 is the last size a slot takes, 65 the first that takes the context's lock; value-only calls go through the zero-copy
    block at 65.  Same kernel, same points: the same bits as with each fast route switched off."""
    gp, _, Qall = handle
    Q = Qall[:, 100:100 + M]
    default = all_calls(gp, Q)
    with switches(SLS_EVAL_SLOTS=0):
        assert_same_bits(default, all_calls(gp, Q), f"M={M} SLS_EVAL_SLOTS=0")
    value_only = {k: v for k, v in default.items() if k.endswith("_value")}
    for sw in (dict(SLS_EVAL_ZEROCOPY=0), dict(SLS_IO_STAGE=0), dict(SLS_EVAL_SLOTS=0, SLS_EVAL_ZEROCOPY=0),
               dict(SLS_EVAL_SLOTS=0, SLS_EVAL_ZEROCOPY=0, SLS_IO_STAGE=0)):
        with switches(**sw):
            got = all_calls(gp, Q)
        assert_same_bits(value_only, {k: got[k] for k in value_only}, f"M={M} {sw}")
    with switches(SLS_EVAL_SLOTS=0, SLS_IO_STAGE=0):      # the pageable upload in front of the same kernel
        assert_same_bits(default, all_calls(gp, Q), f"M={M} SLS_EVAL_SLOTS=0 SLS_IO_STAGE=0")


def against_oracle(got, ref, Q, cols, label):
    """The columns `cols` of a device result against the oracle's batched forms."""
    m = sls()
    Qc = Q[:, cols]
    want = {
        "predict": ref.predict_batch(Qc),
        "predict_grad": ref.predict_grad_batch(Qc),
        "ei": ref.acq_eval_batch(Qc, m.ACQ_EI),
        "ucb": ref.acq_eval_batch(Qc, m.ACQ_UCB, UCB_H),
    }
    want["ei_value"], want["ucb_value"] = (want["ei"][0],), (want["ucb"][0],)
    for name, arrays in want.items():
        for k, w in enumerate(arrays):
            np.testing.assert_allclose(got[name][k][..., cols], w, err_msg=f"{label}: {name}[{k}]", **TOL)


def test_wave_path_limit_against_the_oracle(handle):
    """4096 points are the last batch of the one-wavefront kernels, 4097 the first of the tiled pipeline: both agree with the
    oracle (first and last 64 points), and the tiled pipeline at 4096 agrees with the wave path."""
    gp, ref, Qall = handle
    res = {}
    for M in (4096, 4097):
        Q = Qall[:, :M]
        res[M] = all_calls(gp, Q)
        cols = np.r_[0:64, M - 64:M]
        against_oracle(res[M], ref, Q, cols, f"M={M}")
    with switches(SLS_WAVE_PATH=0):
        tiled = all_calls(gp, Qall[:, :4096])
    for name, arrays in res[4096].items():
        for k, w in enumerate(arrays):
            np.testing.assert_allclose(tiled[name][k], w, err_msg=f"SLS_WAVE_PATH=0: {name}[{k}]", **TOL)


def test_handle_that_leaves_the_wave_path_while_in_use(ctx, oracle):
    """N = 512 fills Np = 512; one appended point makes Np = 640, past the one-wavefront kernels.  The single-point calls before
    and after agree with the oracle on the same data; the call after is the one a slot declines under the state lock, and it
    returns the bits of the locked route."""
    Dl, Nl = 4, 512
    X, y, theta, b = synth_problem(oracle, Dl, Nl)
    x_new, y_new = synth_candidates(oracle, Dl, 1, seed=77)[:, 0], 0.3
    q = synth_candidates(oracle, Dl, 1, seed=78)
    gp = sls().GP(ctx, X, y, theta, b, sls().KERNEL_MATERN52)
    try:
        before = all_calls(gp, q)
        against_oracle(before, oracle.Regressor(X, y, theta, b, kernel=oracle.KERNEL_MATERN52), q, np.r_[0:1], "Np=512")
        gp.append_point(x_new, y_new)
        after = all_calls(gp, q)
        X1, y1 = np.concatenate([X, x_new[:, None]], axis=1), np.concatenate([y, [y_new]])
        against_oracle(after, oracle.Regressor(X1, y1, theta, b, kernel=oracle.KERNEL_MATERN52), q, np.r_[0:1], "Np=640")
        with switches(SLS_EVAL_SLOTS=0):
            assert_same_bits(after, all_calls(gp, q), "Np=640 SLS_EVAL_SLOTS=0")
    finally:
        gp.close()


@pytest.mark.parametrize("mode,M,sw", [
    (0, 3, {}), (1, 3, {}),
    (1, 200, dict(SLS_WAVE_PATH=0)),
    (0, 200, dict(SLS_WAVE_PATH=0, SLS_TRI_PREDICT=0)), (1, 200, dict(SLS_WAVE_PATH=0, SLS_TRI_PREDICT=0)),
], ids=["slot-explicit_inverse", "slot-cholesky_solve", "tiled-cholesky_solve", "tiled_kinv-explicit_inverse", "tiled_kinv-cholesky_solve"])
def test_omitted_gradient_leaves_the_value_unchanged(handles, mode, M, sw):
    """The binding can omit one output, the acquisition's gradient (want_grad=False); mu / sigma / dmu / dsigma cannot be omitted
    from Python.  The values are the same bits with and without the gradient wherever both calls take sigma from the same
    kernel: on the slot route (M = 3), and on the tiled pipeline (M = 200, SLS_WAVE_PATH=0) in Cholesky-solve mode, where sigma
    is |L^-1 k|^2 from var_gemm in both calls (csrc/capi.hip: eval_candidates).  In explicit-inverse mode the tiled value-only
    call takes that triangular contraction BY DESIGN (SLS_TRI_PREDICT, half the flops) while the gradient needs k.K^-1 k from
    acq_gemm: two roundings of sigma, no promise of equal bits -- there the pair is compared with SLS_TRI_PREDICT=0, which
    sends both through acq_gemm."""
    gp, _, Qall = handles[mode]
    Q = Qall[:, 500:500 + M]
    with switches(**sw):
        got = all_calls(gp, Q)
    assert np.array_equal(got["ei"][0], got["ei_value"][0])
    assert np.array_equal(got["ucb"][0], got["ucb_value"][0])


def test_no_points_is_not_an_error(handle):
    gp, _, Qall = handle
    got = all_calls(gp, Qall[:, :0])
    assert all(a.size == 0 for arrays in got.values() for a in arrays)
    assert got["predict"][0].shape == (0,) and got["predict_grad"][0].shape == (D, 0) and got["ei"][1].shape == (D, 0)
