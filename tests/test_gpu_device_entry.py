"""The device-pointer entry points of the C ABI -- sls_ctx_set_stream, sls_ctx_synchronize, sls_gp_refit_dev, sls_acq_maximize_dev
(csrc/capi.hip) -- the sequence bench.py times and the documented way to drive the library from PyTorch without a host round trip.

sls_gp_create and sls_gp_refit_dev both end in gp_fit_device on the same device inputs, and the fit is deterministic: a handle
refitted in place must hold THE SAME BITS as a fresh handle made from host pointers on the same context.  The one sanctioned
exception is the project's own (test_gpu_bench.py): when a single-launch factorisation gave up during the case
(ctx.prof_get("potrf_fallbacks") moved) the comparison is rtol = 1e-11, atol = 1e-12.  Correctness is held to the CPU oracle at the
tolerance of test_gpu_eval_routes.py.  Device buffers are torch tensors, as in bench.py: X (D x N, one point per column) is the
C-ordered N x D tensor of its transpose."""
import ctypes as C

import numpy as np
import pytest
import torch      # before libsls_hip.so is loaded, as in bench.py: the library then binds to the HIP runtime torch brought, and the two share one

from util import relerr, sls, synth_candidates, synth_problem

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-6, atol=1e-9)       # test_gpu_eval_routes.py: device against the oracle's batched forms
SEED_A, SEED_B = 1234, 4321            # two data sets; the oracle (CPU) gives them different best_index (N > 1) and mu_best at every shape used here
UCB_H = 2.0
Y_STAR = np.array([0.95, 1.0, 1.02, 1.05, 1.1, 1.2, 1.4])    # K = 7 samples of the maximum value for sls_mes_eval
N_QUERY = 233                          # 200 points for the pointwise calls, 33 more for the joint ones


def dev_matrix(A):
    """D x M column-major (one point per column) as a device tensor: M x D in C order."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(A, dtype=np.float64).T)).to("cuda")


def dev_vector(v):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64))).to("cuda")


class DevData:
    """(X, y) resident on the device; keeps the tensors referenced for as long as the object lives."""

    def __init__(self, X, y):
        self.X, self.y = dev_matrix(X), dev_vector(y)

    def refit(self, gp):
        gp.refit_dev(self.X.data_ptr(), self.y.data_ptr())


_problems = {}


def problem(oracle, D, N, seed):
    key = (D, N, seed)
    if key not in _problems:
        _problems[key] = synth_problem(oracle, D, N, seed=seed)
    return _problems[key]


def queries(oracle, D):
    key = ("q", D)
    if key not in _problems:
        _problems[key] = synth_candidates(oracle, D, N_QUERY)
    return _problems[key]


@pytest.fixture(scope="module")
def ctx():
    c = sls().Context(0)
    yield c
    c.close()


class Fallbacks:
    """Did a single-launch factorisation give up since this object was made?  Then the two schedules agree to rounding only."""

    def __init__(self, ctx):
        self.ctx, self.at_start = ctx, ctx.prof_get("potrf_fallbacks")[1]

    def none(self):
        return self.ctx.prof_get("potrf_fallbacks")[1] == self.at_start


def assert_same(a, b, fb, label):
    """Two dicts name -> tuple of arrays: the same bits (or, behind a factorisation fall-back, the rule of test_gpu_bench.py)."""
    assert a.keys() == b.keys()
    exact = fb.none()
    for name in a:
        assert len(a[name]) == len(b[name])
        for k, (u, v) in enumerate(zip(a[name], b[name])):
            u, v = np.asarray(u), np.asarray(v)
            assert u.shape == v.shape, f"{label}: {name}[{k}] shape {u.shape} vs {v.shape}"
            if exact:
                assert np.array_equal(u, v), f"{label}: {name}[{k}] differs by up to {float(np.max(np.abs(u - v))):.3e}"
            else:
                np.testing.assert_allclose(u, v, rtol=1e-11, atol=1e-12, err_msg=f"{label}: {name}[{k}] (after a potrf fall-back)")


def pointwise(gp, Q, M):
    m = sls()
    q = Q[:, :M]
    return {f"predict[{M}]": gp.predict(q), f"predict_grad[{M}]": gp.predict_grad(q),
            f"ei[{M}]": gp.acq_eval(q, m.ACQ_EI), f"ucb[{M}]": gp.acq_eval(q, m.ACQ_UCB, UCB_H)}


def snapshot(gp, Q):
    """Everything the C ABI shows of a fitted handle, as a dict name -> tuple of arrays."""
    m = sls()
    out = {name: (gp.matrix(sel),) for name, sel in (("K_y", m.GP_K_Y), ("K_y_inv", m.GP_K_Y_INV), ("L", m.GP_CHOL_L),
                                                      ("alpha", m.GP_ALPHA), ("mu_data", m.GP_MU_DATA))}
    s = gp.summary()
    out["summary"] = (np.array([s["best_index"], s["mu_best"], s["logdet"]]),)
    for M in (1, 65, 200):            # a slot of the context; past the slots; a second 128-block of candidates
        out.update(pointwise(gp, Q, M))
    q33 = Q[:, 200:233]
    out["predict_cov"] = gp.predict_cov(q33)
    F, jitter = gp.sample_posterior(q33, 4, 7)
    out["sample_posterior"] = (F, np.array([jitter]))
    out["mes"] = gp.mes_eval(Y_STAR, q33)
    ps = m.PathSamples(gp, 3, n_freq=64, seed=5)
    try:
        out["path"] = (ps.eval_all(q33),)
    finally:
        ps.close()
    return out


def assert_matches_oracle(snap, ref, Q, label):
    m = sls()
    want = {"predict": ref.predict_batch(Q[:, :200]), "predict_grad": ref.predict_grad_batch(Q[:, :200]),
            "ei": ref.acq_eval_batch(Q[:, :200], m.ACQ_EI), "ucb": ref.acq_eval_batch(Q[:, :200], m.ACQ_UCB, UCB_H)}
    for M in (1, 65, 200):
        for name, arrays in want.items():
            for k, w in enumerate(arrays):
                np.testing.assert_allclose(snap[f"{name}[{M}]"][k], w[..., :M], err_msg=f"{label}: {name}[{M}][{k}] against the oracle", **TOL)


def test_library_calls_leave_no_hip_error_for_the_caller(ctx, oracle):
    """The library and PyTorch share one HIP runtime and one thread: a HIP call of the library whose failure it tolerates must not
    leave that failure as the thread's last error, which PyTorch reads after each of its own launches and reports as its own
    ("HIP error: invalid argument": the refused LDS opt-in of the one-wavefront kernels did).  The first PyTorch launch of this module
    therefore also answers for every library call of the tests that ran before it in the same process."""
    m = sls()
    X, y, theta, b = problem(oracle, 3, 100, SEED_A)
    Q = queries(oracle, 3)
    gp = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
    try:
        for mode in (0, 1):
            gp.set_sigma_mode(mode)
            gp.predict(Q[:, :1])                                   # a slot: the one-wavefront kernel, evaluation only
            gp.acq_maximize(Q[:, :1], 5, want_all=False)           # one start: the cooperative form
            gp.acq_maximize(Q[:, :129], 5, want_all=False)         # the staged form
            assert float((torch.ones(8, device="cuda") * 2.0).sum().item()) == 16.0
    finally:
        gp.close()


# ---- 1. a refit in place equals a fresh fit, on every fit route ---------------------------------------------------------------------
# (D, N): smallest fit; single-workgroup fit at its limit; first tiled fit (Np = 256, separate launches); Np = 384, first fused
# factor-and-inverse launch; last / first size on / past the one-wavefront evaluation path; claimed tile pools (N >= 2432);
# D = 129: two 128-column tiles in every gradient behind the snapshot, no one-wavefront route
FIT_SHAPES = [(1, 1), (3, 128), (3, 129), (5, 300), (4, 512), (6, 640)]
FIT_CASES = [(D, N, k, mode) for D, N in FIT_SHAPES for k in (0, 1) for mode in (0, 1)] + [(6, 2560, 1, 0), (129, 130, 1, 0)]


@pytest.mark.parametrize("D,N,kernel,mode", FIT_CASES, ids=[f"D{D}-N{N}-{'matern' if k else 'se'}-{'solve' if mode else 'inverse'}"
                                                            for D, N, k, mode in FIT_CASES])
def test_refit_in_place_equals_a_fresh_fit(ctx, oracle, D, N, kernel, mode):
    """Handle created on A, sigma mode set, refitted with B: the bits of a fresh handle on B (sigma mode set after its creation) in
    every matrix, the summary and every evaluation; the oracle's numbers up to N = 640; a new generation; a path object made before
    the refit is refused.  Then refits with A, B, A: the first and the third state are the same bits.
    Precondition (else a refit that did nothing could pass): A and B have different mu_best and, where there is more than one data
    point to choose from, different best_index (at N = 1 the index is 0 whatever the data)."""
    m = sls()
    XA, yA, theta, b = problem(oracle, D, N, SEED_A)
    XB, yB, _, _ = problem(oracle, D, N, SEED_B)
    Q = queries(oracle, D)
    dA, dB = DevData(XA, yA), DevData(XB, yB)
    fb = Fallbacks(ctx)
    gp = m.GP(ctx, XA, yA, theta, b, kernel)
    fresh = m.GP(ctx, XB, yB, theta, b, kernel)
    old_path = None
    try:
        gp.set_sigma_mode(mode)
        fresh.set_sigma_mode(mode)
        sA, sB = gp.summary(), fresh.summary()
        assert sA["mu_best"] != sB["mu_best"] and (N == 1 or sA["best_index"] != sB["best_index"]), (sA, sB)
        old_path = m.PathSamples(gp, 2, n_freq=32, seed=1)
        old_path.eval(Q[:, :2], [0, 1])
        g0 = gp.generation()

        dB.refit(gp)
        assert gp.generation() != g0
        with pytest.raises(m.SlsError):
            old_path.eval(Q[:, :2], [0, 1])
        want = snapshot(fresh, Q)
        got = snapshot(gp, Q)
        assert_same(got, want, fb, "refit(B) against a fresh handle on B")
        if N <= 640:
            ref = oracle.Regressor(XB, yB, theta, b, kernel=kernel, reg_type=mode)
            assert_matches_oracle(got, ref, Q, f"D={D} N={N}")
            assert got["summary"][0][0] == ref.best_index()

        dA.refit(gp)
        first = snapshot(gp, Q)
        assert not np.array_equal(first["alpha"][0], got["alpha"][0])
        dB.refit(gp)
        assert_same(snapshot(gp, Q), want, fb, "refit A, B: the second state against a fresh handle on B")
        dA.refit(gp)
        assert_same(snapshot(gp, Q), first, fb, "refit A, B, A: third state against the first")
    finally:
        if old_path is not None:
            old_path.close()
        gp.close()
        fresh.close()


# ---- 2. the host copies are rebuilt from the device after a refit ----------------------------------------------------------------
def assert_grown_handle_agrees(oracle, gp, ref, X, y, theta, b, kernel):
    """The tolerances of test_append_point_equals_refit (test_gpu_parity.py): the rank-1 growth agrees with a refit to rounding."""
    m = sls()
    D = X.shape[0]
    # K_y is rebuilt from the handle's scaled copy of X by the same kernel in both handles: an elementwise function of the data
    np.testing.assert_allclose(gp.matrix(m.GP_K_Y), ref.matrix(m.GP_K_Y), rtol=1e-12, atol=0)
    Ki, Kr = gp.matrix(m.GP_K_Y_INV), ref.matrix(m.GP_K_Y_INV)
    assert relerr(Ki, Kr, floor=np.abs(Kr).max()) < 1e-9
    np.testing.assert_allclose(gp.matrix(m.GP_CHOL_L), ref.matrix(m.GP_CHOL_L), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(gp.matrix(m.GP_ALPHA), ref.matrix(m.GP_ALPHA), rtol=1e-6, atol=1e-7 * np.abs(y).max())
    sa, sb = gp.summary(), ref.summary()
    assert sa["best_index"] == sb["best_index"]
    np.testing.assert_allclose(sa["logdet"], sb["logdet"], rtol=1e-10)
    np.testing.assert_allclose(sa["mu_best"], sb["mu_best"], rtol=1e-8)
    Xs = synth_candidates(oracle, D, 33)
    for a_, b_ in zip(gp.acq_eval(Xs), ref.acq_eval(Xs)):
        np.testing.assert_allclose(a_, b_, rtol=1e-6, atol=1e-9 * max(np.abs(b_).max(), 1e-30))
    oref = oracle.Regressor(X, y, theta, b, kernel=kernel)
    np.testing.assert_allclose(gp.predict(Xs)[1], oref.predict_batch(Xs)[1], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N0", [5, 126, 128])
def test_append_after_refit_grows_the_refitted_data(ctx, oracle, kernel, N0):
    """sls_gp_refit_dev leaves the device copies of X, y authoritative; the next sls_gp_append_point rebuilds the host copies from
    them -- the copies the in-place growth re-uploads (N0 = 5, 126) and the rebuild at a full 128-block fits from (126 + 2, 128).  A
    handle that kept the data it was created from on the host fails every comparison below."""
    m = sls()
    D, extra = 3, 4
    XA, yA, theta, b = problem(oracle, D, N0, SEED_A)
    XB, yB, _, _ = problem(oracle, D, N0 + extra, SEED_B)
    dB = DevData(XB[:, :N0], yB[:N0])
    gp = m.GP(ctx, XA, yA, theta, b, kernel)
    ref = m.GP(ctx, XB, yB, theta, b, kernel)
    try:
        dB.refit(gp)
        for i in range(N0, N0 + extra):
            gp.append_point(XB[:, i], yB[i])
        assert_grown_handle_agrees(oracle, gp, ref, XB, yB, theta, b, kernel)
    finally:
        gp.close()
        ref.close()


@pytest.mark.parametrize("N0", [5, 126])
def test_refit_append_refit(ctx, oracle, N0):
    """Refit, append four points (N0 = 126: across a 128-block, every buffer re-sized), refit again with data of the grown N: the
    handle's buffers have the grown size, and the state is the bits of a fresh handle on that data."""
    m = sls()
    D, extra, kernel = 3, 4, m.KERNEL_MATERN52
    XA, yA, theta, b = problem(oracle, D, N0, SEED_A)
    XB, yB, _, _ = problem(oracle, D, N0 + extra, SEED_B)
    XC, yC, _, _ = problem(oracle, D, N0 + extra, SEED_A + 100)
    Q = queries(oracle, D)
    dB, dC = DevData(XB[:, :N0], yB[:N0]), DevData(XC, yC)
    fb = Fallbacks(ctx)
    gp = m.GP(ctx, XA, yA, theta, b, kernel)
    fresh = m.GP(ctx, XC, yC, theta, b, kernel)
    try:
        dB.refit(gp)
        for i in range(N0, N0 + extra):
            gp.append_point(XB[:, i], yB[i])
        assert gp.N == N0 + extra
        dC.refit(gp)
        got = snapshot(gp, Q)
        assert_same(got, snapshot(fresh, Q), fb, "refit, append, refit against a fresh handle")
        assert_matches_oracle(got, oracle.Regressor(XC, yC, theta, b, kernel=kernel), Q, f"N0={N0}")
    finally:
        gp.close()
        fresh.close()


# ---- 3. device starts equal host starts --------------------------------------------------------------------------------------------
def maximize_both(gp, starts, starts_dev, S, n_local, acq, **kw):
    """(host-starts result, its statistics, device-starts result, its statistics)"""
    rh = gp.acq_maximize(starts, n_local, acq, UCB_H, want_all=False, **kw)
    sh = gp.last_stats()
    rd = gp.acq_maximize_dev(starts_dev.data_ptr(), S, n_local, acq, UCB_H, **kw)
    return rh, sh, rd, gp.last_stats()


def assert_same_winner(rd, sd, rh, sh, label):
    assert rd["index"] == rh["index"] and rd["value"] == rh["value"] and np.array_equal(rd["x"], rh["x"]), (label, rd, rh)
    assert sd == sh, (label, sd, sh)


# (D, N, S, n_local, SLS_WAVE_PATH, oracle): one wavefront per start (twice); lock-step rounds with S past the wave limit of 4096,
# with Np past 512, and -- switched -- with D no multiple of 16
START_CASES = [(1, 20, 1, 40, None, True), (5, 90, 129, 12, None, True), (6, 300, 4097, 6, None, False), (8, 640, 300, 10, None, True),
               (37, 384, 200, 8, "0", False)]


@pytest.mark.parametrize("acq", [0, 1], ids=["ei", "ucb"])
@pytest.mark.parametrize("D,N,S,n_local,wave,with_oracle", START_CASES, ids=[f"D{c[0]}-N{c[1]}-S{c[2]}" for c in START_CASES])
def test_device_starts_equal_host_starts(ctx, oracle, monkeypatch, D, N, S, n_local, wave, with_oracle, acq):
    """sls_acq_maximize_dev reads the D x S starts where they are; sls_acq_maximize uploads them and runs the same maximiser: the
    same winner, value, point and statistics, bit for bit, on both routes of the maximiser."""
    m = sls()
    if wave is not None:
        monkeypatch.setenv("SLS_WAVE_PATH", wave)
    X, y, theta, b = problem(oracle, D, N, SEED_A)
    starts = synth_candidates(oracle, D, S)
    starts_dev = dev_matrix(starts)
    gp = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
    try:
        rh, sh, rd, sd = maximize_both(gp, starts, starts_dev, S, n_local, acq)
        assert_same_winner(rd, sd, rh, sh, "device starts")
        assert 0 <= rd["index"] < S and sd["evals_cap"] == S * n_local and 0 < sd["evals_issued"] <= sd["evals_cap"]
        assert np.all((rd["x"] >= 0) & (rd["x"] <= 1))
        if with_oracle:
            ro = oracle.Regressor(X, y, theta, b, kernel=m.KERNEL_MATERN52).acq_maximize(starts, n_local, acq, UCB_H)
            np.testing.assert_allclose(rd["value"], ro["value"], rtol=1e-6)
    finally:
        gp.close()


@pytest.mark.parametrize("D,N,S,n_local", [(5, 90, 129, 12), (8, 640, 300, 10)], ids=["wave", "lockstep"])
def test_device_starts_index_offset_and_options(ctx, oracle, D, N, S, n_local):
    """start_index_offset shifts the reported index by exactly that much and nothing else; caller-supplied L-BFGS options (a
    shorter memory, NLopt's relative stopping tests) reach the device-starts form as they reach the host-starts form."""
    m = sls()
    X, y, theta, b = problem(oracle, D, N, SEED_A)
    starts = synth_candidates(oracle, D, S)
    starts_dev = dev_matrix(starts)
    gp = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
    try:
        _, _, r0, s0 = maximize_both(gp, starts, starts_dev, S, n_local, m.ACQ_EI)
        rh, sh, rd, sd = maximize_both(gp, starts, starts_dev, S, n_local, m.ACQ_EI, offset=1000)
        assert_same_winner(rd, sd, rh, sh, "offset=1000")
        assert rd["index"] == r0["index"] + 1000 and rd["value"] == r0["value"] and np.array_equal(rd["x"], r0["x"]) and sd == s0
        opts = m.LbfgsOpts(history=3, ftol_rel=1e-6, xtol_rel=1e-6)
        rh, sh, rd, sd = maximize_both(gp, starts, starts_dev, S, n_local, m.ACQ_EI, opts=opts)
        assert_same_winner(rd, sd, rh, sh, "history=3, ftol_rel=xtol_rel=1e-6")
        assert (rd["value"], sd) != (r0["value"], s0)         # the options were read: a start that meets a stopping test leaves the batch
    finally:
        gp.close()


@pytest.mark.parametrize("D,N,S,n_local", [(5, 90, 129, 12), (8, 640, 300, 10)], ids=["wave", "lockstep"])
def test_bench_loop_alternating_data(ctx, oracle, D, N, S, n_local):
    """bench.py's step -- sls_gp_refit_dev, then sls_acq_maximize_dev -- three times on one handle with data A, B, A: steps one and
    three return the same bits and the same statistics (nothing of step two survives in the L-BFGS workspace or the counters), and
    every step returns what a fresh handle on its data returns from host starts."""
    m = sls()
    XA, yA, theta, b = problem(oracle, D, N, SEED_A)
    XB, yB, _, _ = problem(oracle, D, N, SEED_B)
    starts = synth_candidates(oracle, D, S)
    starts_dev = dev_matrix(starts)
    dA, dB = DevData(XA, yA), DevData(XB, yB)
    fb = Fallbacks(ctx)
    gp = m.GP(ctx, XB, yB, theta, b, m.KERNEL_MATERN52)
    steps = []
    try:
        for data in (dA, dB, dA):
            data.refit(gp)
            r = gp.acq_maximize_dev(starts_dev.data_ptr(), S, n_local, m.ACQ_EI, 1.0)
            st = gp.last_stats()
            steps.append({"winner": (np.array([r["index"], r["value"]]), r["x"]),
                          "stats": (np.array([st[k] for k in ("evals_issued", "evals_cap", "rounds", "live_at_end")]),)})
        assert_same(steps[2], steps[0], fb, "step three against step one")
        assert not np.array_equal(steps[1]["winner"][1], steps[0]["winner"][1])
        for (X, y), step, name in (((XA, yA), steps[0], "A"), ((XB, yB), steps[1], "B")):
            fresh = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
            try:
                r = fresh.acq_maximize(starts, n_local, m.ACQ_EI, 1.0, want_all=False)
                st = fresh.last_stats()
            finally:
                fresh.close()
            want = {"winner": (np.array([r["index"], r["value"]]), r["x"]),
                    "stats": (np.array([st[k] for k in ("evals_issued", "evals_cap", "rounds", "live_at_end")]),)}
            assert_same(step, want, fb, f"step on {name} against a fresh handle")
    finally:
        gp.close()


# ---- 4. the caller's stream is the one used ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(5, 300), (3, 100)], ids=["tiled_fit", "single_workgroup_fit"])
def test_work_is_issued_on_the_callers_stream(oracle, D, N):
    """On a non-default torch stream handed over with sls_ctx_set_stream: a few milliseconds of matrix products, then the copies
    that bring B into buffers still holding A, then sls_gp_refit_dev and sls_acq_maximize_dev at once, nothing synchronised in
    between.  Stream order alone makes the fit see B: a library that issued its work elsewhere would fit A.  Back on its own stream
    (NULL) and behind sls_ctx_synchronize the same refit gives the same bits."""
    t, m = torch, sls()
    S, n_local = 129, 8
    XA, yA, theta, b = problem(oracle, D, N, SEED_A)
    XB, yB, _, _ = problem(oracle, D, N, SEED_B)
    Q = queries(oracle, D)
    starts = synth_candidates(oracle, D, S)
    buf, src, starts_dev = DevData(XA, yA), DevData(XB, yB), dev_matrix(starts)
    big = t.randn(4096, 4096, device="cuda")
    products = []
    t.cuda.synchronize()
    stream = t.cuda.Stream()
    c = m.Context(0)
    gp = fresh = None
    try:
        c.set_stream(stream.cuda_stream)
        fb = Fallbacks(c)
        gp = m.GP(c, XA, yA, theta, b, m.KERNEL_MATERN52)
        fresh = m.GP(c, XB, yB, theta, b, m.KERNEL_MATERN52)
        want = snapshot(fresh, Q)
        want_r = fresh.acq_maximize(starts, n_local, m.ACQ_EI, 1.0, want_all=False)
        want_q1 = fresh.predict(Q[:, :1])
        with t.cuda.stream(stream):
            for _ in range(8):
                products.append(big @ big)
            buf.X.copy_(src.X)
            buf.y.copy_(src.y)
            buf.refit(gp)
            r = gp.acq_maximize_dev(starts_dev.data_ptr(), S, n_local, m.ACQ_EI, 1.0)
        got = snapshot(gp, Q)
        assert_same(got, want, fb, "refit behind queued work on the caller's stream")
        assert_same({"winner": (np.array([r["index"], r["value"]]), r["x"])},
                    {"winner": (np.array([want_r["index"], want_r["value"]]), want_r["x"])}, fb, "maximiser on the caller's stream")

        c.set_stream(None)
        c.synchronize()
        t.cuda.synchronize()
        buf.refit(gp)
        assert_same(snapshot(gp, Q), want, fb, "refit on the library's own stream")
        assert_same({"predict": gp.predict(Q[:, :1])}, {"predict": want_q1}, fb, "single point on the slot route")
    finally:
        for h in (gp, fresh):
            if h is not None:
                h.close()
        c.close()
        t.cuda.synchronize()
    del products, big, buf, src, starts_dev          # referenced until here


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refit_dev_refuses_null_arguments(ctx, oracle):
    m = sls()
    L = m.lib()
    X, y, theta, b = problem(oracle, 3, 100, SEED_A)
    d = DevData(X, y)
    gp = m.GP(ctx, X, y, theta, b, m.KERNEL_MATERN52)
    try:
        g0, before = gp.generation(), gp.matrix(m.GP_ALPHA)
        for h, xp, yp in ((None, d.X.data_ptr(), d.y.data_ptr()), (gp.h, None, d.y.data_ptr()), (gp.h, d.X.data_ptr(), None)):
            assert L.sls_gp_refit_dev(h, C.c_void_p(xp), C.c_void_p(yp)) == -1
            assert b"sls_gp_refit_dev" in L.sls_last_error()
        assert gp.generation() == g0 and np.array_equal(gp.matrix(m.GP_ALPHA), before)
    finally:
        gp.close()


def test_maximize_dev_refuses_bad_arguments_before_any_launch(oracle):
    """Every refusal is SLS_ERR_INVALID with a message, decided before anything is launched: with profiling on, no kernel of the
    maximiser is counted, and the statistics of the last good call stay."""
    m = sls()
    L = m.lib()
    D, N, S, n_local = 5, 90, 129, 12
    X, y, theta, b = problem(oracle, D, N, SEED_A)
    starts_dev = dev_matrix(synth_candidates(oracle, D, S))
    c = m.Context(0)
    c.prof_enable(True)
    gp = m.GP(c, X, y, theta, b, m.KERNEL_MATERN52)
    x, val, idx = np.empty(D), C.c_double(), C.c_long()

    def call(h=gp.h, ptr=starts_dev.data_ptr(), S=S, n_local=n_local, acq=m.ACQ_EI, opts=None):
        return L.sls_acq_maximize_dev(h, C.c_int(acq), C.c_double(1.0), C.c_void_p(ptr), C.c_int(S), C.c_int(n_local),
                                      C.byref(opts) if opts is not None else None, C.c_long(0), x.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(val), C.byref(idx))

    def launches():
        return {k: c.prof_get(k)[1] for k in ("acq_wave", "lbfgs", "acq_gemm", "cross_gram", "grad_gemm", "finalize")}
    try:
        assert call() == 0
        stats, counted = gp.last_stats(), launches()
        assert sum(counted.values()) > 0
        bad_size = m.LbfgsOpts()
        bad_size.struct_size = 999
        for kw, word in ((dict(h=None), b"NULL"), (dict(ptr=None), b"NULL"), (dict(S=0), b"S >= 1"), (dict(n_local=0), b"n_local >= 1"),
                         (dict(acq=7), b"acquisition"), (dict(opts=m.LbfgsOpts(history=9)), b"history"),
                         (dict(opts=bad_size), b"struct_size")):
            assert call(**kw) == -1, kw
            msg = L.sls_last_error()
            assert msg and word in msg, (kw, msg)
            assert launches() == counted and gp.last_stats() == stats, kw
        assert call() == 0 and gp.last_stats() == stats
    finally:
        gp.close()
        c.close()


def test_refused_fit_leaves_a_handle_that_refits(ctx, oracle):
    """Exact duplicates among the data points and no noise (the construction of test_singular_matrix_is_rejected_by_every_fused_form,
    through the same gp_fit_device): sls_gp_refit_dev reports "not positive definite"; the fitted state is undefined until the next
    successful refit (include/sls_hip.h), which gives the bits of a fresh handle; the context stays usable."""
    m = sls()
    D, N, kernel = 6, 640, m.KERNEL_MATERN52
    XA, yA, theta, _ = problem(oracle, D, N, SEED_A)
    XB, yB, _, _ = problem(oracle, D, N, SEED_B)
    Q = queries(oracle, D)
    Xdup = XA.copy()
    Xdup[:, N - 3:] = XA[:, :3]
    bad, good = DevData(Xdup, yA), DevData(XB, yB)
    fb = Fallbacks(ctx)
    gp = m.GP(ctx, XA, yA, theta, 0.0, kernel)          # K_f alone is positive definite here: smallest eigenvalue 3e-3 (oracle, CPU)
    fresh = None
    try:
        g0 = gp.generation()
        with pytest.raises(m.SlsError, match="not positive definite"):
            bad.refit(gp)
        assert gp.generation() != g0                    # whatever the handle holds now, it is not the predictor of before
        good.refit(gp)
        fresh = m.GP(ctx, XB, yB, theta, 0.0, kernel)
        got = snapshot(gp, Q)
        assert_same(got, snapshot(fresh, Q), fb, "refit after a refused fit against a fresh handle")
        assert_matches_oracle(got, oracle.Regressor(XB, yB, theta, 0.0, kernel=kernel), Q, "after a refused fit")
    finally:
        gp.close()
        if fresh is not None:
            fresh.close()
