"""What every single-winner maximiser returns around its search (csrc/lbfgs_driver.hpp: maximize_begin / maximize_finish), pinned for
each entry point that goes through it: sls_acq_maximize with the three acquisition types on the one-launch wave route and on the
lock-step rounds, sls_mes_maximize, sls_eubo_maximize, sls_qeubo_maximize and sls_qnei_maximize (baseline: every draw's maximum
over the data, sls_path_max_over_points).  The winner is the first maximum of y_stars and its column of x_stars, bit for bit; the start index offset only shifts the index; leaving x_stars / y_stars out changes nothing else;
sls_acq_last_stats describes the run; a history outside 1..8 is refused by name and leaves the handle usable.

Shapes: N = 40, D = 3 takes the wave route for EI and UCB (LogEI has no wave objective and runs the rounds there); N = 200, D = 5 with
SLS_WAVE_PATH=0 runs the rounds for all three.  S = 1, 128 and 129 starts: one start, a full 128-column tile, one column into the
next tile.  No stored numbers: the results are compared with each other."""
import numpy as np
import pytest

from util import sls

pytestmark = pytest.mark.gpu
SE, MATERN52 = 0, 1
N_LOCAL = 12
OFFSET = 12345
CASES = ["ei_wave", "ucb_wave", "logei_small", "ei_rounds", "ucb_rounds", "logei_rounds", "mes", "eubo", "qeubo", "qnei"]
ACQ = {"ei": 0, "ucb": 1, "logei": 2}


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def problem(D, N, seed, ell=0.5, a=0.5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


class Route:
    """One entry point on one shape: run(starts, **kw) -> the binding's result dict, stats() -> sls_acq_last_stats."""

    def __init__(self, m, ctx, case, monkeypatch):
        name, _, shape = case.partition("_")
        small = shape in ("wave", "small") or name in ("qeubo", "qnei")
        N, D = (40, 3) if small else (200, 5)
        if shape == "rounds":
            monkeypatch.setenv("SLS_WAVE_PATH", "0")
        self.wave = shape == "wave"
        X, y, theta = problem(D, N, seed=N + D)
        self.gp = gp = m.GP(ctx, X, y, theta, 0.05, MATERN52)
        self.path = None
        self.nvar = D
        if name in ACQ:
            self.run = lambda starts, **kw: gp.acq_maximize(starts, N_LOCAL, acq=ACQ[name], ucb_h=1.5, **kw)
        elif name == "mes":
            y_star = y.max() + np.array([0.1, 0.25, 0.6])
            self.run = lambda starts, **kw: gp.mes_maximize(y_star, starts, N_LOCAL, **kw)
        elif name == "eubo":
            self.nvar = 2 * D
            self.run = lambda starts, **kw: gp.eubo_maximize(starts, N_LOCAL, **kw)
        else:
            self.nvar = 3 * D
            self.path = ps = m.PathSamples(gp, 8, 64, seed=7)
            if name == "qeubo":
                self.run = lambda starts, **kw: ps.qeubo_maximize(starts, 3, N_LOCAL, **kw)
            else:
                t, _ = ps.max_over_points(X)
                self.run = lambda starts, **kw: ps.qnei_maximize(starts, 3, N_LOCAL, t, **kw)

    def starts(self, S):
        return np.random.default_rng(100 + S).uniform(0.0, 1.0, (self.nvar, S))

    def close(self):
        if self.path is not None:
            self.path.close()
        self.gp.close()


def check_winner(r, S, nvar, offset):
    xs, ys = r["x_stars"], r["y_stars"]
    assert xs.shape == (nvar, S) and ys.shape == (S,) and r["x"].shape == (nvar,)
    best = int(np.argmax(ys))                                          # numpy: the first index of the maximum
    assert _bits(r["value"]) == _bits(ys.max())
    assert r["index"] - offset == best
    assert np.array_equal(_bits(r["x"]), _bits(xs[:, best]))


@pytest.mark.parametrize("S", [1, 128, 129])
@pytest.mark.parametrize("case", CASES)
def test_winner_offset_optional_outputs_and_statistics(m, ctx, monkeypatch, case, S):
    rt = Route(m, ctx, case, monkeypatch)
    starts = rt.starts(S)
    ctx.prof_enable(True)
    ctx.prof_reset()
    r0 = rt.run(starts)
    st = rt.gp.last_stats()
    wave_launches = ctx.prof_get("acq_wave")[1]
    ctx.prof_enable(False)
    check_winner(r0, S, rt.nvar, 0)
    # the statistics of that run
    cap = S * N_LOCAL
    assert st["evals_cap"] == cap and S <= st["evals_issued"] <= cap and 0 <= st["live_at_end"] <= S, st
    if rt.wave:
        assert wave_launches == 1 and st["rounds"] == N_LOCAL, (wave_launches, st)
    else:
        assert wave_launches == 0 and 1 <= st["rounds"] <= N_LOCAL, (wave_launches, st)
    # the offset moves the index and nothing else
    r1 = rt.run(starts, offset=OFFSET)
    check_winner(r1, S, rt.nvar, OFFSET)
    assert r1["index"] == r0["index"] + OFFSET
    for k in ("x", "value", "x_stars", "y_stars"):
        assert np.array_equal(_bits(r1[k]), _bits(r0[k])), k
    # without x_stars / y_stars: the same winner
    r2 = rt.run(starts, want_all=False)
    assert r2["x_stars"] is None and r2["y_stars"] is None
    assert r2["index"] == r0["index"]
    assert np.array_equal(_bits(r2["x"]), _bits(r0["x"])) and _bits(r2["value"]) == _bits(r0["value"])
    assert rt.gp.last_stats() == st
    rt.close()


@pytest.mark.parametrize("case", CASES)
def test_history_outside_1_to_8_is_refused_and_the_handle_stays_usable(m, ctx, monkeypatch, case):
    rt = Route(m, ctx, case, monkeypatch)
    starts = rt.starts(129)
    before = rt.run(starts)
    for history in (0, 9):
        with pytest.raises(m.SlsError, match="history"):
            rt.run(starts, opts=m.LbfgsOpts(history=history))
        assert "history" in m.lib().sls_last_error().decode()
        after = rt.run(starts)
        check_winner(after, 129, rt.nvar, 0)
        for k in ("index", "x", "value", "x_stars", "y_stars"):
            assert np.array_equal(_bits(after[k]), _bits(before[k])), (history, k)
    rt.close()
