"""What every single-winner maximiser returns around its search (csrc/lbfgs_driver.hpp: maximize_begin / maximize_finish), pinned for
each entry point that goes through it: sls_acq_maximize with the three acquisition types on the one-launch wave route and on the
lock-step rounds, sls_mes_maximize, sls_eubo_maximize, sls_jes_maximize (K = 5 optima at seeded uniform points), sls_kg_maximize (K = 7
seeded points, the candidate itself included), sls_acq_maximize_sub (EI) and sls_mes_maximize_sub (d = 2; two maps on alternating
starts: a box around data point 0 in its first two coordinates, and a centred pair of directions; the winner's z and x are columns
of z_stars and x_stars), sls_qeubo_maximize and sls_qnei_maximize (baseline: every draw's maximum
over the data, sls_path_max_over_points).  The winner is the first maximum of y_stars and its column of x_stars, bit for bit; the start index offset only shifts the index; leaving x_stars / y_stars out changes nothing else;
sls_acq_last_stats describes the run; a history outside 1..8 is refused by name and leaves the handle usable.

Shapes: N = 40, D = 3 takes the wave route for EI and UCB (LogEI has no wave objective and runs the rounds there); N = 200, D = 5 with
SLS_WAVE_PATH=0 runs the rounds for all three and for the *_sub routes; JES and KG run on the small shape.  S = 1, 128 and 129 starts: one start, a full 128-column tile, one column into the
next tile.  No stored numbers: the results are compared with each other."""
import numpy as np
import pytest

import subspace_cases as sc
from util import sls

pytestmark = pytest.mark.gpu
SE, MATERN52 = 0, 1
N_LOCAL = 12
OFFSET = 12345
CASES = ["ei_wave", "ucb_wave", "logei_small", "ei_rounds", "ucb_rounds", "logei_rounds", "mes", "eubo", "jes", "kg", "acq_sub", "mes_sub",
         "qeubo", "qnei"]
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
        small = shape in ("wave", "small") or name in ("qeubo", "qnei", "jes", "kg")
        N, D = (40, 3) if small else (200, 5)
        if shape in ("rounds", "sub"):
            monkeypatch.setenv("SLS_WAVE_PATH", "0")
        self.wave = shape == "wave"
        X, y, theta = problem(D, N, seed=N + D)
        self.gp = gp = m.GP(ctx, X, y, theta, 0.05, MATERN52)
        self.path = None
        self.nvar = D
        self.var, self.xrows = "x", None      # the *_sub routes: the variables are z, and x (xrows = D rows) comes with them
        y_star = y.max() + np.array([0.1, 0.25, 0.6])
        rng = np.random.default_rng(1000 + N + D)
        if shape == "sub":
            self.nvar, self.var, self.xrows = 2, "z", D
            Ab, cb = sc.box_maps(X, 1)
            Ac, cc = sc.centred_maps(rng, D, 2, 1)
            A, c = np.concatenate([Ab[:, :, :2], Ac]), np.concatenate([cb, cc])
            maps = lambda starts: m.SubMaps(A, c, np.arange(starts.shape[1]) % 2)
            if name == "acq":
                self.run = lambda starts, **kw: gp.acq_maximize_sub(maps(starts), starts, N_LOCAL, acq=ACQ["ei"], **kw)
            else:
                self.run = lambda starts, **kw: gp.mes_maximize_sub(y_star, maps(starts), starts, N_LOCAL, **kw)
        elif name == "jes":
            self.path = js = gp.jes_create(rng.uniform(0.0, 1.0, (D, 5)), y.max() + np.linspace(0.1, 0.6, 5))
            self.run = lambda starts, **kw: js.maximize(starts, N_LOCAL, 0.05, **kw)
        elif name == "kg":
            self.path = kg = gp.kg_create(rng.uniform(0.0, 1.0, (D, 7)))
            self.run = lambda starts, **kw: kg.maximize(starts, N_LOCAL, 0.05, include_self=True, **kw)
        elif name in ACQ:
            self.run = lambda starts, **kw: gp.acq_maximize(starts, N_LOCAL, acq=ACQ[name], ucb_h=1.5, **kw)
        elif name == "mes":
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

    def points(self):
        """(key, rows) of what a result holds per start: the variables, and for the *_sub routes their points as well."""
        return [(self.var, self.nvar)] + ([("x", self.xrows)] if self.xrows else [])

    def close(self):
        if self.path is not None:
            self.path.close()
        self.gp.close()


def check_winner(r, S, rt, offset):
    ys = r["y_stars"]
    assert ys.shape == (S,)
    best = int(np.argmax(ys))                                          # numpy: the first index of the maximum
    assert _bits(r["value"]) == _bits(ys.max())
    assert r["index"] - offset == best
    for var, rows in rt.points():
        xs = r[var + "_stars"]
        assert xs.shape == (rows, S) and r[var].shape == (rows,)
        assert np.array_equal(_bits(r[var]), _bits(xs[:, best]))


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
    check_winner(r0, S, rt, 0)
    # the statistics of that run
    cap = S * N_LOCAL
    assert st["evals_cap"] == cap and S <= st["evals_issued"] <= cap and 0 <= st["live_at_end"] <= S, st
    if rt.wave:
        assert wave_launches == 1 and st["rounds"] == N_LOCAL, (wave_launches, st)
    else:
        assert wave_launches == 0 and 1 <= st["rounds"] <= N_LOCAL, (wave_launches, st)
    # the offset moves the index and nothing else
    r1 = rt.run(starts, offset=OFFSET)
    check_winner(r1, S, rt, OFFSET)
    assert r1["index"] == r0["index"] + OFFSET
    keys = [var + tail for var, _ in rt.points() for tail in ("", "_stars")]
    for k in keys + ["value", "y_stars"]:
        assert np.array_equal(_bits(r1[k]), _bits(r0[k])), k
    # without x_stars / y_stars: the same winner
    r2 = rt.run(starts, want_all=False)
    assert r2["y_stars"] is None and all(r2[var + "_stars"] is None for var, _ in rt.points())
    assert r2["index"] == r0["index"] and _bits(r2["value"]) == _bits(r0["value"])
    assert all(np.array_equal(_bits(r2[var]), _bits(r0[var])) for var, _ in rt.points())
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
        check_winner(after, 129, rt, 0)
        for k in ["index", "value", "y_stars"] + [var + tail for var, _ in rt.points() for tail in ("", "_stars")]:
            assert np.array_equal(_bits(after[k]), _bits(before[k])), (history, k)
    rt.close()
