"""The optional outputs of the evaluations on the path draws (sls_qeubo_eval, sls_qnei_eval, sls_qlognei_eval, sls_line_eval free and
anchored: gradient and win counts; sls_path_eval_sub: gradient and expanded points) in every combination of present and absent: the
values are the same bits in all four calls, and a gradient, win count or point block that is returned is, bit for bit, that of the
call that asks for everything.  The outputs of these entry points are staged through one host body each, so no combination may depend
on which of them an earlier test happened to use."""
import itertools

import numpy as np
import pytest

import maximize_cases as mc
from util import sls

pytestmark = pytest.mark.gpu
D, N, ND, F, M, Q = 3, 20, 5, 64, 3, 2
ROUTES = ["qeubo_eval", "qnei_eval", "qlognei_eval", "line_eval_free", "line_eval_anchored", "eval_sub"]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("route", ROUTES)
def test_every_combination_of_optional_outputs(route):
    m = sls()
    ctx = m.Context(0)
    X, y, theta = mc.problem(D, N, seed=N + D)
    gp = m.GP(ctx, X, y, theta, 0.05, m.KERNEL_MATERN52)
    ps = m.PathSamples(gp, ND, F, seed=99)
    rng = np.random.default_rng(17)
    t = ps.max_over_points(X)[0] - 1.0   # a baseline low enough that the sets improve on it in some draws: a gradient that is not zero
    if route == "eval_sub":
        d = 2
        maps = m.SubMaps(rng.uniform(0.0, 0.5, (2, D, d)), rng.uniform(0.0, 0.2, (2, D)), [0, 1, 0])
        Z, dr = rng.uniform(0.0, 1.0, (d, M)), [4, 0, 2]
        second = "want_x"
        call = lambda **kw: ps.eval_sub(maps, Z, dr, **kw)
        shapes = ((d, M), (D, M))
    else:
        anchored = route == "line_eval_anchored"
        rows = {"line_eval_free": 2 * D, "line_eval_anchored": D}.get(route, Q * D)
        block = rng.uniform(0.0, 1.0, (rows, M))
        second = "want_wins"
        shapes = ((rows, M), (Q, M))
        if route.startswith("line_eval"):   # free: the EUBO form; anchored: the qNEI form over the baseline
            anchor = rng.uniform(0.0, 1.0, D) if anchored else None
            call = lambda **kw: ps.line_eval(block, Q, anchor=anchor, baseline=t if anchored else None, **kw)
        elif route == "qeubo_eval":
            call = lambda **kw: ps.qeubo_eval(block, Q, **kw)
        else:
            call = lambda **kw: getattr(ps, route)(block, Q, t, **kw)
    full = call(**{"want_grad": True, second: True})
    assert len(full) == 3 and full[0].shape == (M,) and (full[1].shape, full[2].shape) == shapes
    assert np.all(np.isfinite(full[0])) and np.any(full[1] != 0.0)
    for want_grad, want_second in itertools.product([False, True], repeat=2):
        out = call(**{"want_grad": want_grad, second: want_second})
        out = out if isinstance(out, tuple) else (out,)
        assert len(out) == 1 + want_grad + want_second
        print(f"{route}: want_grad={want_grad} {second}={want_second} -> values {out[0]}")
        assert _same(out[0], full[0])
        if want_grad:
            assert _same(out[1], full[1])
        if want_second:
            assert _same(out[-1], full[2])
    ps.close()
    gp.close()
    ctx.close()
