"""sls_jes_maximize start by start against the restated bounded L-BFGS (tests/lbfgs_ref.py) driven by the device's own sls_jes_eval,
through util.assert_starts_agree unchanged: end values to 1e-6 on at least 95 % of the starts, every other start with a restated
Armijo margin below 1e-6.  tests/test_jes_maximize_cpu.py shows that the cases (tests/jes_cases.py) keep the reference alone within
that share.  Active-set compaction does not change a start's bits."""
import numpy as np
import pytest

import jes_cases as jc
import lbfgs_ref
from util import assert_starts_agree, sls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    return sls()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("h", jc.HISTORIES)
@pytest.mark.parametrize("c", jc.CASES, ids=jc.case_id)
def test_maximiser_against_the_restated_lbfgs(m, ctx, monkeypatch, c, h):
    case = jc.Case(c)
    gp = m.GP(ctx, case.X, case.y, case.theta, jc.B, case.kernel)
    j = gp.jes_create(case.x_star, case.f_star, jc.STAR_NOISE)
    opts = m.LbfgsOpts(history=h)                                            # the default options, and a one-pair memory
    rg = j.maximize(case.starts, case.n_local, jc.B, offset=500, opts=opts)
    rr = lbfgs_ref.run(lambda T: j.eval(T, jc.B), case.starts, case.n_local, history=h, order="lanes")
    agree = assert_starts_agree(rg, rr, label=f"jes {jc.case_id(c)} history {h}")
    print(f"{jc.case_id(c)} history {h}: {int((~agree).sum())} of {case.S} starts end elsewhere; winner {rg['value']:.12g}")
    assert np.all((rg["x_stars"] >= 0) & (rg["x_stars"] <= 1)) and np.all(np.isfinite(rg["y_stars"]))
    assert rg["value"] == rg["y_stars"].max() and rg["index"] - 500 == int(np.argmax(rg["y_stars"]))
    assert np.array_equal(rg["x_stars"][:, rg["index"] - 500], rg["x"])
    assert abs(rg["value"] - rr["value"]) <= 1e-6 * max(1.0, abs(rr["value"]))
    st = gp.last_stats()
    assert 0 < st["evals_issued"] <= case.S * case.n_local and st["evals_cap"] == case.S * case.n_local
    assert st["rounds"] <= case.n_local
    monkeypatch.setenv("SLS_COMPACT", "0")
    r0 = j.maximize(case.starts, case.n_local, jc.B, offset=500, opts=opts)
    monkeypatch.delenv("SLS_COMPACT")
    assert np.array_equal(rg["x_stars"], r0["x_stars"]) and np.array_equal(rg["y_stars"], r0["y_stars"])
    assert rg["index"] == r0["index"] and rg["value"] == r0["value"]
    j.close()
    gp.close()
