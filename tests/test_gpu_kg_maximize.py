"""sls_kg_maximize start by start against the restated bounded L-BFGS (tests/lbfgs_ref.py) driven by the device's own sls_kg_eval,
through util.assert_starts_agree unchanged: end values to 1e-6 on at least 95 % of the starts, every other start with a restated
Armijo margin below 1e-6.  tests/test_kg_maximize_cpu.py shows that the cases (tests/kg_cases.py) keep the reference alone within
that share.  Active-set compaction does not change a start's bits."""
import numpy as np
import pytest

import kg_cases as kc
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


@pytest.mark.parametrize("h", kc.HISTORIES)
@pytest.mark.parametrize("c", kc.CASES, ids=kc.case_id)
def test_maximiser_against_the_restated_lbfgs(m, ctx, monkeypatch, c, h):
    case = kc.Case(c)
    own = case.include_self
    gp = m.GP(ctx, case.X, case.y, case.theta, kc.B, case.kernel)
    kg = gp.kg_create(case.x_ref)
    opts = m.LbfgsOpts(history=h)                                            # the default options, and a one-pair memory
    rg = kg.maximize(case.starts, case.n_local, kc.B, include_self=own, offset=500, opts=opts)
    rr = lbfgs_ref.run(lambda T: kg.eval(T, kc.B, include_self=own, want_grad=True), case.starts, case.n_local, history=h, order="lanes")
    agree = assert_starts_agree(rg, rr, label=f"kg {kc.case_id(c)} history {h}")
    print(f"{kc.case_id(c)} history {h}: {int((~agree).sum())} of {case.S} starts end elsewhere; winner {rg['value']:.12g}")
    assert np.all((rg["x_stars"] >= 0) & (rg["x_stars"] <= 1)) and np.all(np.isfinite(rg["y_stars"])) and np.all(rg["y_stars"] >= 0)
    assert rg["value"] == rg["y_stars"].max() and rg["index"] - 500 == int(np.argmax(rg["y_stars"]))
    assert np.array_equal(rg["x_stars"][:, rg["index"] - 500], rg["x"])
    assert abs(rg["value"] - rr["value"]) <= 1e-6 * max(1.0, abs(rr["value"]))
    st = gp.last_stats()
    assert 0 < st["evals_issued"] <= case.S * case.n_local and st["evals_cap"] == case.S * case.n_local
    assert st["rounds"] <= case.n_local
    monkeypatch.setenv("SLS_COMPACT", "0")
    r0 = kg.maximize(case.starts, case.n_local, kc.B, include_self=own, offset=500, opts=opts)
    monkeypatch.delenv("SLS_COMPACT")
    assert np.array_equal(rg["x_stars"], r0["x_stars"]) and np.array_equal(rg["y_stars"], r0["y_stars"])
    assert rg["index"] == r0["index"] and rg["value"] == r0["value"]
    kg.close()
    gp.close()
