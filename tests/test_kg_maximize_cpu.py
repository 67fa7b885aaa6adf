"""The inputs of tests/test_gpu_kg_maximize.py are not sensitive to rounding in the evaluation -- shown without a GPU.

util.assert_starts_agree lets 5 % of the starts end elsewhere when one of their Armijo tests sat at rounding level of its threshold.
That share is a condition on the INPUTS.  Here every case of tests/kg_cases.py runs tests/lbfgs_ref.py on the numpy restatement of the
knowledge gradient (tests/kg_ref.py), in both summation orders of the step, and once more on a copy of the objective perturbed at the
evaluation's rounding level (1e-12 relative: cond(K_y) eps of these fits): at least 95 % of the starts end within 1e-6 of the largest
value of each other (the precedent of tests/test_jes_maximize_cpu.py)."""
import numpy as np
import pytest

import kg_cases as kc
import lbfgs_ref


def perturbed(evaluate, level=1e-12):
    """The objective with a deterministic relative wobble of `level` on the value and every gradient component."""
    def ev(T):
        v, g = evaluate(T)
        ph = 1e5 * np.asarray(T).sum(axis=0)
        return v + level * (1.0 + np.abs(v)) * np.cos(ph), g * (1.0 + level * np.sin(ph + np.arange(g.shape[0])[:, None]))
    return ev


@pytest.fixture(scope="module")
def runs():
    out = {}
    for c in kc.CASES:
        case = kc.Case(c)
        ev = case.cpu_objective()
        for h in kc.HISTORIES:
            out[c, h] = (case, lbfgs_ref.run(ev, case.starts, case.n_local, history=h, order="lanes"),
                         lbfgs_ref.run(ev, case.starts, case.n_local, history=h, order="sequential"),
                         lbfgs_ref.run(perturbed(ev), case.starts, case.n_local, history=h, order="lanes"))
    return out


@pytest.mark.parametrize("h", kc.HISTORIES)
@pytest.mark.parametrize("c", kc.CASES, ids=kc.case_id)
def test_at_least_95_percent_of_the_starts_do_not_depend_on_rounding(runs, c, h):
    case, a, b, p = runs[c, h]
    scale = np.abs(a["y_stars"]).max()
    for other, name in ((b, "summation order"), (p, "perturbed evaluation")):
        apart = np.abs(a["y_stars"] - other["y_stars"]) > 1e-6 * scale
        print(f"{kc.case_id(c)} history {h}, {name}: {apart.sum()} of {case.S} starts ({apart.mean():.2%}) end more than 1e-6 apart; "
              f"evaluations {a['evals_issued']}, live at the end {a['live_at_end']}, smallest Armijo margin {a['armijo_margin'].min():.2e}")
        assert apart.mean() <= 0.05


@pytest.mark.parametrize("c", kc.CASES, ids=kc.case_id)
def test_cases_reach_the_branches_they_are_there_for(runs, c):
    case, a, _, _ = runs[c, 6]
    assert (case.starts < 0.0).any() and (case.starts > 1.0).any(), "the clamp"
    assert (a["evals"] - 1 - a["accepted"]).max() >= 1, "a rejected trial"
    assert a["accepted"].max() >= 4, "steps"
    assert np.all(np.isfinite(a["y_stars"])) and a["y_stars"].max() > a["y_stars"].min() and a["y_stars"].min() >= 0.0
