"""The escape case shared by tests/test_qlognei_cpu.py (on the restatement) and tests/test_gpu_qlognei.py (on the device): D = 1,
q = 2, a constant baseline 0.05 below the largest value any draw takes on a grid of [0, 1].  Only around the top draws' peaks does a
point improve on it; a start pair elsewhere has qNEI exactly 0 and the zero gradient, and sls_qnei_maximize returns it unmoved.  The
log form at the default temperatures has the gradient of the best draw there and climbs.

ESC_ASSERTED lists the starts both tests assert on.  They were chosen on the CPU (restatement + tests/lbfgs_ref.py, ESC_N_LOCAL
evaluations): qNEI exactly 0 at the start with every value at least 1e-3 below the baseline, so no device rounding revives them, and
qNEI at the end 6.28e-3 (the top draw's peak over the baseline, divided by the 8 draws) against ESC_MARGIN = 1e-3.  A start whose
climb ends on a local maximum below the baseline stays dead under either form and is not listed."""
import numpy as np

import lbfgs_ref
import path_ref as ph
import qlognei_ref as lr

ESC_D, ESC_N, ESC_F, ESC_DRAWS, ESC_Q, ESC_STARTS, ESC_N_LOCAL = 1, 12, 64, 8, 2, 24, 30
ESC_B, ESC_PATH_SEED, ESC_GAP = 0.02, 77, 0.05
ESC_TAUS = (1e-6, 1e-2)
ESC_MARGIN = 1e-3
ESC_ASSERTED = [2, 3, 4, 5, 7, 9, 12, 15, 16, 17, 19]


def escape_case():
    rng = np.random.default_rng(11)
    X = rng.uniform(0.0, 1.0, (ESC_D, ESC_N))
    y = np.sin(6.0 * X[0]) + 0.05 * rng.standard_normal(ESC_N)
    theta = np.array([0.5, 0.15])
    ref = ph.PathRef(X, y, theta, ESC_B, ph.MATERN52, ESC_DRAWS, ESC_F, seed=ESC_PATH_SEED)
    grid = np.linspace(0.0, 1.0, 201)
    t = np.full(ESC_DRAWS, ref.eval_all(grid[None, :]).max() - ESC_GAP)
    starts = np.random.default_rng(12).uniform(0.0, 1.0, (ESC_Q * ESC_D, ESC_STARTS))
    return dict(X=X, y=y, theta=theta, b=ESC_B, kernel=ph.MATERN52, ref=ref, t=t, starts=starts)


def escape_cpu_run(e):
    """(end points (2, S), end values) of the bounded L-BFGS on the restatement of the log form."""
    def evaluate(T):
        out = lr.qlognei(e["ref"], T, ESC_Q, e["t"], *ESC_TAUS, want_G=False)
        return out["val"], out["grad"]
    r = lbfgs_ref.run(evaluate, e["starts"], ESC_N_LOCAL)
    return r["x_stars"], r["y_stars"]
