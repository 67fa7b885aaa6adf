"""Cases of gallery EUBO (sls_patch_eval / sls_patch_maximize), shared by tests/test_gpu_patch.py (the device held to the numpy
restatement tests/patch_ref.py, and its maximiser to tests/lbfgs_ref.py driven by the device's own patch_eval) and
tests/test_patch_cpu.py (the same cases on the CPU restatement, to show that the inputs keep their winners and are not sensitive to
the summation order).  Built on tests/maximize_cases.py, which stays as it is: its generator, its starts (box_starts: uniform in
[-0.2, 1.2], every third column rounded to a corner), N_LOCAL = 15 and its four option sets VARIANTS.

Data as the line cases: N = 60, F = 64, 8 draws, b = 0.05, Matern-5/2.  The anchor of an anchored maximiser case is the best data point.

Order sensitivity of the maximiser inputs (test_patch_cpu.py asserts it for every case and option set and prints it): the share of
starts whose end values differ by more than 1e-6 of the largest between lbfgs_ref.run(order="lanes") and order="sequential" on the CPU
objective, at most 2 %.  Start seed = SEED + position in PATCHES.  Seeds tried: SEED = 900 only -- the first one holds for all 16 runs
(4 shapes x 4 option sets: 0 of 129 starts apart in each)."""
import numpy as np

import maximize_cases as mc

PATCHES = [dict(qs=2, qt=2, D=5, anchored=False), dict(qs=4, qt=4, D=5, anchored=True), dict(qs=3, qt=5, D=16, anchored=False),
           dict(qs=2, qt=3, D=33, anchored=True)]                          # nvar = 20, 15, 64, 99
SEED = 900


def case_ids():
    return [(i, v) for i in range(len(PATCHES)) for v in mc.VARIANTS]


def case_name(c):
    i, v = c
    sh = PATCHES[i]
    return f"patch-{sh['qs']}x{sh['qt']}-D{sh['D']}-{'anchored' if sh['anchored'] else 'free'}-{v}"


class PatchCase:
    """Inputs of one shape: X, y, theta, b, kernel, n_draws, F, path_seed, qs, qt, D, anchor (None: free form), nvar, S, starts."""

    def __init__(self, i):
        self.shape = dict(PATCHES[i])
        sh = self.shape
        D, N = sh["D"], 60
        self.X, self.y, self.theta = mc.problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
        self.kernel, self.b = mc.MATERN52, 0.05
        self.n_draws, self.F, self.path_seed = 8, 64, 1234 + D
        self.qs, self.qt, self.D, self.S = sh["qs"], sh["qt"], D, 129
        self.anchor = self.X[:, int(np.argmax(self.y))].copy() if sh["anchored"] else None
        self.nvar = (3 if sh["anchored"] else 4) * D
        self.starts = mc.box_starts(self.nvar, self.S, SEED + i)


# ---- inputs of the restatement test ---------------------------------------------------------------------------------------------------
# (kernel, D, qs, qt, M, anchored[, N, F]): M = 129 / 130 / 257 reach into a second / third 128-wide tile, M = 1 is a lone patch; the
# fourth case also runs with the per-draw baseline of the data.  A patch whose restated gap (qeubo_ref / qnei_ref: how far the values
# may move before a winner changes) is inside the value tolerance cannot be compared in wins; test_patch_cpu.py asserts that at most
# 5 % of a case's patches are such (patches seed = RESTATED_SEED + position; the first seed tried was kept: 0 of M in every case, the
# smallest gap 1.2e-4 against a tolerance of about 6e-11).
# The last two: D > 128 (N = 90, F = 100 and N = 130, F = 300), where the folded gradient comes from two and three 128-column tiles.
RESTATED = [(mc.SE, 5, 2, 2, 129, False), (mc.MATERN52, 33, 3, 4, 130, True), (mc.MATERN52, 5, 4, 4, 1, False),
            (mc.SE, 16, 5, 3, 257, True), (mc.SE, 129, 2, 2, 130, False, 90, 100), (mc.MATERN52, 257, 2, 3, 129, True, 130, 300)]
RESTATED_SEED = 60
WITH_BASELINE = 3                                                          # the case that also runs with the per-draw baseline


class RestatedCase:
    def __init__(self, k):
        self.kernel, self.D, self.qs, self.qt, self.M, anchored = RESTATED[k][:6]
        D, (N, F) = self.D, RESTATED[k][6:] or (60, 64)
        self.X, self.y, self.theta = mc.problem(D, N, seed=N + D, ell=0.3 * np.sqrt(D))
        self.b, self.n_draws, self.F, self.path_seed = 0.05, 8, F, 1234 + D
        rng = np.random.default_rng(RESTATED_SEED + k)
        # the anchor (drawn first, as the line cases draw theirs) is not a data point: cell (0, 0) of every patch would then tie with
        # its own incumbent in the baseline form
        self.anchor = rng.uniform(0.0, 1.0, D) if anchored else None
        self.patches = rng.uniform(0.0, 1.0, ((3 if anchored else 4) * D, self.M))
        self.with_baseline = (False, True) if k == WITH_BASELINE else (False,)
