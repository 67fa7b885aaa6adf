"""The inputs of tests/test_gpu_jes_maximize.py, shared with tests/test_jes_maximize_cpu.py, which shows without a GPU that they are not
sensitive to rounding in the evaluation (the 95 % share of util.assert_starts_agree is a condition on these inputs)."""
import numpy as np

import jes_ref

SE, MATERN52 = 0, 1
B, K, STAR_NOISE = 0.05, 7, 1e-8
# (kernel, D, N, S, n_local)
CASES = [(SE, 2, 90, 37, 30), (MATERN52, 16, 300, 200, 25)]
HISTORIES = (6, 1)          # the default options and a one-pair memory


def case_id(c):
    return "k%d-D%d-N%d-S%d" % c[:4]


class Case:
    def __init__(self, c):
        self.kernel, self.D, self.N, self.S, self.n_local = c
        D, N = self.D, self.N
        rng = np.random.default_rng(100 * D + N)
        self.X = np.asfortranarray(rng.uniform(0.0, 1.0, (D, N)))
        self.y = np.sin(2.0 * self.X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
        self.theta = np.concatenate([[0.5], 0.3 * np.sqrt(D) * rng.uniform(0.8, 1.25, D)])
        # optima as posterior draws would leave them: near the best data points, values around and above max(y), one below the mean
        best = np.argsort(self.y)[-K:]
        self.x_star = np.asfortranarray(np.clip(self.X[:, best] + 0.05 * rng.standard_normal((D, K)), 0.0, 1.0))
        self.f_star = self.y.max() + 0.15 * np.abs(rng.standard_normal(K))
        self.f_star[1] = self.y.mean() - 0.1
        self.starts = np.asfortranarray(rng.uniform(-0.2, 1.2, (D, self.S)))      # outside the box too: the clamp

    def cpu_objective(self):
        f = jes_ref.fit(self.X, self.y, self.theta[1:], self.theta[0], B, self.kernel)
        o = jes_ref.condition(f, self.x_star, self.f_star, STAR_NOISE)
        return lambda T: jes_ref.evaluate(f, o, T, B)[:2]
