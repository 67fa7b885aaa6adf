"""The inputs of tests/test_gpu_kg_maximize.py, shared with tests/test_kg_maximize_cpu.py, which shows without a GPU that they are not
sensitive to rounding in the evaluation (the 95 % share of util.assert_starts_agree is a condition on these inputs)."""
import numpy as np

import jes_ref
import kg_ref

SE, MATERN52 = 0, 1
B = 0.05
# (kernel, D, N, S, n_local, K, include_self)
CASES = [(SE, 2, 90, 37, 30, 7, True), (MATERN52, 16, 300, 200, 25, 40, True), (SE, 2, 90, 37, 30, 90, False)]
HISTORIES = (6, 1)          # the default options and a one-pair memory


def case_id(c):
    return "k%d-D%d-N%d-S%d-K%d-self%d" % (c[0], c[1], c[2], c[3], c[5], c[6])


class Case:
    def __init__(self, c):
        self.kernel, self.D, self.N, self.S, self.n_local, self.K, self.include_self = c
        D, N, K = self.D, self.N, self.K
        rng = np.random.default_rng(100 * D + N + K)
        self.X = np.asfortranarray(rng.uniform(0.0, 1.0, (D, N)))
        self.y = np.sin(2.0 * self.X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
        self.theta = np.concatenate([[0.5], 0.3 * np.sqrt(D) * rng.uniform(0.8, 1.25, D)])
        # the fixed points: the K data points of highest y (K = N: all of them, the host layer's default set), in index order
        keep = np.sort(np.argsort(self.y)[-K:])
        self.x_ref = np.asfortranarray(self.X[:, keep])
        self.starts = np.asfortranarray(rng.uniform(-0.2, 1.2, (D, self.S)))      # outside the box too: the clamp

    def cpu_objective(self):
        f = jes_ref.fit(self.X, self.y, self.theta[1:], self.theta[0], B, self.kernel)
        o = kg_ref.points(f, self.x_ref)
        return lambda T: kg_ref.evaluate(f, o, T, B, self.include_self)[:2]


# degenerate line sets (a, b) of the combiner tests (tests/test_kg_cpu.py, tests/test_gpu_kg.py)
DEGENERATE = {
    "all slopes equal": ([0.3, 1.1, -0.2, 1.1], [0.25, 0.25, 0.25, 0.25]),
    "exact duplicates": ([0.3, 0.3, -0.2, -0.2, 0.1, 0.1], [0.5, 0.5, -1.0, -1.0, 0.1, 0.1]),
    "three lines through one point": ([3.0, 2.0, 1.0, 0.5], [-1.0, 0.0, 1.0, 0.25]),
    "a line dominated everywhere": ([0.0, 0.2, -50.0, 0.1], [-1.0, 1.0, 0.3, 0.0]),
    "all b = 0": ([0.4, -0.1, 0.4, 0.2], [0.0, 0.0, -0.0, 0.0]),
    "slopes 1e-300 apart beside slopes of order 1": ([0.1, 0.2, 0.0, 0.0, 0.15], [0.0, 1e-300, 1.0, -1.0, -1e-300]),
    "a breakpoint that overflows to +inf": ([1e10, 0.0, 0.5], [0.0, 1e-300, -1.0]),
    "a breakpoint that overflows to -inf": ([0.0, 1e10, 0.5], [0.0, 1e-300, 1.0]),
}
