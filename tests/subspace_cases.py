"""Cases of the search over affine subspaces (sls_*_sub), shared by tests/test_gpu_subspace.py (the device held to tests/lbfgs_ref.py
driven by the device's own *_eval_sub) and tests/test_subspace_cpu.py (the same cases on the oracle's acquisition composed with the
map, to show that the inputs are not sensitive to the summation order).  Built on tests/maximize_cases.py, which stays as it is: its
generator, its starts (box_starts: uniform in [-0.2, 1.2], every third column rounded to a corner), N_LOCAL = 15 and VARIANTS.

Every shape: mc.problem(D, N, seed=N + D, ell=0.15 sqrt(D)), Matern 5/2, b = 0.05; rng = default_rng(900 + i); 129 starts
box_starts(d, 129, 900 + i); start j searches map 7 j mod n_maps, so neighbouring columns never share a map (n_maps > 1).
Kinds, per map k and in this order of rng calls:
  segment  a, b ~ U(0,1)^D;  c = a, A[:, 0] = b - a                                         (a slider: d = 1)
  box      lo, hi = clip(X[:, k] -+ 0.45, 0, 1);  c = lo, A = diag(hi - lo)                  (a trust region around data point k)
  centred  ctr ~ U(0.45, 0.55)^D, then B ~ N(0,1)^(D x d), every row scaled so that 0.5 sum_j |B_rj| = min(ctr_r, 1 - ctr_r);
           c = ctr - 0.5 B 1, A = B       (the image of [0,1]^d is centred at ctr and touches the cube: a full-scale embedding)
Order sensitivity of these inputs (test_subspace_cpu.py asserts at most 2 % per case and option set and prints it)."""
import numpy as np

import maximize_cases as mc

#            kind        D    N    d   n_maps acq
SHAPES = [("segment", 7, 200, 1, 5, mc.EI), ("segment", 7, 200, 1, 5, mc.UCB), ("centred", 20, 200, 2, 1, mc.UCB),
          ("centred", 20, 200, 2, 3, mc.EI), ("centred", 33, 90, 6, 3, mc.UCB), ("centred", 33, 90, 6, 3, mc.EI),
          ("box", 129, 90, 129, 3, mc.UCB), ("box", 17, 200, 17, 4, mc.EI)]
SEED = 900
S = 129
BOX_HALF = 0.45


def case_ids(shapes=None):
    return [(i, v) for i in (range(len(SHAPES)) if shapes is None else shapes) for v in mc.VARIANTS]


def shape_name(i):
    kind, D, N, d, K, acq = SHAPES[i]
    return f"sub{i}-{kind}-D{D}-N{N}-d{d}-maps{K}-{'EI' if acq == mc.EI else 'UCB'}"


def case_name(c):
    return f"{shape_name(c[0])}-{c[1]}"


def segment_maps(rng, D, K):
    A, c = np.zeros((K, D, 1)), np.zeros((K, D))
    for k in range(K):
        a, b = rng.uniform(0.0, 1.0, D), rng.uniform(0.0, 1.0, D)
        c[k], A[k, :, 0] = a, b - a
    return A, c


def box_maps(X, K, half=BOX_HALF):
    D = X.shape[0]
    A, c = np.zeros((K, D, D)), np.zeros((K, D))
    for k in range(K):
        lo, hi = np.clip(X[:, k] - half, 0.0, 1.0), np.clip(X[:, k] + half, 0.0, 1.0)
        c[k], A[k] = lo, np.diag(hi - lo)
    return A, c


def centred_maps(rng, D, d, K):
    A, c = np.zeros((K, D, d)), np.zeros((K, D))
    for k in range(K):
        ctr = rng.uniform(0.45, 0.55, D)
        B = rng.standard_normal((D, d))
        B *= (np.minimum(ctr, 1.0 - ctr) / (0.5 * np.abs(B).sum(axis=1)))[:, None]
        c[k], A[k] = ctr - 0.5 * B.sum(axis=1), B
    return A, c


class SubCase:
    """Inputs of one shape: X, y, theta, b, kernel, D, d, n_maps, acq, A (n_maps, D, d), c (n_maps, D), map_of_start (S,), starts
    (d x S), nvar = d.  The attribute names of maximize_cases.Case where they mean the same, so that mc.restated takes it."""

    def __init__(self, i):
        self.kind, D, N, d, K, self.acq = SHAPES[i]
        self.X, self.y, self.theta = mc.problem(D, N, seed=N + D, ell=0.15 * np.sqrt(D))
        self.kernel, self.b = mc.MATERN52, 0.05
        self.D, self.N, self.d, self.n_maps, self.nvar, self.S = D, N, d, K, d, S
        rng = np.random.default_rng(SEED + i)
        if self.kind == "segment":
            self.A, self.c = segment_maps(rng, D, K)
        elif self.kind == "box":
            self.A, self.c = box_maps(self.X, K)
        else:
            self.A, self.c = centred_maps(rng, D, d, K)
        self.starts = mc.box_starts(d, S, SEED + i)
        self.map_of_start = (7 * np.arange(S)) % K

    def eval_points(self, M, seed):
        """M points z in [0,1]^d with shuffled maps (map boundaries fall inside the 128-wide tiles): (Z d x M, map_of_point)."""
        rng = np.random.default_rng(seed)
        return rng.uniform(0.0, 1.0, (self.d, M)), rng.integers(0, self.n_maps, M)
