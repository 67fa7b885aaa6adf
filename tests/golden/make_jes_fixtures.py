"""Writes tests/golden/jes_terms.npz: the scalar terms of joint entropy search, tau(t) = 1 - r (t + r) and
tau'(t) = r ((t + r)(t + 2 r) - 1) with r = phi / Phi, from mpmath at 60 digits, rounded to double, on 201 points of [-1e4, 38]:
t = -logspace(4, -3, 90), 41 points of [-30.5, -29.5] (the switch to the series), 0, 29 points of +-[1e-8, 1e-4] and of [-0.05, 0.05]
(around 0, where the branch changes), logspace(-3, log10(38), 40).  Run from the repository root: python tests/golden/make_jes_fixtures.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import jes_ref  # noqa: E402


def grid():
    near0 = np.concatenate([-np.logspace(-8, -4, 7), np.logspace(-8, -4, 7), np.linspace(-0.05, 0.05, 15)])
    return np.concatenate([-np.logspace(4, -3, 90), np.linspace(-30.5, -29.5, 41), [0.0], near0, np.logspace(-3, np.log10(38), 40)])


def main():
    t = grid()
    # tau = 1 - r (t + r) cancels to ~1 / t^2 and tau' to ~2 / |t|^3: 24 of the 60 digits at t = -1e4
    td = np.array([[float(a) for a in jes_ref.terms_mp(v, 60)] for v in t])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jes_terms.npz")
    np.savez(out, t=t, tau=td[:, 0], dtau=td[:, 1])
    print(out, t.size, "points")


if __name__ == "__main__":
    main()
