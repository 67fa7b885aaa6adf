"""Writes tests/golden/qlognei_terms.npz: the scalar terms of log-space noisy expected improvement, L(a) = log softplus(a) =
log log(1 + exp(a)) and R(a) = L'(a) = sigmoid(a) / softplus(a), from mpmath at 50 digits (the exact functions, not the header's
branches), rounded to double, on a = +-{0, 1e-3, 0.5413, 3, 35.9999, 36.0001, 40, 700, 745.2, 800, 1e4, 1e9} and 200 log-spaced
magnitudes 1e-6 .. 1e9 on each side.
Run from the repository root: python tests/golden/make_qlognei_fixtures.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50


def terms(a):
    a = mp.mpf(float(a))
    # mpmath's exponent range is unbounded: exp(-1e9) is a number, and log1p keeps its 50 digits
    sp = mp.log1p(mp.exp(a))
    return float(mp.log(sp)), float(1 / ((1 + mp.exp(-a)) * sp))


def main():
    pts = np.array([0.0, 1e-3, 0.5413, 3.0, 35.9999, 36.0001, 40.0, 700.0, 745.2, 800.0, 1e4, 1e9])
    mags = np.logspace(-6, 9, 200)
    a = np.concatenate([pts, -pts[1:], mags, -mags])
    v = np.array([terms(x) for x in a])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "qlognei_terms.npz")
    np.savez(out, a=a, L=v[:, 0], R=v[:, 1])
    print(out, a.size, "points")


if __name__ == "__main__":
    main()
