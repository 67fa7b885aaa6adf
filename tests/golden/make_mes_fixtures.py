"""Writes tests/golden/mes_terms.npz: the scalar terms of max-value entropy search, g(t) = 1/2 t r - log Phi and
g'(t) = -1/2 r (1 + t (t + r)) with r = phi / Phi, from mpmath at 60 digits, rounded to double, on
t = -logspace(4, -3, 141), 0, logspace(-3, log10(38), 80).  Run from the repository root: python tests/golden/make_mes_fixtures.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60


def terms(t):
    t = mp.mpf(float(t))
    # 1 + t^2 + t r cancels to ~2 / t^2: 16 of the 60 digits at t = -1e4; mpmath's exponent range has no Phi that underflows
    Phi, phi = mp.ncdf(t), mp.npdf(t)
    r = phi / Phi
    return float(mp.mpf("0.5") * t * r - mp.log(Phi)), float(-mp.mpf("0.5") * r * (1 + t * t + t * r))


def main():
    t = np.concatenate([-np.logspace(4, -3, 141), [0.0], np.logspace(-3, np.log10(38), 80)])
    gd = np.array([terms(v) for v in t])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mes_terms.npz")
    np.savez(out, t=t, g=gd[:, 0], dg=gd[:, 1])
    print(out, t.size, "points")


if __name__ == "__main__":
    main()
