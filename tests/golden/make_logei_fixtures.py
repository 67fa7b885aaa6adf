"""Writes tests/golden/logei_terms.npz: the scalar terms of log expected improvement, log h(u), Phi / h and phi / h with
h = phi + u Phi, from mpmath at 60 digits, rounded to double, on
u = -logspace(12, -6, 361), logspace(-6, 10, 321), linspace(-45, 10, 441), and 0, +-1, -30 with its two neighbours, -38.6.
Run from the repository root: python tests/golden/make_logei_fixtures.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60


def terms(u):
    u = mp.mpf(float(u))
    # phi + u Phi cancels to ~phi / u^2: 24 of the 60 digits at u = -1e12; mpmath's exponent range has no Phi that underflows
    Phi, phi = mp.ncdf(u), mp.npdf(u)
    h = phi + u * Phi
    return float(mp.log(h)), float(Phi / h), float(phi / h)


def main():
    u = np.concatenate([-np.logspace(12, -6, 361), np.logspace(-6, 10, 321), np.linspace(-45.0, 10.0, 441),
                        [0.0, 1.0, -1.0, -30.0, np.nextafter(-30.0, -np.inf), np.nextafter(-30.0, np.inf), -38.6]])
    v = np.array([terms(x) for x in u])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "logei_terms.npz")
    np.savez(out, u=u, log_h=v[:, 0], b1=v[:, 1], b2=v[:, 2])
    print(out, u.size, "points")


if __name__ == "__main__":
    main()
