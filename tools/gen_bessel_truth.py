"""Correctly rounded Bessel values for the tests of eigensolver_amd/csrc/es_bessel.hpp.

    python tools/gen_bessel_truth.py            # writes tests/golden/bessel_truth.npz

mpmath at 40 significant digits, every value rounded once to the nearest double -- a reference that is exact to half an
ulp, where scipy.special (tests/test_hostmath.py) is itself a few ulp off.  Two point sets:

  ik_n, ik_x     orders {0, 1, 2, 3, 5, 10, 11, 20, 40} x arguments log-spaced over [1e-6, 700], plus 0.5 and 2.0 (the
                 branch points of ie_pair_from_k and ke01) with both neighbouring doubles
  ik_ke0/ke1     e^x K_n(x), e^x K_{n+1}(x)
  ik_ie0/ie1     e^-x I_n(x), e^-x I_{n+1}(x)      (the ascending series ie_pair is meant for x <= 60: the tests select)
  jy_n, jy_x     the same orders x arguments log-spaced over [1e-5, 80], plus the doubles next to the first three zeros of
                 J_n and of Y_n (the nearest double and 4 ulp to either side)
  jy_j0/j1/y0/y1 J_n, J_{n+1}, Y_n, Y_{n+1}

Rows with a value outside [1e-290, 1e290] are left out (order 40 at the smallest arguments: I_41 is subnormal there and
a relative error says nothing).  The tests read the file only; mpmath is needed to regenerate it, not to run them.
"""
import os

import mpmath as mp
import numpy as np

ORDERS = (0, 1, 2, 3, 5, 10, 11, 20, 40)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "bessel_truth.npz")
LO, HI = 1e-290, 1e290


def _neighbours(x):
    return [np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)]


def ik_arguments():
    xs = list(np.logspace(-6, np.log10(700.0), 160))
    xs += _neighbours(0.5) + _neighbours(2.0)
    return np.array(sorted(set(float(x) for x in xs)))


def jy_arguments(n):
    xs = list(np.logspace(-5, np.log10(80.0), 136))
    for zero in (mp.besseljzero, mp.besselyzero):
        for m in (1, 2, 3):
            z = float(zero(n, m))                      # nearest double to the zero
            if z < 80.0:
                u = np.spacing(z)
                xs += [z - 4 * u, z, z + 4 * u]
    return np.array(sorted(set(float(x) for x in xs)))


def main():
    mp.mp.dps = 40
    ik = {k: [] for k in ("n", "x", "ke0", "ke1", "ie0", "ie1")}
    jy = {k: [] for k in ("n", "x", "j0", "j1", "y0", "y1")}
    for n in ORDERS:
        for x in ik_arguments():
            X = mp.mpf(x)                              # exact: the argument IS the double
            ex = mp.exp(X)
            v = [float(ex * mp.besselk(n, X)), float(ex * mp.besselk(n + 1, X)),
                 float(mp.besseli(n, X) / ex), float(mp.besseli(n + 1, X) / ex)]
            if all(LO < abs(t) < HI for t in v):
                for key, t in zip(("n", "x", "ke0", "ke1", "ie0", "ie1"), [n, x] + v):
                    ik[key].append(t)
        for x in jy_arguments(n):
            X = mp.mpf(x)
            v = [float(mp.besselj(n, X)), float(mp.besselj(n + 1, X)), float(mp.bessely(n, X)), float(mp.bessely(n + 1, X))]
            if all(abs(t) < HI for t in v) and LO < np.hypot(v[0], v[2]) and LO < np.hypot(v[1], v[3]):
                for key, t in zip(("n", "x", "j0", "j1", "y0", "y1"), [n, x] + v):
                    jy[key].append(t)
    arrays = {}
    for tag, d in (("ik", ik), ("jy", jy)):
        for key, vals in d.items():
            arrays[f"{tag}_{key}"] = np.asarray(vals, dtype=np.int32 if key == "n" else np.float64)
    np.savez_compressed(OUT, **arrays)
    print(OUT, {k: v.shape for k, v in arrays.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
