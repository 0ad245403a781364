"""eigensolver_amd/csrc/es_bessel_complex.hpp compiled for the host (tests/hostmath/hostmath_complex.cpp, test-only harness):
the scaled modified Bessel functions at complex argument against scipy.special.kve / ive (AMOS).

Region: orders 0 ... 11, |z| in [1e-3, 300], arg z in {-pi/4, 0, pi/8, pi/4} (the sector the exterior of the cylinder needs:
mu = principal sqrt(m_e) with Re m_e >= 0), with points packed around |z| = 2 (series / continued fraction) and |z| = 0.5
(series / backward recurrence of I).  scipy's ive scales by e^-|Re z|, the header by e^-z: the reference is multiplied by
e^{-i Im z}.

Worst relative error |f - f_ref| / |f_ref| of the host build on these points (the figures of the header comment):
  e^z K_n, K_{n+1}     4.9e-15  at n = 1, z = 1.98 (K_MEASURED)
  e^-z I_n, I_{n+1}    1.92e-14 at n = 9, |z| = 0.0042, arg z = pi/8 (I_MEASURED): the error of scipy's ive at small |z| -- mpmath
                       at 40 digits has this header within 3e-16 there and scipy 1.9e-14 off
The tests assert twice these figures, rounded up to one digit; the host build is deterministic, the factor covers another libm.
Both are far below 1e-12, the level at which a loss would mean a cancellation in the method."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from scipy import special as sp

HERE = os.path.dirname(os.path.abspath(__file__))
K_MEASURED, I_MEASURED = 4.9e-15, 1.92e-14
K_BOUND, I_BOUND = 1e-14, 4e-14

ORDERS = range(11)                                   # the pairs (n, n + 1): orders 0 ... 11
ARGS = (-np.pi / 4, 0.0, np.pi / 8, np.pi / 4)
RADII = np.unique(np.concatenate([np.logspace(-3, np.log10(300.0), 160), np.linspace(1.9, 2.1, 41), 2.0 + np.array([-1e-9, 0.0, 1e-9]),
                                  np.linspace(0.45, 0.55, 21), 0.5 + np.array([-1e-9, 0.0, 1e-9])]))


@pytest.fixture(scope="module")
def hmc():
    src = os.path.join(HERE, "hostmath", "hostmath_complex.cpp")
    so = os.path.join(HERE, "hostmath", "libhostmath_complex.so")
    csrc = os.path.join(HERE, "..", "eigensolver_amd", "csrc")
    deps = [src, os.path.join(csrc, "es_bessel_complex.hpp"), os.path.join(csrc, "es_bessel.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    for f in (lib.hmc_ke_pair, lib.hmc_ie_pair_from_k):
        f.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    return lib


def worst(f, ref):
    """(worst relative error, (n, z) where) of f(n, z) -> (order n, order n + 1) against ref(order, z)."""
    out = (ctypes.c_double * 4)()
    w, at = 0.0, None
    for n in ORDERS:
        for a in ARGS:
            for r in RADII:
                z = r * np.exp(1j * a)
                f(n, z.real, z.imag, out)
                got = (complex(out[0], out[1]), complex(out[2], out[3]))
                for j in (0, 1):
                    want = ref(n + j, z)
                    if not np.isfinite(want):
                        continue                       # K_n overflows at small |z| and large n
                    assert np.isfinite(got[j]), (n + j, z)
                    e = abs(got[j] - want) / abs(want)
                    if e > w:
                        w, at = e, (n + j, z)
    return w, at


def test_scaled_K_complex(hmc):
    w, at = worst(hmc.hmc_ke_pair, lambda n, z: sp.kve(n, z))
    print(f"e^z K_n: worst relative error {w:.3e} at (n, z) = {at}")
    assert w < K_BOUND, (w, at)


def test_scaled_I_complex(hmc):
    w, at = worst(hmc.hmc_ie_pair_from_k, lambda n, z: sp.ive(n, z) * np.exp(-1j * z.imag))
    print(f"e^-z I_n: worst relative error {w:.3e} at (n, z) = {at}")
    assert w < I_BOUND, (w, at)


def test_real_axis_is_the_real_routine(hmc):
    """On the real axis the complex routines agree with the real ones of es_bessel.hpp (same series; Chebyshev there, CF2
    here beyond 2) to the accuracy both hold, and their imaginary parts vanish."""
    out = (ctypes.c_double * 4)()
    for n in (0, 1, 3, 11):
        for x in (0.01, 0.7, 1.999, 2.001, 9.0, 150.0):
            hmc.hmc_ke_pair(n, x, 0.0, out)
            assert out[1] == 0.0 and out[3] == 0.0
            assert abs(out[0] / sp.kve(n, x) - 1) < K_BOUND and abs(out[2] / sp.kve(n + 1, x) - 1) < K_BOUND
