"""eigensolver_amd/csrc/es_bessel_complex.hpp and es_cjet.hpp compiled for the host (tests/hostmath/hostmath_complex.cpp,
test-only harness): the scaled modified Bessel functions at complex argument against scipy.special.kve / ive (AMOS), and
-- with their z-derivatives (the CJet<1> forms) and the primitives of the complex scalar -- against the correctly rounded
values of tests/golden/bessel_complex_truth.npz (mpmath at 40 digits; tests/bessel_complex_truth.py).

Against scipy:

Region: orders 0 ... 11, |z| in [1e-3, 300], arg z in {-pi/4, 0, pi/8, pi/4} (the sector the exterior of the cylinder needs:
mu = principal sqrt(m_e) with Re m_e >= 0), with points packed around |z| = 2 (series / continued fraction) and |z| = 0.5
(series / backward recurrence of I).  scipy's ive scales by e^-|Re z|, the header by e^-z: the reference is multiplied by
e^{-i Im z}.

Worst relative error |f - f_ref| / |f_ref| of the host build on these points (the figures of DESIGN 8i):
  e^z K_n, K_{n+1}     4.9e-15  at n = 1, z = 1.98 (K_MEASURED)
  e^-z I_n, I_{n+1}    1.92e-14 at n = 9, |z| = 0.0042, arg z = pi/8 (I_MEASURED): the error of scipy's ive at small |z| -- mpmath
                       at 40 digits has this header within 3e-16 there and scipy 1.9e-14 off
The tests assert twice these figures, rounded up to one digit; the host build is deterministic, the factor covers another libm.
Both are far below 1e-12, the level at which a loss would mean a cancellation in the method.

Against the fixture (orders 0, 1, 2, 3, 5, 10, 11, 20, 40; nine angles in [-pi/4, pi/4]; |z| in [1e-6, 700] with both sides of
the branches at |z| = 2 and 0.5; |z| = 3e3 and 3e4 apart), worst error per order in u = 2^-52, measured here and recorded as
bessel_complex_truth.E_HOST_C (|z| <= 700) and E_HOST_C_FAR; test_truth_complex holds the host build to them with 25 %
headroom, rounded up to a whole u.  Values relative to |f|, derivatives relative to (|f_n| + |f_{n+1}|)(1 + (n + 1) / |z|):
  |z| <= 700   cke_pair            32.08 24.04 15.60 15.60 15.08 13.67 14.13 22.26 41.54
               cie_pair_from_k     16.11 15.66 14.84 15.97 15.89 14.27 14.91 20.74 37.60
               cke_pair, d/dz      12.62  5.46  4.43  5.71  7.56 12.16 14.74 22.81 41.94
               cie_pair_from_k, d/dz 2.13  1.15  1.68  3.10  5.84  8.63 10.08 17.20 34.74
  |z| > 700    cke_pair             2.86  2.86  2.86  2.86  3.51  3.46  3.46  3.35  3.10
               cie_pair_from_k      3.32  3.76  3.49  3.40  4.38  2.94  2.63  3.00  3.39
               cke_pair, d/dz       0.50  0.44  0.50  0.63  0.74  0.80  0.92  0.91  0.72
               cie_pair_from_k, d/dz 2.17  1.47  1.91  1.74  1.76  2.50  1.97  1.68  1.08
With Miller's start index sized by |z| (before it was sized by |z|^2 / Re z) cie_pair_from_k and its derivatives stood at
1350 u (order 0) ... 169 u (order 40) at |z| = 3e4, arg z = -pi/4, and the derivatives at 9.8 u at |z| = 391, arg z = -pi/4.

Primitives, worst error in u of the modulus of the true result on the fixture's 400 arguments each (moduli 1e-100 ... 1e100,
exp: up to 700; all quadrants, the axes with both signs of zero):
  cz_sqrt 0.89   cz_log 0.61   cz_exp 1.00   cz / cz 1.42   double / cz 1.45
Counted from the operations, each libm call taken as 1 u and each IEEE operation as 1/2:
  sqrt       hypot 1, the sum 1/2; the root halves both and adds 1/2: 1.25 on the larger part; the quotient for the other
             part 1/2 more: below 2
  log        hypot 1 passes into log as an absolute error, log 1 on the real part; atan2 1 on the imaginary: below 2
  exp        exp 1 and cos or sin 1 on either part: 2.  |Im z| u more is allowed, for a libm whose cos and sin reduce their
             argument with a rounded pi (the error of the result is then |Im z| u / 2 ... u); glibc's do not need it
  divisions  two products 1/2 each against |a| |b|, their sum 1/2, |b|^2 1, the quotient 1/2: 3
The assertions keep these counted bounds (2 u, 2 u + |Im z| u, 3 u); the measured figures are all below 1.5 u.  On the
negative real axis the sign of the imaginary part of sqrt and log follows the sign of the zero, exactly.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import special as sp

from tests import bessel_complex_truth as bc

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
    deps = [src] + [os.path.join(csrc, h) for h in ("es_cjet.hpp", "es_bessel_complex.hpp", "es_bessel.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    for f in (lib.hmc_ke_pair, lib.hmc_ie_pair_from_k):
        f.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    vp, i = ctypes.c_void_p, ctypes.c_int
    for name, nptr in (("ke_pair_v", 4), ("ie_pair_from_k_v", 4), ("ke_pair_jet_v", 6), ("ie_pair_from_k_jet_v", 6)):
        getattr(lib, "hmc_" + name).argtypes = [vp, vp, i] + [vp] * (nptr - 2)
    for name in ("sqrt", "log", "exp"):
        getattr(lib, f"hmc_{name}_v").argtypes = [vp, i, vp]
    lib.hmc_div_v.argtypes = lib.hmc_rdiv_v.argtypes = [vp, vp, i, vp]
    lib.hmc_cf2_passes_v.argtypes = [vp, i, vp, vp]
    return lib


@pytest.fixture(scope="module")
def truth():
    return bc.load()


def _ptr(a):
    assert a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.c_void_p)


def _rows(lib, name, truth, nout):
    """the array entry point `name` on every Bessel row of the fixture -> nout complex arrays"""
    n, z = np.ascontiguousarray(truth["c_n"], dtype=np.int32), np.ascontiguousarray(truth["c_z"])
    outs = [np.full(len(n), complex(np.nan, np.nan)) for _ in range(nout)]
    getattr(lib, name)(_ptr(n), _ptr(z), len(n), *[_ptr(o) for o in outs])
    return outs


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


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


@pytest.mark.parametrize("func", bc.FUNCTIONS)
def test_truth_complex(hmc, truth, func):
    """Against the correctly rounded values of the fixture: the worst error per order stays within the measured E_HOST_C
    (|z| <= 700) and E_HOST_C_FAR (|z| > 700) plus 25 %, rounded up to a whole u = 2^-52; every row gives a finite result;
    component 0 of the jet forms is the plain routine bit for bit; beyond 700, I stays at the level it has below."""
    pair = "ke_pair" if func.startswith("cke") else "ie_pair_from_k"
    plain = _rows(hmc, f"hmc_{pair}_v", truth, 2)
    jet = _rows(hmc, f"hmc_{pair}_jet_v", truth, 4)
    assert len(plain[0]) > 3500
    assert _same_bits(plain[0], jet[0]) and _same_bits(plain[1], jet[1])
    err = bc.errors(truth, func, jet[2:] if func.endswith("_d") else plain)
    for far, table in ((False, bc.E_HOST_C), (True, bc.E_HOST_C_FAR)):
        worst = bc.worst_per_order(truth, err, far)
        print(func, "|z| > 700" if far else "|z| <= 700", "E_host [u]:", {o: (round(e, 2), za) for o, (e, za) in worst.items()})
        for order, (e, z_at) in worst.items():
            assert e <= math.ceil(1.25 * table[func][order]), (func, far, order, e, z_at)
            if far:
                assert e <= math.ceil(1.25 * bc.E_HOST_C[func][order]), (func, order, e, z_at)


def test_cf2_passes(hmc, truth):
    """The CF2 loop of cke01 restated in the harness with a counter gives the header's K_0 bit for bit on every row beyond
    |z| = 2, so it counts the header's passes; their maximum per band of |z| is what bessel_complex_truth.CF2_PASSES says
    (the device margin is counted from it), and the fixture has rows on both sides of index 64, where the reciprocal tables
    of the device end."""
    z = np.ascontiguousarray(truth["c_z"][truth["c_n"] == 0])
    n = np.zeros(len(z), dtype=np.int32)
    k0, k1 = np.zeros(len(z), dtype=complex), np.zeros(len(z), dtype=complex)
    hmc.hmc_ke_pair_v(_ptr(n), _ptr(z), len(z), _ptr(k0), _ptr(k1))
    passes, k0_restated = np.full(len(z), -1, dtype=np.int32), np.zeros(len(z), dtype=complex)
    hmc.hmc_cf2_passes_v(_ptr(z), len(z), _ptr(passes), _ptr(k0_restated))
    cf2 = z.real * z.real + z.imag * z.imag > 4.0
    assert np.array_equal(passes > 0, cf2) and 100 < cf2.sum() < len(z) - 100
    assert _same_bits(k0[cf2], k0_restated[cf2])
    lo = 0.0
    for hi, most in bc.CF2_PASSES:
        band = cf2 & (np.abs(z) > lo) & (np.abs(z) <= hi)
        assert band.sum() >= 9 and passes[band].max() == most, (hi, band.sum(), passes[band].max())
        lo = hi
    assert (passes[cf2] + 1 >= bc.CF2_TABLE).sum() > 30 and (passes[cf2] + 1 < bc.CF2_TABLE).sum() > 30


def test_fixture_straddles_the_branches(truth):
    """Every angle has rows on either side of re^2 + im^2 <= 4 (cke01) and of hypot < 0.5 (cie_pair_from_k) within 1e-9 of
    the branch point, and the arguments lie in the sector Re z^2 >= 0."""
    z = truth["c_z"]
    assert np.all(z.real * z.real - z.imag * z.imag >= 0.0) and np.all(z.real > 0.0)
    abs2, hyp = z.real * z.real + z.imag * z.imag, np.hypot(z.real, z.imag)
    for ia in range(9):
        for order in bc.ORDERS:
            sel = (truth["c_angle"] == ia) & (truth["c_n"] == order)
            near2, near05 = sel & (np.abs(hyp - 2.0) < 1e-9), sel & (np.abs(hyp - 0.5) < 1e-9)
            assert (abs2[near2] <= 4.0).any() and (abs2[near2] > 4.0).any(), (ia, order)
            assert (hyp[near05] < 0.5).any() and (hyp[near05] >= 0.5).any(), (ia, order)


@pytest.mark.parametrize("name", bc.PRIMITIVES)
def test_primitives_complex(hmc, truth, name):
    want = truth[name + "_w"]
    got = np.full(len(want), complex(np.nan, np.nan))
    if name in ("div", "rdiv"):
        a, b = np.ascontiguousarray(truth[name + "_a"]), np.ascontiguousarray(truth[name + "_b"])
        assert 1e-150 <= np.abs(b).min() and np.abs(b).max() <= 1e150
        getattr(hmc, f"hmc_{name}_v")(_ptr(a), _ptr(b), len(want), _ptr(got))
    else:
        getattr(hmc, f"hmc_{name}_v")(_ptr(np.ascontiguousarray(truth[name + "_z"])), len(want), _ptr(got))
    assert len(want) >= 400
    bc.primitive_checks(truth, name, got)
