"""Shared by tests/test_hostmath_complex.py (host build of csrc/es_bessel_complex.hpp and es_cjet.hpp) and
tests/test_devmath_gpu.py (device build): the correctly rounded values of tests/golden/bessel_complex_truth.npz
(tools/gen_bessel_truth.py, mpmath at 40 digits), the error measures, the measured worst errors of the host build (E_HOST_C,
E_HOST_C_FAR) and the margin the device paths get on top of them.

Errors are in units of u = 2^-52, of complex numbers by modulus:
  values        |got - true| / |true| / u
  derivatives   |got - true| / ((|f_n| + |f_{n+1}|) (1 + (n + 1) / |z|)) / u  -- the scale of the terms the identities of
                es_cjet.hpp sum; the derivative itself is smaller than its terms by about 2 |z| at large |z|
"""
import os

import numpy as np

from tests.bessel_truth import ORDERS, U

# the *_d entries are the derivative components of the CJet<1> forms of the two pairs, z the variable
FUNCTIONS = ("cke_pair", "cie_pair_from_k", "cke_pair_d", "cie_pair_from_k_d")
PRIMITIVES = ("sqrt", "log", "exp", "div", "rdiv")

# Worst error of the HOST build (g++ -O2 -ffp-contract=off, glibc libm) per function and order on the rows with |z| <= 700,
# in u, as measured by test_hostmath_complex.py::test_truth_complex (which holds the host build to these figures with 25 %
# headroom).  Against mpmath, never against the device.
E_HOST_C = {
    # orders 0 ... 10: worst at |z| = 2 (arg z = -1e-3) or 1.98, where the ascending series of K_0 subtracts terms 12 times
    # the result; 11, 40: |z| = 0.063, arg z = -pi/4; 20: |z| = 1e-6 -- the upward recurrence
    "cke_pair":          {0: 32.08, 1: 24.04, 2: 15.60, 3: 15.60, 5: 15.08, 10: 13.67, 11: 14.13, 20: 22.26, 40: 41.54},
    # orders 0 ... 10: |z| = 1.98, inherited from K; 20, 40: |z| = 0.5, arg z = -pi/4
    "cie_pair_from_k":   {0: 16.11, 1: 15.66, 2: 14.84, 3: 15.97, 5: 15.89, 10: 14.27, 11: 14.91, 20: 20.74, 40: 37.60},
    "cke_pair_d":        {0: 12.62, 1: 5.46, 2: 4.43, 3: 5.71, 5: 7.56, 10: 12.16, 11: 14.74, 20: 22.81, 40: 41.94},
    "cie_pair_from_k_d": {0: 2.13, 1: 1.15, 2: 1.68, 3: 3.10, 5: 5.84, 10: 8.63, 11: 10.08, 20: 17.20, 40: 34.74},
}
# The same on the rows with |z| > 700 (|z| = 3e3 and 3e4, nine angles: 18 rows per order).  With the start index of Miller's
# recurrence sized by |z| alone, as it was before it was sized by |z|^2 / Re z, the row |z| = 3e4, arg z = -pi/4 of
# cie_pair_from_k stood at 1349.81, 1283.18, 1215.55, 1154.61, 1041.90, 800.80, 761.53, 479.38, 168.66 u for these orders
# (and its derivatives the same), every other row as now.
E_HOST_C_FAR = {
    "cke_pair":          {0: 2.86, 1: 2.86, 2: 2.86, 3: 2.86, 5: 3.51, 10: 3.46, 11: 3.46, 20: 3.35, 40: 3.10},
    "cie_pair_from_k":   {0: 3.32, 1: 3.76, 2: 3.49, 3: 3.40, 5: 4.38, 10: 2.94, 11: 2.63, 20: 3.00, 40: 3.39},
    "cke_pair_d":        {0: 0.50, 1: 0.44, 2: 0.50, 3: 0.63, 5: 0.74, 10: 0.80, 11: 0.92, 20: 0.91, 40: 0.72},
    "cie_pair_from_k_d": {0: 2.17, 1: 1.47, 2: 1.91, 3: 1.74, 5: 1.76, 10: 2.50, 11: 1.97, 20: 1.68, 40: 1.08},
}
# Most passes through the CF2 loop of cke01 on the fixture's rows with |z| up to the given radius (beyond the one before), as
# the host harness counts them (test_hostmath_complex.py::test_cf2_passes): 102 at z = sqrt 2 (1 - i); the 324 rows next to
# |z| = 2 take 87 or more, past the reciprocal tables
CF2_PASSES = ((2.5, 102), (5.0, 60), (20.0, 37), (100.0, 17), (700.0, 8), (np.inf, 5))
CF2_TABLE = 64                       # kRcpTable of es_bessel.hpp
SERIES_CANCELLATION = 12             # "the series of K_0 subtracts terms 12 times the result" (es_bessel_complex.hpp)


def device_margin_c(func, z):
    """What the device build may add to E_HOST_C[func][n] on the row of argument z (an array: per row), in u: one u for
    every operation on the row's path whose result can differ from the host's, counted from es_bessel_complex.hpp, times the
    cancellation factor of the sum it feeds.  Complex sums, products and every '/' (operator/ of cz, 1 / z, 2 / z, n / z)
    are IEEE operations without contraction on both sides and count nothing: so the upward recurrence of cke_pair, Miller's
    recurrence and the identities of es_cjet.hpp add nothing of their own, and the order does not enter.

    cke01, re^2 + im^2 <= 4   the series: cz_log(z / 2) = (log(hypot), atan2) feeds lg, whose products with i0, i1 are the
                              terms that cancel: 3 x 12; cz_exp(z) = exp x (cos, sin) multiplies the result: 3 x 1.  The
                              1 / k table holds the correctly rounded reciprocals and every use is 1.0 * table[k], the
                              quotient the host computes: no difference.                                            39
    cke01, beyond             CF2: hypot and sqrt in cz_sqrt(pi / 2z): 2.  Per pass of the loop, c = qdiv_int(-a c, i) is a product
                              with the rounded 1 / i below index 64 and qdiv beyond, where the host divides -- c carries
                              it into every later pass: 1 per pass; qdiv_cf2a(1, i, a) is the host's quotient below index
                              64 and qdiv beyond: 1 per pass from index 64.  The terms of Temme's sums are of one sign on
                              the real axis: factor 1.  With P the most passes on the fixture at the row's radius
                              (CF2_PASSES; the last index is P + 1):  2 + P + max(0, P + 1 - 63)
                              |z| <= 2.5: 144;  <= 5: 62;  <= 20: 39;  <= 100: 19;  <= 700: 10;  beyond: 7
    cke_pair                  K_0, K_1 as above; the recurrence is IEEE on both sides and stable
    cie_pair_from_k           hypot(z) < 0.5: cie_pair, cz_exp(-z): 3, on rows that are on the series side of cke01;
                              otherwise 1 / (z (f K_n + K_{n+1})) with f from IEEE operations (hypot only sizes the
                              recurrence, 6+ orders beyond need): it inherits the error of K_n, K_{n+1} -- as cke_pair
    *_d                       sums of the values with IEEE factors, measured against the scale of their terms: as the values
    """
    assert func in FUNCTIONS
    z = np.asarray(z)
    series = z.real * z.real + z.imag * z.imag <= 4.0            # as cz_abs2 forms it
    passes = np.array([p for _, p in CF2_PASSES])[np.searchsorted([r for r, _ in CF2_PASSES], np.abs(z))]
    cf2 = 2 + passes + np.maximum(0, passes + 1 - (CF2_TABLE - 1))
    return np.where(series, 3 * SERIES_CANCELLATION + 3, cf2).astype(np.float64)


def load():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bessel_complex_truth.npz"))
    return {k: z[k] for k in z.files}


def true_values(truth, func):
    """(f_n, f_{n+1}, d/dz f_n, d/dz f_{n+1}) of the pair `func` (or `func`_d) evaluates"""
    t = "ke" if func.startswith("cke") else "ie"
    return tuple(truth[f"c_{p}{t}{j}"] for p in ("", "d") for j in (0, 1))


def errors(truth, func, got):
    """Per-row error in u (the larger of the two outputs' errors).  got: (f_n, f_{n+1}) for a value function, (d f_n,
    d f_{n+1}) for a *_d one, complex arrays over the fixture's rows."""
    n, z = truth["c_n"], truth["c_z"]
    f0, f1, d0, d1 = true_values(truth, func)
    if func.endswith("_d"):
        scale = (np.abs(f0) + np.abs(f1)) * (1.0 + (n + 1.0) / np.abs(z))
        errs = [np.abs(got[0] - d0) / scale, np.abs(got[1] - d1) / scale]
    else:
        errs = [np.abs(got[0] - f0) / np.abs(f0), np.abs(got[1] - f1) / np.abs(f1)]
    err = np.max(np.stack(errs), axis=0) / U
    return np.where(np.isfinite(err), err, np.inf)            # a NaN result is an infinite error, not a skipped row


def worst_per_order(truth, err, far):
    """{order: (worst error in u, argument where it occurs)} over the rows with |z| > 700 (far) or the others"""
    out = {}
    n, z = truth["c_n"], truth["c_z"]
    for order in ORDERS:
        sel = np.where((n == order) & (truth["c_far"] == far))[0]
        assert sel.size > (10 if far else 200), (order, sel.size)
        i = sel[np.argmax(err[sel])]
        out[order] = (float(err[i]), complex(z[i]))
    return out


def primitive_errors(truth, name, got):
    """Per-row error of a primitive in u of the modulus of the true result (0 / 0: exact or infinite)"""
    true = truth[name + "_w"]
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - true) / np.abs(true) / U
    err = np.where(np.abs(true) == 0.0, np.where(got == true, 0.0, np.inf), err)
    return np.where(np.isfinite(err), err, np.inf)


# u of the modulus of the true result; exp: plus |Im z| u (the docstring of tests/test_hostmath_complex.py has the count)
PRIMITIVE_BOUND = {"sqrt": 2.0, "log": 2.0, "exp": 2.0, "div": 3.0, "rdiv": 3.0}


def primitive_checks(truth, name, got):
    """What both legs assert of a primitive's results `got`: the bound per row, and on the negative real axis the sign of
    the imaginary part of sqrt and log follows the sign of the zero exactly (sqrt: with real part +0)."""
    err = primitive_errors(truth, name, got)
    arg = truth[name + "_b"] if name in ("div", "rdiv") else truth[name + "_z"]
    bound = PRIMITIVE_BOUND[name] + (np.abs(arg.imag) if name == "exp" else 0.0)
    i = int(np.argmax(err - bound))
    print(f"cz {name}: worst {err.max():.3f} u at {arg[int(np.argmax(err))]!r}")
    assert np.all(err <= bound), (name, arg[i], got[i], truth[name + "_w"][i], err[i])
    if name in ("sqrt", "log"):
        cut = (arg.real < 0.0) & (arg.imag == 0.0)
        assert cut.sum() == 20 and np.signbit(arg.imag[cut]).sum() == 10
        assert np.array_equal(np.signbit(got.imag[cut]), np.signbit(arg.imag[cut]))
        assert np.all(got.imag[cut] != 0.0)
        if name == "sqrt":
            assert np.all(got.real[cut] == 0.0) and not np.signbit(got.real[cut]).any()
            zero = arg == 0.0
            assert zero.sum() == 1 and np.all(got[zero] == 0.0)
