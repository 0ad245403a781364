"""Shared by tests/test_hostmath.py (host build of csrc/es_bessel.hpp) and tests/test_devmath_gpu.py (device build): the
correctly rounded Bessel values of tests/golden/bessel_truth.npz (tools/gen_bessel_truth.py, mpmath at 40 digits), the error
measures, the measured worst errors of the host build (E_HOST) and the margin the device paths get on top of them.

Errors are in units of u = 2^-52 ("ulp": the relative spacing of doubles is between u/2 and u):
  I, K   |got - true| / |true| / u
  J, Y   |got - true| / hypot(J_n, Y_n) / u  -- relative to the envelope, which has no zeros
"""
import os

import numpy as np

U = 2.0 ** -52
ORDERS = (0, 1, 2, 3, 5, 10, 11, 20, 40)
IE_SERIES_XMAX = 60.0                # the ascending series ie_pair is meant for x <~ 60 (es_bessel.hpp)
FUNCTIONS = ("ke_pair", "ie_pair", "ie_pair_from_k", "jy_pair")

# Worst error of the HOST build (g++ -O2 -ffp-contract=off, glibc libm) per function and order on the fixture, in u, as
# measured by test_hostmath.py::test_truth (which holds the host build to these figures with 25 % headroom).
E_HOST = {
    # worst at x = 2 - 2^-52 for most orders: the ascending series of K_0, K_1 subtracts terms 12 times the result there
    "ke_pair":        {0: 11.88, 1: 9.47, 2: 8.00, 3: 8.87, 5: 9.83, 10: 12.44, 11: 12.44, 20: 16.90, 40: 25.85},
    # worst at x = 47.5: ~70 series terms and exp(-x)
    "ie_pair":        {0: 9.69, 1: 9.55, 2: 11.26, 3: 12.13, 5: 9.13, 10: 9.32, 11: 6.79, 20: 6.28, 40: 6.27},
    # worst on x in [1.1, 2): it inherits the error of K there
    "ie_pair_from_k": {0: 12.26, 1: 14.99, 2: 13.99, 3: 11.37, 5: 11.90, 10: 14.16, 11: 12.97, 20: 17.72, 40: 27.72},
    # worst at x = 63.2 (order 40: x = 0.25): ~110 steps of the backward recurrence
    "jy_pair":        {0: 32.07, 1: 31.76, 2: 32.37, 3: 29.87, 5: 33.48, 10: 33.11, 11: 27.81, 20: 30.94, 40: 20.96},
}


def device_margin(func, n):
    """What the device build may add to E_HOST[func][n], in u: one ulp for every operation on its path whose result can
    differ from the host's, counted from es_bessel.hpp (the host divides, the device takes qdiv: 1.5 ulp against 0.5;
    log / exp / sqrt of two math libraries: <= 1 ulp each).  The 1/k table holds the correctly rounded reciprocals and
    every use is 1.0 * table[k], the quotient the host computes: no difference.  ie_pair, jy_pair and the Miller
    recurrence of ie_pair_from_k divide with '/', which is the IEEE quotient on both sides.

    ke_pair         x <= 2: log, exp, qdiv(1, x);  x > 2: qdiv(4, x), sqrt, qdiv(1, sqrt x) -- 3 either way; then
                    tox = qdiv(2, x) enters the upward recurrence once per order: 3 + n
    ie_pair         exp(-x): 1
    ie_pair_from_k  x < 0.5: ie_pair (1);  x >= 0.5: 1 / (x (f K_n + K_{n+1})), f and the rest IEEE on both sides (sqrt
                    only sizes the recurrence), a sum of positive terms, so it inherits the relative error of the
                    device's K_n, K_{n+1}: 3 + n
    jy_pair         log(x / 2): 1
    """
    return {"ke_pair": 3 + n, "ie_pair": 1, "ie_pair_from_k": 3 + n, "jy_pair": 1}[func]


def load():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bessel_truth.npz"))
    return {k: z[k] for k in z.files}


def points(truth, func):
    """(orders, arguments, tuple of true value arrays) of the fixture rows `func` is measured on."""
    if func == "jy_pair":
        return truth["jy_n"], truth["jy_x"], (truth["jy_j0"], truth["jy_j1"], truth["jy_y0"], truth["jy_y1"])
    n, x = truth["ik_n"], truth["ik_x"]
    if func == "ke_pair":
        return n, x, (truth["ik_ke0"], truth["ik_ke1"])
    sel = x <= IE_SERIES_XMAX if func == "ie_pair" else np.ones(x.shape, dtype=bool)
    return n[sel], x[sel], (truth["ik_ie0"][sel], truth["ik_ie1"][sel])


def errors(func, got, true):
    """Per-row error in u (the larger of the outputs' errors); got, true: tuples of arrays as points() orders them."""
    got = [np.asarray(g, dtype=np.float64) for g in got]
    if func == "jy_pair":
        e0, e1 = np.hypot(true[0], true[2]), np.hypot(true[1], true[3])
        errs = [np.abs(got[0] - true[0]) / e0, np.abs(got[1] - true[1]) / e1,
                np.abs(got[2] - true[2]) / e0, np.abs(got[3] - true[3]) / e1]
    else:
        errs = [np.abs(g - t) / np.abs(t) for g, t in zip(got, true)]
    err = np.max(np.stack(errs), axis=0) / U
    return np.where(np.isfinite(err), err, np.inf)            # a NaN result is an infinite error, not a skipped row


def worst_per_order(n, x, err):
    """{order: (worst error in u, argument where it occurs)}"""
    out = {}
    for order in ORDERS:
        sel = np.where(n == order)[0]
        assert sel.size > 50, (order, sel.size)
        i = sel[np.argmax(err[sel])]
        out[order] = (float(err[i]), float(x[i]))
    return out
