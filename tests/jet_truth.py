"""Shared by the real-jet tests of tests/test_devmath_gpu.py (not a test): tests/golden/jet_truth.npz (tools/gen_bessel_truth.py
jets, mpmath at 40 digits), the operator codes of dm_jet_op (tests/devmath/devmath_probe.hip), and the derived bounds.

All errors are in units of u = 2^-52 times a MAGNITUDE stored beside the true value: the header's expression for the component
with every sum replaced by the sum of the magnitudes of its terms and every product by the product of the magnitudes.  On that
scale a running error bound is a count of roundings, and a wrong sign or a dropped term is an error of order one, 2^52 u.

Counting rule (first order in u), one u per rounded operation -- a correctly rounded operation commits u / 2, so each count
carries a factor two, which also covers the u / 2 by which the stored truth is rounded:
    a rounded operation adds 1 to the count of its result; an exact one (negation, a power of two, ldexp, a select) adds 0
    product, quotient      the counts of the factors add (relative errors add)
    sum, difference        the largest count among the terms (each term's error is at most its count times its magnitude)
    fma(a, b, c)           max(count a + count b, count c) + 1
    device sqrt, exp       1 (at most one ulp);  IEEE 1 / x and a / b: 1;  fast_rcp: 2, what test_qdiv_within_two_ulp holds
"""
import os

import numpy as np

from tests import bessel_truth as bt

U = bt.U

# ---- the Bessel lifts ------------------------------------------------------------------------------------------------------------
# launcher -> (the plain routine whose E_HOST and device_margin bound the value error, the two members in the fixture)
BESSEL_JETS = {"dm_ke_pair_jets": ("ke_pair", ("ke0", "ke1")), "dm_ie_pair_from_k_jets": ("ie_pair_from_k", ("ie0", "ie1"))}
# c: the floating-point operations of the identity as es_jet.hpp / es_jet2.hpp write it, every one counted once whether it can
# round or not (an upper bound of what the counting rule of the module docstring gives), the larger of the two members:
#   first   A: vK - vK1 + (dn / x) * vK                        -, /, *, +              4
#           B: vK1 - vK - ((dn + 1.0) / x) * vK1               -, +, /, *, -           5
#   second  nx = n / x (1), n1x = (n + 1.0) / x (2), dK = A - B + nx * A (3), dK1 = B - A - n1x * B (3): 9 shared, then
#           A'': dK - dK1 + nx * dK - (nx / x) * A             -, *, +, /, *, -        6 -> 15
#           B'': dK1 - dK - n1x * dK1 + (n1x / x) * B          -, *, -, /, *, +        6 -> 15
#   lift and lift_onto then multiply by x.d = 1 and add x.h = 0: exact.  ie_pair_from_k has the same expressions.
BESSEL_JET_C = {1: 5, 2: 15}


def load():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jet_truth.npz"))
    return {k: z[k] for k in z.files}


def bessel_bound(routine, n, nu):
    """per row: E_HOST + device_margin + c, in u times the identity's magnitude"""
    return np.array([bt.E_HOST[routine][int(o)] + bt.device_margin(routine, int(o)) for o in n]) + BESSEL_JET_C[nu]


def bessel_errors(jets, launcher, got, nu):
    """(error in u x magnitude, error in u x |true|, magnitude / |true|) per row, the larger of the two members; got: the
    launcher's [rows, 10] output (Jet<1>: A.v, A.d, B.v, B.d; Jet2<1>: A.v, A.d, A.h, B.v, B.d, B.h)"""
    cols = (1, 3) if nu == 1 else (6, 9)
    by_mag, by_true, cond = [], [], []
    for col, f in zip(cols, BESSEL_JETS[launcher][1]):
        true, mag = jets[f"bj_{f}_d{nu}"], jets[f"bj_{f}_m{nu}"]
        diff = np.abs(got[:, col] - true)
        diff = np.where(np.isfinite(diff), diff, np.inf)           # a NaN result is an infinite error, not a skipped row
        by_mag.append(diff / (U * mag))
        by_true.append(diff / (U * np.abs(true)))
        cond.append(mag / np.abs(true))
    pick = np.argmax(np.stack(by_true), axis=0)
    rows = np.arange(got.shape[0])
    return np.max(np.stack(by_mag), axis=0), np.stack(by_true)[pick, rows], np.stack(cond)[pick, rows]


# ---- the operators -----------------------------------------------------------------------------------------------------------------
# code of dm_jet_op -> name in the fixture; 29 .. 32 have exact answers and no fixture
OPS = {0: "neg", 1: "add", 2: "sub", 3: "add_jd", 4: "add_dj", 5: "sub_jd", 6: "sub_dj", 7: "mul_jd", 8: "mul_dj",
       9: "mul_assign", 10: "mul", 11: "fma_jjj", 12: "fma_djj", 13: "fma_jjd", 14: "fma_djd", 15: "fma_jdj", 16: "fma_jdd",
       17: "rcp_from", 18: "rcp", 19: "fast_rcp", 20: "div", 21: "div_dj", 22: "div_jd", 23: "sqrt", 24: "exp", 25: "ldexp",
       26: "lift_onto", 27: "lift", 28: "fabs"}
OP_JET_FINITE, OP_VAL, OP_CONSTANT, OP_VARIABLE = 29, 30, 31, 32
N_OPS = 33

# c_op: the count of the rule above for the deepest component (a second derivative wherever there is one), from the
# expressions of es_jet.hpp and es_jet2.hpp; x_a: a first derivative, x_ab: a second one
C_OP = {
    "neg": 0, "fabs": 0, "ldexp": 0,              # exact: a sign, a select, a power of two
    "add": 1, "sub": 1,                           # one rounding per component
    "add_jd": 1, "add_dj": 1, "sub_jd": 1, "sub_dj": 1,          # the value; the derivatives pass through (exact)
    "mul_jd": 1, "mul_dj": 1, "mul_assign": 1, "div_jd": 1,      # one product / quotient per component
    "fma_djj": 1, "fma_jdj": 1, "fma_djd": 1, "fma_jdd": 1,      # one fma (or product) per component
    # cross = fma(x_a, y_b, x_b * y_a): 2; fma(x_ab, y.v, cross): 3; fma(x.v, y_ab, .): 4   (first order: 2)
    "mul": 4, "fma_jjd": 4,
    # cross + z_ab: 3, then the two fma: 5
    "fma_jjj": 5,
    # r: 1; d1 = -(r r): 3; d2 = -2 (d1 r): 5; x_a x_b: 1; d2 (x_a x_b): 7; fma(d1, x_ab, .): max(3, 7) + 1 = 8
    "rcp_from": 8, "rcp": 8,
    # the same with r at 2: d1 5, d2 8, d2 (x_a x_b) 10, fma 11
    "fast_rcp": 11,
    # q, r: 1; q_a = (x_a - q y_a) r: 2, 3, 3 + 1 + 1 = 5; cross(q, y) = fma(q_a, y_b, q_b y_a): max(5, 6) + 1 = 7;
    # fma(q.v, y_ab, cross): 8; x_ab - .: 9; times r: 9 + 1 + 1 = 11
    "div": 11,
    # q_a = -(q y_a) r: 2 + 1 + 1 = 4; cross: max(4, 5) + 1 = 6; fma(q.v, y_ab, cross): 7; times r: 9
    "div_dj": 9,
    # s: 1; r = 0.5 / s: 2; s_a = x_a r: 3; fma(-2 s_a, s_b, x_ab): 6 + 1 = 7; times r: 7 + 2 + 1 = 10
    "sqrt": 10,
    # e: 1; fma(x_a, x_b, x_ab): 1; e times it: 3   (first order: 2)
    "exp": 3,
    # x_a x_b: 1; d2f times it: 2; fma(df, x_ab, .): 3   (lift's first order df x_a: 1)
    "lift_onto": 3, "lift": 3,
}
assert set(C_OP) == set(OPS.values()) and max(C_OP.values()) <= 16


def op_operands(jets, code):
    """dict x, y, z ([rows, 6]), a, b, c ([rows]), e ([rows] int32) of an operator: the fixture's, ones (e: zero) for those the
    operator does not take"""
    name = OPS[code]
    rows = len(jets[f"op_{name}_t"])
    out = {}
    for key in ("x", "y", "z", "a", "b", "c", "e"):
        stored = jets.get(f"op_{name}_{key}")
        if stored is None:
            stored = np.zeros(rows, dtype=np.int32) if key == "e" else np.ones((rows, 6) if key in "xyz" else rows)
        assert len(stored) == rows
        out[key] = stored
    return out


def op_errors(jets, code, got, nv):
    """[rows, components] error in u x magnitude; got: the Jet2 rows [rows, 6]; nv = 1 takes the components (v, d[0], h[0])"""
    name = OPS[code]
    comp = [0, 1, 2, 3, 4, 5] if nv == 2 else [0, 1, 3]
    t, m, g = jets[f"op_{name}_t"][:, comp], jets[f"op_{name}_m"][:, comp], got[:, comp]
    diff = np.abs(g - t)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(diff == 0.0, 0.0, diff / (U * m))           # a magnitude of zero: only the exact zero passes
    return np.where(np.isfinite(err), err, np.inf)                 # a NaN result is an infinite error, not a skipped row
