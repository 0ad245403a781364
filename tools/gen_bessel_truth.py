"""Correctly rounded Bessel values for the tests of eigensolver_amd/csrc/es_bessel.hpp, es_bessel_complex.hpp and es_cjet.hpp,
and correctly rounded results of every operator of the real jets es_jet.hpp and es_jet2.hpp.

    python tools/gen_bessel_truth.py            # writes tests/golden/bessel_truth.npz, bessel_complex_truth.npz, jet_truth.npz
    python tools/gen_bessel_truth.py real       # one of them: real | complex | jets (jets reads bessel_truth.npz)

mpmath at 40 significant digits, every value rounded once to the nearest double (complex values: real and imaginary part
separately) -- a reference that is exact to half an ulp, where scipy.special (tests/test_hostmath.py,
tests/test_hostmath_complex.py) is itself a few ulp off.

bessel_truth.npz, real argument, two point sets:

  ik_n, ik_x     orders {0, 1, 2, 3, 5, 10, 11, 20, 40} x arguments log-spaced over [1e-6, 700], plus 0.5 and 2.0 (the
                 branch points of ie_pair_from_k and ke01) with both neighbouring doubles
  ik_ke0/ke1     e^x K_n(x), e^x K_{n+1}(x)
  ik_ie0/ie1     e^-x I_n(x), e^-x I_{n+1}(x)      (the ascending series ie_pair is meant for x <= 60: the tests select)
  jy_n, jy_x     the same orders x arguments log-spaced over [1e-5, 80], plus the doubles next to the first three zeros of
                 J_n and of Y_n (the nearest double and 4 ulp to either side)
  jy_j0/j1/y0/y1 J_n, J_{n+1}, Y_n, Y_{n+1}

Rows with a value outside [1e-290, 1e290] are left out (order 40 at the smallest arguments: I_41 is subnormal there and
a relative error says nothing).  The tests read the file only; mpmath is needed to regenerate it, not to run them.

bessel_complex_truth.npz, complex argument (complex128 arrays; the arguments are the doubles themselves):

  c_n, c_z       the same orders x nine angles {-pi/4, -pi/8, -1e-3, 0, 1e-9, pi/16, pi/8, 3pi/16, pi/4} (c_angle: the index)
                 x radii: 36 log-spaced over [1e-6, 700]; 0.5 and 2.0 with the doubles 1 and 4 ulp to either side (the branch
                 points of cie_pair_from_k, on hypot(re, im) < 0.5, and of cke01, on re^2 + im^2 <= 4 as doubles: both sides
                 of either occur on every angle, checked here); 1.98, 2.02; 3e3 and 3e4 (c_far: |z| > 700, which the tests
                 treat apart).  z = (r cos a, r sin a) in doubles; at +-pi/4, |Im z| is the double below Re z, so that
                 Re z^2 >= 0: the sector the header supports
  c_ke0/ke1      e^z K_n(z), e^z K_{n+1}(z)
  c_ie0/ie1      e^-z I_n(z), e^-z I_{n+1}(z)
  c_dke0/dke1, c_die0/die1
                 their derivatives in z by the identities of es_cjet.hpp (cke_pair, cie_pair_from_k), summed at 40 digits
                 Rows with any |value| outside [1e-290, 1e290] are left out, as above.
  sqrt_z/_w, log_z/_w
                 arguments and principal values of cz_sqrt, cz_log: 320 arguments log-uniform in modulus over [1e-100, 1e100]
                 at random angles (all four quadrants), and the four half axes, ten moduli each, with the vanishing part +0
                 and -0 -- on the negative real axis, the cut of both, the sign of the result's imaginary part follows the
                 sign of the zero, as C99's csqrt and clog have it; sqrt also at z = 0
  exp_z/_w       cz_exp: as above with the modulus in [1e-100, 700], three quarters of them in [1e-2, 700]
  div_a/_b/_w    cz / cz: w = a / b, both from the argument set above;  rdiv_a/_b/_w: double / cz
                 The moduli of divisors stay inside [1e-150, 1e150]: operator/ forms |b|^2 and is not meant beyond that, so
                 nothing outside is in the fixture or tested.

jet_truth.npz, the real jets (tests/jet_truth.py reads it):

  bj_<f>_d1/_d2  for f in ke0, ke1, ie0, ie1 and every ik row of bessel_truth.npz: the first and second derivative in x of
                 e^x K_n, e^x K_{n+1}, e^-x I_n, e^-x I_{n+1} by the identities of es_jet.hpp and es_jet2.hpp, summed at 40
                 digits.  On 240 rows spread over every order and decade of x this script compares them with mpmath.diff of
                 the function itself and fails above 1e-30 relative: neither the fixture nor the header's comment can carry
                 a wrong identity.
  bj_<f>_m1/_m2  the identity's magnitude: the sum of the absolute values of its terms, the first derivatives inside the
                 second identity expanded into their own terms -- the scale the rounding errors of the identity live on
  op_codes, op_names
                 the operators with a fixture, by the code of dm_jet_op (tests/devmath/devmath_probe.hip)
  op_<name>_x/_y/_z, _a/_b/_c, _e
                 66 operand rows per operator (1914 in all, and the two zeros of fabs): the Jet2<2> operands as rows
                 (v, d[0], d[1], h[0], h[1], h[2]), the double and int operands; only the operands the operator takes are
                 stored.  Every component is log-uniform in magnitude over [2^-40, 2^40] with both signs (the range DESIGN.md
                 documents for the march); a tenth of the rows of each operand are constants (d = h = 0), a tenth variables
                 (unit d, h = 0), at different rows for x, y and z.  sqrt: positive values; exp: values uniform in [-60, 60];
                 rcp_from: a is the IEEE quotient 1 / v; ldexp: e in [-20, 20]; fabs: both signs and the rows +0.0, -0.0,
                 to which the header's rule gives the sign +1 (the derivatives pass unchanged)
  op_<name>_t    the six true components, from arithmetic of bivariate Taylor polynomials of total degree <= 2 at 40 digits
                 (multiply and truncate; reciprocal, square root and exponential from their series about the value): a route
                 that does not restate the header's product and chain rules.  A Jet2<1> result is the components
                 (v, d[0], h[0]) of the same row
  op_<name>_m    the magnitude of each component: the header's expression with every sum the sum of the magnitudes and every
                 product the product of the magnitudes
"""
import os
import sys

import mpmath as mp
import numpy as np

ORDERS = (0, 1, 2, 3, 5, 10, 11, 20, 40)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
OUT = os.path.join(GOLDEN, "bessel_truth.npz")
OUT_COMPLEX = os.path.join(GOLDEN, "bessel_complex_truth.npz")
OUT_JETS = os.path.join(GOLDEN, "jet_truth.npz")
LO, HI = 1e-290, 1e290
ANGLES = (-np.pi / 4, -np.pi / 8, -1e-3, 0.0, 1e-9, np.pi / 16, np.pi / 8, 3 * np.pi / 16, np.pi / 4)
FAR = 700.0


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


def real_fixture():
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


# ---- complex argument ----------------------------------------------------------------------------------------------------------
def complex_radii():
    rs = list(np.logspace(-6, np.log10(FAR), 36))
    for b in (0.5, 2.0):
        u = np.spacing(b)                              # the spacing above b; below it is u / 2
        rs += [b - 2 * u, b - u / 2, b, b + u, b + 4 * u]
    rs += [1.98, 2.02, 3e3, 3e4]
    return np.array(sorted(set(float(r) for r in rs)))


def complex_argument(r, a):
    re, im = float(r * np.cos(a)), float(r * np.sin(a))
    if abs(a) == np.pi / 4:
        im = float(np.copysign(np.nextafter(re, 0.0), a))
    return complex(re, im)


def _mpc(z):
    return mp.mpc(mp.mpf(z.real), mp.mpf(z.imag))


def _c(w):
    return complex(float(w.real), float(w.imag))


def complex_bessel_rows():
    keys = ("n", "angle", "z", "ke0", "ke1", "ie0", "ie1", "dke0", "dke1", "die0", "die1")
    rows = {k: [] for k in keys}
    radii = complex_radii()
    for ia, a in enumerate(ANGLES):
        zs = [complex_argument(r, a) for r in radii]
        abs2 = np.array([z.real * z.real + z.imag * z.imag for z in zs])      # as cz_abs2 forms it
        hyp = np.array([np.hypot(z.real, z.imag) for z in zs])
        near2, near05 = np.abs(radii - 2.0) < 1e-9, np.abs(radii - 0.5) < 1e-9
        assert (abs2[near2] <= 4.0).any() and (abs2[near2] > 4.0).any(), a
        assert (hyp[near05] < 0.5).any() and (hyp[near05] >= 0.5).any(), a
        for n in ORDERS:
            for z in zs:
                Z = _mpc(z)
                ez = mp.exp(Z)
                k0, k1 = ez * mp.besselk(n, Z), ez * mp.besselk(n + 1, Z)
                i0, i1 = mp.besseli(n, Z) / ez, mp.besseli(n + 1, Z) / ez
                v = [k0, k1, i0, i1,
                     k0 - k1 + (n / Z) * k0, k1 - k0 - ((n + 1) / Z) * k1,
                     i1 - i0 + (n / Z) * i0, i0 - i1 - ((n + 1) / Z) * i1]
                v = [_c(t) for t in v]
                if all(LO < abs(t) < HI for t in v):
                    for key, t in zip(keys, [n, ia, z] + v):
                        rows[key].append(t)
    out = {}
    for key, vals in rows.items():
        dtype = np.int32 if key == "n" else np.int8 if key == "angle" else np.complex128
        out["c_" + key] = np.asarray(vals, dtype=dtype)
    out["c_far"] = np.abs(out["c_z"]) > FAR
    return out


def primitive_arguments(rng, lo_exp, hi):
    """320 arguments of random angle and 80 on the half axes with both signs of the vanishing part; moduli log-uniform in
    [10^lo_exp, hi]"""
    def moduli(count):
        return 10.0 ** rng.uniform(lo_exp, np.log10(hi), count)
    r, a = moduli(320), rng.uniform(-np.pi, np.pi, 320)
    zs = [complex(x, y) for x, y in zip(r * np.cos(a), r * np.sin(a))]
    for sign in (1.0, -1.0):
        for zero in (0.0, -0.0):
            zs += [complex(sign * m, zero) for m in moduli(10)]          # the real axis, from above and from below
            zs += [complex(zero, sign * m) for m in moduli(10)]          # the imaginary axis, from the right and the left
    return np.asarray(zs, dtype=np.complex128)


def _signed(f, z):
    """f at the double z, for f with f(conj z) = conj f(z): mpmath knows no signed zero, so the lower side of a cut is the
    conjugate of the upper side"""
    if np.signbit(z.imag):
        w = _c(f(_mpc(z.conjugate())))
        return complex(w.real, -w.imag)
    return _c(f(_mpc(z)))


def complex_primitive_rows():
    rng = np.random.default_rng(20250114)
    z = primitive_arguments(rng, -100.0, 1e100)
    out = {}
    out["sqrt_z"] = np.concatenate([z, np.asarray([0j])])
    out["sqrt_w"] = np.asarray([_signed(mp.sqrt, t) for t in z] + [0j])
    out["log_z"] = z
    out["log_w"] = np.asarray([_signed(mp.log, t) for t in z])
    ze = np.concatenate([primitive_arguments(rng, -100.0, 700.0)[::4], primitive_arguments(rng, -2.0, 700.0)[100:]])
    assert len(ze) == 400 and np.abs(ze).max() <= 700.0
    out["exp_z"] = ze
    out["exp_w"] = np.asarray([_signed(mp.exp, t) for t in ze])
    a = z[rng.permutation(len(z))]
    out["div_a"], out["div_b"] = a, z
    out["div_w"] = np.asarray([_c(_mpc(s) / _mpc(t)) for s, t in zip(a, z)])
    ra = 10.0 ** rng.uniform(-100.0, 100.0, len(z)) * rng.choice([-1.0, 1.0], len(z))
    out["rdiv_a"], out["rdiv_b"] = ra, z
    out["rdiv_w"] = np.asarray([_c(mp.mpf(float(s)) / _mpc(t)) for s, t in zip(ra, z)])
    assert 1e-150 <= np.abs(z).min() and np.abs(z).max() <= 1e150
    return out


def complex_fixture():
    mp.mp.dps = 40
    arrays = complex_bessel_rows()
    arrays.update(complex_primitive_rows())
    np.savez_compressed(OUT_COMPLEX, **arrays)
    print(OUT_COMPLEX, {k: v.shape for k, v in arrays.items()}, os.path.getsize(OUT_COMPLEX), "bytes")


# ---- the real jets: es_jet.hpp, es_jet2.hpp ---------------------------------------------------------------------------------------
BESSEL_JET_FUNCS = ("ke0", "ke1", "ie0", "ie1")
DIFF_CHECK_ROWS = 240                          # rows on which the identities are held to mpmath.diff of the function
OP_ROWS = 66                                   # operand rows per operator: 29 operators, 1914 rows (and the two zeros of fabs)
# operator code (tests/devmath/devmath_probe.hip, dm_jet_op) -> (name, jet operands, scalar operands); the codes 29 .. 32
# (jet_finite, val, the constant, the variable) have exact answers and need no fixture
JET_OPS = {0: ("neg", "x", ""), 1: ("add", "xy", ""), 2: ("sub", "xy", ""), 3: ("add_jd", "x", "a"), 4: ("add_dj", "x", "a"),
           5: ("sub_jd", "x", "a"), 6: ("sub_dj", "x", "a"), 7: ("mul_jd", "x", "a"), 8: ("mul_dj", "x", "a"),
           9: ("mul_assign", "x", "a"), 10: ("mul", "xy", ""), 11: ("fma_jjj", "xyz", ""), 12: ("fma_djj", "xy", "a"),
           13: ("fma_jjd", "xy", "a"), 14: ("fma_djd", "x", "ab"), 15: ("fma_jdj", "xy", "a"), 16: ("fma_jdd", "x", "ab"),
           17: ("rcp_from", "x", "a"), 18: ("rcp", "x", ""), 19: ("fast_rcp", "x", ""), 20: ("div", "xy", ""),
           21: ("div_dj", "x", "a"), 22: ("div_jd", "x", "a"), 23: ("sqrt", "x", ""), 24: ("exp", "x", ""),
           25: ("ldexp", "x", "e"), 26: ("lift_onto", "xy", "ab"), 27: ("lift", "x", "abc"), 28: ("fabs", "x", "")}
MONOMIALS = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))       # of a row (v, d[0], d[1], h[0], h[1], h[2])
FACTORIAL = (1, 1, 1, 2, 1, 2)                                     # derivative = FACTORIAL x Taylor coefficient


def bessel_jet_rows():
    """d/dx and d2/dx2 of the four scaled functions on the ik rows of bessel_truth.npz by the identities of es_jet.hpp and
    es_jet2.hpp summed at 40 digits, with the sum of the magnitudes of their terms (first derivatives inside the second
    identity expanded); on DIFF_CHECK_ROWS rows spread over every order and decade the identities are held to mpmath.diff."""
    truth = np.load(OUT)
    ns, xs = truth["ik_n"], truth["ik_x"]
    out = {f"bj_{f}_{q}": np.empty(len(xs)) for f in BESSEL_JET_FUNCS for q in ("d1", "d2", "m1", "m2")}
    check = set(np.round(np.linspace(0, len(xs) - 1, DIFF_CHECK_ROWS)).astype(int).tolist())
    assert len(check) >= 200
    covered = set()
    worst = mp.mpf(0)
    for i, (n, x) in enumerate(zip(ns.tolist(), xs.tolist())):
        X = mp.mpf(x)
        ex = mp.exp(X)
        kA, kB = ex * mp.besselk(n, X), ex * mp.besselk(n + 1, X)
        iA, iB = mp.besseli(n, X) / ex, mp.besseli(n + 1, X) / ex
        nx, n1x = n / X, (n + 1) / X
        # (d1, d2, m1, m2) per function; s: the sign of the pair's own terms, K: A' = A - B + ..., I: A' = B - A + ...
        for (fa, fb), (A, B), s in ((("ke0", "ke1"), (kA, kB), 1), (("ie0", "ie1"), (iA, iB), -1)):
            dA, dB = s * (A - B) + nx * A, s * (B - A) - n1x * B
            mA, mB = abs(A) + abs(B) + nx * abs(A), abs(B) + abs(A) + n1x * abs(B)
            ddA = s * (dA - dB) + nx * dA - (nx / X) * A
            ddB = s * (dB - dA) - n1x * dB + (n1x / X) * B
            mmA = mA + mB + nx * mA + (nx / X) * abs(A)
            mmB = mB + mA + n1x * mB + (n1x / X) * abs(B)
            for f, vals in ((fa, (dA, ddA, mA, mmA)), (fb, (dB, ddB, mB, mmB))):
                for q, v in zip(("d1", "d2", "m1", "m2"), vals):
                    out[f"bj_{f}_{q}"][i] = float(v)
            if i in check:
                covered.add((n, int(np.floor(np.log10(x)))))
                sgn = 1 if s == 1 else -1
                for order, (d1, d2) in ((n, (dA, ddA)), (n + 1, (dB, ddB))):
                    def f(t, order=order, sgn=sgn):
                        return mp.exp(sgn * t) * (mp.besselk(order, t) if sgn == 1 else mp.besseli(order, t))
                    for nu, have in ((1, d1), (2, d2)):
                        want = mp.diff(f, X, nu)
                        rel = abs(have - want) / abs(want)
                        worst = max(worst, rel)
                        assert rel <= mp.mpf("1e-30"), (n, x, order, nu, have, want)
    decades = set(int(np.floor(np.log10(x))) for x in xs)
    assert set(n for n, _ in covered) == set(ORDERS) and set(d for _, d in covered) == decades, covered
    print(f"identities against mpmath.diff on {len(check)} rows: worst {float(worst):.1e} relative")
    return out


class Poly(dict):
    """A bivariate Taylor polynomial of total degree <= 2 about the operands' point: {(i, j): coefficient of dw^i dk^j}"""

    @staticmethod
    def of_row(row):
        return Poly({m: mp.mpf(float(c)) / f for m, c, f in zip(MONOMIALS, row, FACTORIAL)})

    @staticmethod
    def const(c):
        return Poly({m: (mp.mpf(float(c)) if m == (0, 0) else mp.mpf(0)) for m in MONOMIALS})

    def row(self):
        return [self[m] * f for m, f in zip(MONOMIALS, FACTORIAL)]

    def __add__(self, o):
        return Poly({m: self[m] + o[m] for m in MONOMIALS})

    def __neg__(self):
        return Poly({m: -self[m] for m in MONOMIALS})

    def __sub__(self, o):
        return self + (-o)

    def __mul__(self, o):                                          # multiply and truncate
        if not isinstance(o, Poly):
            return Poly({m: self[m] * o for m in MONOMIALS})
        r = {m: mp.mpf(0) for m in MONOMIALS}
        for (a, b), s in self.items():
            for (c, d), t in o.items():
                if a + b + c + d <= 2:
                    r[(a + c, b + d)] += s * t
        return Poly(r)

    def tail(self):
        """(the constant term, the polynomial without it)"""
        t = Poly(self)
        t[(0, 0)] = mp.mpf(0)
        return self[(0, 0)], t

    def series(self, c0, c1, c2):
        """c0 + c1 t + c2 t^2 in t = this polynomial's part without the constant term (t^3 is of degree 3: truncated)"""
        _, t = self.tail()
        r = t * c1 + (t * t) * c2
        r[(0, 0)] = mp.mpf(c0)
        return r

    def reciprocal(self):                                          # 1 / (v + t) = 1/v - t / v^2 + t^2 / v^3
        v = self[(0, 0)]
        return self.series(1 / v, -1 / v ** 2, 1 / v ** 3)

    def sqrt(self):                                                # sqrt(v + t) = s + t / (2 s) - t^2 / (8 s^3)
        s = mp.sqrt(self[(0, 0)])
        return self.series(s, 1 / (2 * s), -1 / (8 * s ** 3))

    def exp(self):                                                 # e^(v + t) = e^v (1 + t + t^2 / 2)
        e = mp.exp(self[(0, 0)])
        return self.series(e, e, e / 2)


def op_truth(code, x, y, z, a, b, c, e):
    """the six true components of operator `code`: Taylor arithmetic, not the header's product and chain rules"""
    X, Y, Z = Poly.of_row(x), Poly.of_row(y), Poly.of_row(z)
    A, B, C = Poly.const(a), Poly.const(b), Poly.const(c)
    r = {0: lambda: -X, 1: lambda: X + Y, 2: lambda: X - Y, 3: lambda: X + A, 4: lambda: A + X, 5: lambda: X - A,
         6: lambda: A - X, 7: lambda: X * A, 8: lambda: A * X, 9: lambda: X * A, 10: lambda: X * Y, 11: lambda: X * Y + Z,
         12: lambda: A * X + Y, 13: lambda: X * Y + A, 14: lambda: A * X + B, 15: lambda: X * A + Y, 16: lambda: X * A + B,
         17: lambda: X.reciprocal(), 18: lambda: X.reciprocal(), 19: lambda: X.reciprocal(), 20: lambda: X * Y.reciprocal(),
         21: lambda: A * X.reciprocal(), 22: lambda: X * A.reciprocal(), 23: lambda: X.sqrt(), 24: lambda: X.exp(),
         25: lambda: X * mp.ldexp(mp.mpf(1), int(e)),
         # f(x) for f given by f(v) = a (lift) resp. y's value, f'(v) = first scalar, f''(v) = second scalar
         26: lambda: X.series(mp.mpf(0), mp.mpf(float(a)), mp.mpf(float(b)) / 2),
         27: lambda: X.series(mp.mpf(float(a)), mp.mpf(float(b)), mp.mpf(float(c)) / 2),
         28: lambda: -X if float(x[0]) < 0.0 else X}[code]().row()
    if code == 26:                                                 # lift_onto takes value and first-order part as given
        r[:3] = [mp.mpf(float(t)) for t in y[:3]]
    return r


def op_magnitude(code, x, y, z, a, b, c, e):
    """the header's expression for each component with every sum the sum of the magnitudes and every product the product
    of the magnitudes: the companion of a running error bound (this does restate the header, for the scale alone)"""
    value = mp.mpf(float(x[0]))                                    # signed: exp is not even
    x, y, z = ([abs(mp.mpf(float(t))) for t in row] for row in (x, y, z))
    a, b, c = (abs(mp.mpf(float(t))) for t in (a, b, c))
    PAIR = ((1, 1), (1, 2), (2, 2))                                # h[p] is the pair (d[a], d[b]) of row indices

    def cross(s, t, p):
        i, j = PAIR[p]
        return s[i] * t[j] + s[j] * t[i]

    def product(s, t):
        return [s[0] * t[0], s[0] * t[1] + s[1] * t[0], s[0] * t[2] + s[2] * t[0]] + \
               [s[0] * t[3 + p] + s[3 + p] * t[0] + cross(s, t, p) for p in range(3)]

    def plus(s, t):
        return [u + v for u, v in zip(s, t)]

    def scaled(s, f):
        return [u * f for u in s]

    def with_value(s, v):
        return [s[0] + v] + s[1:]

    def chain(v, d1, d2, s):                                       # f(s): value v, d1 s_c, d1 s_ab + d2 s_a s_b
        return [v, d1 * s[1], d1 * s[2]] + [d1 * s[3 + p] + d2 * s[PAIR[p][0]] * s[PAIR[p][1]] for p in range(3)]

    def quotient(num, den, num_is_jet):
        q, r = (num[0] if num_is_jet else num) / den[0], 1 / den[0]
        first = [((num[i] if num_is_jet else 0) + q * den[i]) * r for i in (1, 2)]
        qj = [q] + first
        second = [((num[3 + p] if num_is_jet else 0) + q * den[3 + p] + cross(qj, den, p)) * r for p in range(3)]
        return qj + second

    if code == 0 or code == 28:
        return x
    if code in (1, 2):
        return plus(x, y)
    if code in (3, 4, 5, 6):
        return with_value(x, a)
    if code in (7, 8, 9):
        return scaled(x, a)
    if code == 10:
        return product(x, y)
    if code == 11:
        return plus(product(x, y), z)
    if code in (12, 15):
        return plus(scaled(x, a), y)
    if code == 13:
        return with_value(product(x, y), a)
    if code in (14, 16):
        return with_value(scaled(x, a), b)
    if code in (17, 18, 19):
        r = 1 / x[0]
        return chain(r, r * r, 2 * r ** 3, x)
    if code == 20:
        return quotient(x, y, True)
    if code == 21:
        return quotient(a, x, False)
    if code == 22:
        return scaled(x, 1 / a)
    if code == 23:
        s = mp.sqrt(x[0])
        r = mp.mpf("0.5") / s
        sd = [s, x[1] * r, x[2] * r]
        return sd + [(2 * sd[PAIR[p][0]] * sd[PAIR[p][1]] + x[3 + p]) * r for p in range(3)]
    if code == 24:
        ev = mp.exp(value)
        return [ev, ev * x[1], ev * x[2]] + [ev * (x[PAIR[p][0]] * x[PAIR[p][1]] + x[3 + p]) for p in range(3)]
    if code == 25:
        return scaled(x, mp.ldexp(mp.mpf(1), int(e)))
    if code == 26:
        return y[:3] + chain(0, a, b, x)[3:]
    if code == 27:
        return chain(a, b, c, x)
    raise ValueError(code)


def jet_operands(rng, rows, shift):
    """rows x 6 operand rows: every component log-uniform in magnitude over [2^-40, 2^40], both signs; row i is a constant
    where (i + shift) % 10 == 0 (every d and h zero) and a variable where (i + shift) % 10 == 1 (unit d, zero h)"""
    v = np.exp2(rng.uniform(-40.0, 40.0, (rows, 6))) * rng.choice([-1.0, 1.0], (rows, 6))
    kind = (np.arange(rows) + shift) % 10
    v[kind <= 1, 1:] = 0.0
    variable = np.where(kind == 1)[0]
    v[variable, 1 + (variable // 10) % 2] = 1.0
    return v


def jet_operator_rows():
    rng = np.random.default_rng(20250611)
    out = {"op_codes": np.array(sorted(JET_OPS), dtype=np.int32), "op_names": np.array([JET_OPS[c][0] for c in sorted(JET_OPS)])}
    total = 0
    for code in sorted(JET_OPS):
        name, jets, scalars = JET_OPS[code]
        x, y, z = (jet_operands(rng, OP_ROWS, s) for s in (0, 3, 6))
        a, b, c = (np.exp2(rng.uniform(-40.0, 40.0, OP_ROWS)) * rng.choice([-1.0, 1.0], OP_ROWS) for _ in range(3))
        e = rng.integers(-20, 21, OP_ROWS).astype(np.int32)
        if name == "sqrt":
            x[:, 0] = np.abs(x[:, 0])
        if name == "exp":
            x[:, 0] = rng.uniform(-60.0, 60.0, OP_ROWS)
        if name == "rcp_from":
            a = 1.0 / x[:, 0]                                      # the IEEE quotient: the correctly rounded reciprocal
        if name == "fabs":                                         # both zeros: the header's rule gives sign +1 to both
            assert (x[:, 0] < 0).sum() >= 10 and (x[:, 0] > 0).sum() >= 10
            x = np.concatenate([x, x[2:4]])
            x[-2, 0], x[-1, 0] = 0.0, -0.0
            y, z = (np.concatenate([t, t[2:4]]) for t in (y, z))
            a, b, c, e = (np.concatenate([t, t[2:4]]) for t in (a, b, c, e))
        rows = len(x)
        t, m = np.empty((rows, 6)), np.empty((rows, 6))
        for i in range(rows):
            t[i] = [float(u) for u in op_truth(code, x[i], y[i], z[i], a[i], b[i], c[i], e[i])]
            m[i] = [float(u) for u in op_magnitude(code, x[i], y[i], z[i], a[i], b[i], c[i], e[i])]
        assert np.all(m >= np.abs(t) * (1.0 - 1e-15)), name          # a sum of magnitudes is no smaller than the sum
        stored = dict(t=t, m=m, **{k: v for k, v in (("x", x), ("y", y), ("z", z)) if k in jets},
                      **{k: v for k, v in (("a", a), ("b", b), ("c", c), ("e", e)) if k in scalars})
        for key, arr in stored.items():
            assert len(arr) == rows and np.all(np.isfinite(arr)), (name, key)      # nothing dropped, every number finite
            out[f"op_{name}_{key}"] = arr
        total += rows
    assert total == OP_ROWS * len(JET_OPS) + 2
    return out


def jets_fixture():
    mp.mp.dps = 40
    arrays = bessel_jet_rows()
    arrays.update(jet_operator_rows())
    for key, arr in arrays.items():
        assert arr.dtype.kind in "US" or np.all(np.isfinite(arr)), key
    np.savez_compressed(OUT_JETS, **arrays)
    size = os.path.getsize(OUT_JETS)
    print(OUT_JETS, {k: v.shape for k, v in arrays.items()}, size, "bytes")
    assert size < 500_000, size


def main(which):
    if which in ("all", "real"):
        real_fixture()
    if which in ("all", "complex"):
        complex_fixture()
    if which in ("all", "jets"):
        jets_fixture()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "all")
