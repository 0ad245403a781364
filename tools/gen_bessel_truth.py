"""Correctly rounded Bessel values for the tests of eigensolver_amd/csrc/es_bessel.hpp, es_bessel_complex.hpp and es_cjet.hpp.

    python tools/gen_bessel_truth.py            # writes tests/golden/bessel_truth.npz and bessel_complex_truth.npz
    python tools/gen_bessel_truth.py real       # one of them: real | complex

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
"""
import os
import sys

import mpmath as mp
import numpy as np

ORDERS = (0, 1, 2, 3, 5, 10, 11, 20, 40)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
OUT = os.path.join(GOLDEN, "bessel_truth.npz")
OUT_COMPLEX = os.path.join(GOLDEN, "bessel_complex_truth.npz")
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


def main(which):
    if which in ("all", "real"):
        real_fixture()
    if which in ("all", "complex"):
        complex_fixture()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "all")
