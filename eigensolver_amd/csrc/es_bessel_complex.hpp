// fp64 modified Bessel functions of integer order at COMPLEX argument, for the exterior solution of the cylinder at complex
// frequency (es_cyl_complex.hip; include/eigensolver_amd.h section 14):  P_e(r) = a I_m(mu |r|) + b K_m(mu |r|) with
// mu = principal sqrt(m_e).  The caller guarantees Re m_e >= 0, so mu lies in the sector |arg z| <= pi/4: only that sector
// is supported (the continued fraction and the backward recurrence below need Re z > 0).
//
// Exponentially scaled forms, as in es_bessel.hpp:  Ke_n(z) = e^z K_n(z),  Ie_n(z) = e^-z I_n(z)  (the complex exponent: scipy's
// ive scales by e^-|Re z| instead).
//   * K_0, K_1:  |z| <= 2  the ascending series of esb::ke01 with the complex logarithm;
//                |z| >  2  Steed's continued fraction CF2 (Temme) at order 0 -- the Chebyshev series of the real routine does
//                          not continue off the real axis; its two coefficient sequences are real and come from the tables
//                          of es_bessel.hpp (qdiv_int, qdiv_cf2a);
//                then the upward recurrence K_{n+1} = K_{n-1} + (2n/z) K_n (K dominant for Re z > 0: stable).
//   * I_n, I_{n+1}: Miller's backward recurrence for the ratio and the Wronskian I_n K_{n+1} + I_{n+1} K_n = 1/z for the
//                normalisation (esb::ie_pair_from_k); |z| < 0.5: the ascending series.
// Accuracy against correctly rounded values (tests/golden/bessel_complex_truth.npz: mpmath at 40 digits; orders 0, 1, 2, 3, 5,
// 10, 11, 20, 40; arg z in {-pi/4, -pi/8, -1e-3, 0, 1e-9, pi/16, pi/8, 3pi/16, pi/4}; 36 radii log-spaced over [1e-6, 700],
// 0.5 and 2 with the doubles 1 and 4 ulp to either side, 1.98, 2.02, and 3e3, 3e4 apart), worst error relative to |f| in
// u = 2^-52 = 2.2e-16, host build (tests/test_hostmath_complex.py::test_truth_complex):
//   e^z K_n, K_{n+1}    |z| <= 700: 32 u (7.1e-15) at n = 0, z = 2 e^{-0.001 i}: at |z| = 2 the series of K_0 subtracts terms
//                       12 times the result; 24 u at n = 1, 14 ... 16 u at n = 2 ... 11, 22 u at n = 20, 42 u (9.2e-15) at
//                       n = 40 (the upward recurrence, |z| = 0.06);  |z| = 3e3, 3e4: 3.5 u
//   e^-z I_n, I_{n+1}   |z| <= 700: 14 ... 16 u for n <= 11 at |z| = 1.98 (it inherits the error of K), 21 u at n = 20, 38 u
//                       at n = 40 (|z| = 0.5, arg z = -pi/4);  |z| = 3e3, 3e4: 4.4 u (1350 u at n = 0, |z| = 3e4,
//                       arg z = -pi/4 while Miller's start index was sized by |z|: see cie_pair_from_k)
//   d/dz of either      (CJet of es_cjet.hpp) relative to (|f_n| + |f_{n+1}|)(1 + (n + 1)/|z|), the terms of the
//                       identities: 13 u at n = 0, 42 u at n = 40 for K; 2 u at n = 0, 35 u at n = 40 for I
// The device build (gfx950: __constant__ reciprocal tables, qdiv past index 64 of CF2, the device exp / log / hypot / atan2 /
// sin / cos) has its worst error per order within 1.1 u of these (14.7 u against 13.7 u at n = 10; equal at n = 0, 1, 40),
// with the same bits per row whether the order is wave-uniform or every lane runs its own order and branch
// (tests/test_devmath_gpu.py, which records the table).  The primitives cz_sqrt,
// cz_log, cz_exp and the two divisions are within 1.5 u of the modulus of the result on host and device, the sign on the
// cut of sqrt and log following the sign of the zero.  scipy.special.kve / ive is itself up to 1.9e-14 off (I at order 9,
// |z| = 0.004); the comparison with it stays as a second, independent reference.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <type_traits>
#include "es_bessel.hpp"

#if defined(__HIPCC__)
#define ES_HDM __host__ __device__
#else
#define ES_HDM
#endif

namespace esb {

// ---- the complex scalar: every operator the formula text of es_shoot_device.hpp asks of its scalar type ---------------------
// esb::cz is the library's only complex scalar and esb::CJet<ND> (es_cjet.hpp) its only complex jet: the slab, the cylinder,
// the Bessel routines and the field kernels all compute with these two, so a primitive is measured, and corrected, in one place.
struct cz {
  double re, im;
  cz() = default;
  ES_HDM explicit cz(double a) : re(a), im(0.0) {}
  ES_HDM cz(double a, double b) : re(a), im(b) {}
};
template <class T> struct is_cz { static constexpr bool value = false; };
template <> struct is_cz<cz> { static constexpr bool value = true; };

ES_HD cz operator-(cz a) { return cz(-a.re, -a.im); }
ES_HD cz operator+(cz a, cz b) { return cz(a.re + b.re, a.im + b.im); }
ES_HD cz operator-(cz a, cz b) { return cz(a.re - b.re, a.im - b.im); }
ES_HD cz operator+(cz a, double b) { return cz(a.re + b, a.im); }
ES_HD cz operator+(double a, cz b) { return cz(a + b.re, b.im); }
ES_HD cz operator-(cz a, double b) { return cz(a.re - b, a.im); }
ES_HD cz operator-(double a, cz b) { return cz(a - b.re, -b.im); }
ES_HD cz operator*(cz a, cz b) { return cz(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re); }
ES_HD cz operator*(cz a, double b) { return cz(a.re * b, a.im * b); }
ES_HD cz operator*(double a, cz b) { return cz(a * b.re, a * b.im); }
ES_HD cz& operator*=(cz& a, double b) { a = a * b; return a; }
ES_HD cz operator/(cz a, double b) { return cz(a.re / b, a.im / b); }
ES_HD cz operator/(cz a, cz b) {
  const double n = b.re * b.re + b.im * b.im;
  return cz((a.re * b.re + a.im * b.im) / n, (a.im * b.re - a.re * b.im) / n);
}
ES_HD cz operator/(double a, cz b) {
  const double n = b.re * b.re + b.im * b.im;
  return cz((a * b.re) / n, -(a * b.im) / n);
}
// a b + c_ with at least one complex operand: a product and a sum (no fused form of the complex product exists)
template <class A, class B, class C, class = typename std::enable_if<is_cz<A>::value || is_cz<B>::value || is_cz<C>::value>::type>
ES_HD cz fma(A a, B b, C c_) { return a * b + c_; }
ES_HD double val(cz a) { return a.re; }
ES_HD double cz_abs2(cz a) { return a.re * a.re + a.im * a.im; }
ES_HD double cz_abs(cz a) { return hypot(a.re, a.im); }
ES_HD bool cz_finite(cz a) { return isfinite(a.re) && isfinite(a.im); }
// principal square root (Re >= 0)
ES_HD cz cz_sqrt(cz z) {
  const double r = hypot(z.re, z.im);
  if (r == 0.0) return cz(0.0, 0.0);
  const double a = sqrt(0.5 * (r + fabs(z.re)));
  const double b = 0.5 * z.im / a;
  if (z.re >= 0.0) return cz(a, b);
  return cz(fabs(b), copysign(a, z.im));
}
ES_HD cz cz_exp(cz z) {
  const double e = exp(z.re);
  return cz(e * cos(z.im), e * sin(z.im));
}
// The same exponential with sine and cosine from one sincos call: the flow slab's (es_complex_shared.hpp, es_complex.hip).
// Two forms for the registers, not for the values: with cos and sin apart the slab kernels take up to 12 more vector registers
// and cx_refine_kernel spills; with sincos here and in the cylinder's exterior cylc_refine_kernel<FAM_CYLT> spills four vector
// registers, which it must not (tests/test_cyl_complex_codeobj.py).  On an MI355X the two gave the same bits in every output
// of tools/compare_complex_builds.py; only the es_complex_* entry points use this form, and no formula uses both.
ES_HD cz cz_exp_sincos(cz z) {
  const double e = exp(z.re);
  double s, c;
  sincos(z.im, &s, &c);
  return cz(e * c, e * s);
}
// principal logarithm
ES_HD cz cz_log(cz z) { return cz(log(hypot(z.re, z.im)), atan2(z.im, z.re)); }

// scaled K_0, K_1 (e^z K), |arg z| <= pi/4
ES_HD void cke01(cz z, cz& k0, cz& k1) {
  if (cz_abs2(z) <= 4.0) {
    // esb::ke01's series, term for term, in t = z^2 / 4
    const cz t = 0.25 * (z * z);
    const cz lg = cz_log(0.5 * z) + kEulerGamma;
    cz term0(1.0), i0(1.0), s0(0.0);
    cz term1(1.0), i1(1.0), s1(1.0);
    double hk = 0.0;
    for (int k = 1; k < 40; ++k) {
      const double rk = qdiv_int(1.0, k), rk1 = qdiv_int(1.0, k + 1);
      term0 = term0 * t * (rk * rk);
      hk += rk;
      i0 = i0 + term0;
      s0 = s0 + hk * term0;
      term1 = term1 * t * (rk * rk1);
      i1 = i1 + term1;
      s1 = s1 + (hk + hk + rk1) * term1;
      if (cz_abs2(term0) < 1e-36 * cz_abs2(i0)) break;
    }
    const cz ex = cz_exp(z);
    k0 = ex * (s0 - lg * i0);
    k1 = ex * (1.0 / z + lg * (0.5 * z) * i1 - 0.25 * (z * s1));
  } else {
    // CF2 at order 0 (Temme's sums beside Steed's continued fraction): a_i, c_i real, everything that carries z complex
    cz b = 2.0 * (1.0 + z), d = 1.0 / b, h = d, delh = d;
    cz q1(0.0), q2(1.0);
    const double a1 = 0.25;
    double c = a1, a = -a1;
    cz q(a1);
    cz s = 1.0 + q * delh;
    for (int i = 2; i < 500; ++i) {
      a -= 2.0 * (double)(i - 1);
      c = qdiv_int(-a * c, i);
      const cz qnew = (q1 - b * q2) * qdiv_cf2a(1.0, i, a);
      q1 = q2;
      q2 = qnew;
      q = q + c * qnew;
      b = b + 2.0;
      d = 1.0 / (b + a * d);
      delh = (b * d - 1.0) * delh;
      h = h + delh;
      const cz dels = q * delh;
      s = s + dels;
      if (!(cz_abs2(dels) >= 1e-34 * cz_abs2(s))) break;     // converged, or not a number
    }
    h = a1 * h;
    k0 = cz_sqrt((0.5 * kPi) / z) / s;
    k1 = (k0 * (z + 0.5 - h)) / z;
  }
}

// scaled K_n, K_{n+1} for integer n >= 0
ES_HD void cke_pair(int n, cz z, cz& kn, cz& knp1) {
  cz a, b;
  cke01(z, a, b);
  const cz toz = 2.0 / z;
  for (int j = 1; j <= n; ++j) {      // (a, b) = (K_{j-1}, K_j) -> (K_j, K_{j+1})
    const cz c = a + ((double)j * toz) * b;
    a = b;
    b = c;
  }
  kn = a;
  knp1 = b;
}

// scaled I_n, I_{n+1} by the ascending series (small |z|: all terms of one phase, no cancellation)
ES_HD void cie_pair(int n, cz z, cz& in_, cz& inp1) {
  const cz t = 0.25 * (z * z);
  const cz hz = 0.5 * z;
  cz pre(1.0);
  for (int j = 1; j <= n; ++j) pre = pre * (hz / (double)j);
  cz term_a(1.0), sum_a(1.0), term_b(1.0), sum_b(1.0);
  for (int k = 1; k < 400; ++k) {
    const double kk = (double)k;
    term_a = (term_a * t) / (kk * (kk + (double)n));
    term_b = (term_b * t) / (kk * (kk + (double)n + 1.0));
    sum_a = sum_a + term_a;
    sum_b = sum_b + term_b;
    if (!(cz_abs2(term_a) >= 1e-36 * cz_abs2(sum_a))) break;
  }
  const cz ex = cz_exp(-z);
  in_ = ex * pre * sum_a;
  inp1 = ex * pre * (hz / ((double)n + 1.0)) * sum_b;
}

// scaled I_n, I_{n+1} from the scaled K_n, K_{n+1} at the same argument: Miller's backward recurrence for the ratio
// I_{n+1} / I_n (I is the minimal solution for Re z > 0), the Wronskian for the normalisation.  The start index follows
// esb::ie_pair_from_k with |z|^2 / Re z for x: the error of the arbitrary start decays like exp(-M^2 Re z / |z|^2), so this,
// not |z|, is what M^2 = 40 x has to cover.  It is |z| on the real axis, bit for bit (hypot(x, 0) = x and x / x = 1: M as
// before), and at most sqrt 2 |z| in the sector.  Sized by |z| alone the decay at arg z = +-pi/4 was exp(-28), and
// the additive terms of M stop helping as |z| grows: at |z| = 3e4, arg z = -pi/4 the host build was 1350 u off at n = 0,
// 801 u at n = 10, 169 u at n = 40 (u = 2^-52, against mpmath), and the z-derivative 9.8 u at |z| = 391; now 4.4 u at
// worst on |z| = 3e3 and 3e4, every order and angle, as for |z| <= 700, and the derivative 2.1 u.  The quantity is capped so
// that an argument the caller never meant (an iterate that ran away, Re z <= 0 or not a number) costs a bounded number of
// steps.
ES_HD void cie_pair_from_k(int n, cz z, cz kn, cz knp1, cz& in_, cz& inp1) {
  const double az = cz_abs(z);
  if (az < 0.5) { cie_pair(n, z, in_, inp1); return; }
  const int M = n + 10 + (int)sqrt(40.0 * fmin(az * fabs(az / z.re), 1.0e6));
  const cz toz = 2.0 / z;
  cz ip(0.0), ic(1.0);                                        // I_{M+1}, I_M up to a common factor, kept within range
  for (int k = M; k > n; --k) {                               // (ip, ic) = (I_{k+1}, I_k) -> (I_k, I_{k-1})
    const cz im = ((double)k * toz) * ic + ip;
    ip = ic;
    ic = im;
    if (cz_abs2(ic) > 1e200) { ic = 1e-100 * ic; ip = 1e-100 * ip; }
  }
  const cz f = ip / ic;                                       // I_{n+1} / I_n
  in_ = 1.0 / (z * (f * kn + knp1));
  inp1 = f * in_;
}

}  // namespace esb
