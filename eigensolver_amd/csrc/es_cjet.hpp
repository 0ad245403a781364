// Forward-mode jets of the complex-frequency paths: the cylinder (include/eigensolver_amd.h sections 15 and 18) and the flow
// slab (section 12).  esb::cz (es_bessel_complex.hpp) and esb::CJet are the library's only complex scalar and complex jet.
//   CJet<ND>   an esb::cz value with ND esb::cz derivative components, and the operators and overloads the FAM_CYL0 formula
//              text of es_shoot_device.hpp, the exterior of es_cyl_complex_shared.hpp and the slab's text of
//              es_complex_shared.hpp need of their scalar type (fma, rcp, sqrt, exp, val, lift, cke_pair, cie_pair_from_k,
//              all_finite).  ND = 2 is (value, d/d omega, d/dk); ND = 1 is (value, d/d omega), what a Newton step in omega
//              at fixed k needs -- k is then a constant.  Every operator is written once, over the component index, as
//              Jet<ND> of es_jet.hpp is.
//   * all derivatives are holomorphic in omega; k is real and is differentiated as a real parameter, so d/dk of a
//     holomorphic expression is again one complex number per component
//   * the value component of every operation is the one esb::cz operation the plain complex path takes, and the library is
//     built without contraction: component 0 of a jet evaluation is the cz evaluation
//   * the Bessel pairs of es_bessel_complex.hpp are evaluated at the VALUES of their arguments; a pair carries its own
//     argument derivative (lift) by the identities of es_jet.hpp, which hold unchanged at complex argument
//   RealK      a real function of k with its k-derivative, the wavenumber type of the slab's evaluation at CJet<2>; real_of_k
// Builds for the host as well (ES_HD), as es_bessel_complex.hpp does.
#pragma once
#include "es_bessel_complex.hpp"

namespace esb {

// ---- the names the shared text uses for both scalars, for cz -----------------------------------------------------------------
ES_HD cz sqrt(cz a) { return cz_sqrt(a); }
ES_HD cz exp(cz a) { return cz_exp(a); }
ES_HD cz value_of(cz a) { return a; }
ES_HD bool all_finite(cz a) { return cz_finite(a); }
ES_HD cz lift(cz f, cz, cz) { return f; }                      // f(x) of a plain value: no derivative to carry

// ---- the jet -----------------------------------------------------------------------------------------------------------------
template <int ND> struct CJet {
  cz v, d[ND];
  CJet() = default;
  ES_HDM explicit CJet(cz v_) : v(v_) {                        // a constant
    for (int c = 0; c < ND; ++c) d[c] = cz(0.0);
  }
  ES_HDM explicit CJet(double v_) : CJet(cz(v_)) {}
};
template <class T> struct is_cjet { static constexpr bool value = false; };
template <int ND> struct is_cjet<CJet<ND>> { static constexpr bool value = true; };
// what a jet combines with: a complex or a real constant
template <class T> struct is_cconst { static constexpr bool value = is_cz<T>::value || std::is_same<T, double>::value; };

// value v_, derivative component c = fd(c)
template <int ND, class FD> ES_HD CJet<ND> cjet_of(cz v_, FD fd) {
  CJet<ND> r;
  r.v = v_;
  for (int c = 0; c < ND; ++c) r.d[c] = fd(c);
  return r;
}
// the independent variable number `comp` at the value v_ (comp outside 0 .. ND - 1: a constant)
template <int ND> ES_HD CJet<ND> cjet_variable(cz v_, int comp) {
  return cjet_of<ND>(v_, [&](int c) { return cz(c == comp ? 1.0 : 0.0); });
}

template <int ND> ES_HD double val(const CJet<ND>& a) { return a.v.re; }      // as val(cz): what the text branches on
template <int ND> ES_HD cz value_of(const CJet<ND>& a) { return a.v; }
template <int ND> ES_HD bool all_finite(const CJet<ND>& a) {
  bool f = cz_finite(a.v);
  for (int c = 0; c < ND; ++c) f = f && cz_finite(a.d[c]);
  return f;
}

#define ES_CJET template <int ND> ES_HD CJet<ND>
#define ES_CJET_S template <int ND, class S, class = typename std::enable_if<is_cconst<S>::value>::type> ES_HD CJet<ND>
ES_CJET operator-(const CJet<ND>& a) { return cjet_of<ND>(-a.v, [&](int c) { return -a.d[c]; }); }
ES_CJET operator+(const CJet<ND>& a, const CJet<ND>& b) { return cjet_of<ND>(a.v + b.v, [&](int c) { return a.d[c] + b.d[c]; }); }
ES_CJET operator-(const CJet<ND>& a, const CJet<ND>& b) { return cjet_of<ND>(a.v - b.v, [&](int c) { return a.d[c] - b.d[c]; }); }
ES_CJET operator*(const CJet<ND>& a, const CJet<ND>& b) {
  return cjet_of<ND>(a.v * b.v, [&](int c) { return a.v * b.d[c] + a.d[c] * b.v; });
}
// a / b: the derivatives (a' - q b') / b share one reciprocal
ES_CJET operator/(const CJet<ND>& a, const CJet<ND>& b) {
  const cz q = a.v / b.v, r = 1.0 / b.v;
  return cjet_of<ND>(q, [&](int c) { return (a.d[c] - q * b.d[c]) * r; });
}
// against a constant S: cz or double
ES_CJET_S operator+(const CJet<ND>& a, S b) { return cjet_of<ND>(a.v + b, [&](int c) { return a.d[c]; }); }
ES_CJET_S operator+(S a, const CJet<ND>& b) { return cjet_of<ND>(a + b.v, [&](int c) { return b.d[c]; }); }
ES_CJET_S operator-(const CJet<ND>& a, S b) { return cjet_of<ND>(a.v - b, [&](int c) { return a.d[c]; }); }
ES_CJET_S operator-(S a, const CJet<ND>& b) { return cjet_of<ND>(a - b.v, [&](int c) { return -b.d[c]; }); }
ES_CJET_S operator*(const CJet<ND>& a, S b) { return cjet_of<ND>(a.v * b, [&](int c) { return a.d[c] * b; }); }
ES_CJET_S operator*(S a, const CJet<ND>& b) { return cjet_of<ND>(a * b.v, [&](int c) { return a * b.d[c]; }); }
ES_CJET_S operator/(const CJet<ND>& a, S b) { return cjet_of<ND>(a.v / b, [&](int c) { return a.d[c] / b; }); }
ES_CJET_S operator/(S a, const CJet<ND>& b) {
  const cz q = a / b.v, r = 1.0 / b.v;
  return cjet_of<ND>(q, [&](int c) { return -(q * b.d[c]) * r; });
}
template <int ND> ES_HD CJet<ND>& operator*=(CJet<ND>& a, double b) { a = a * b; return a; }
// a b + c_ with at least one jet among jets and real constants: a product and a sum, as fma of cz
template <class A, class B, class C, class = typename std::enable_if<is_cjet<A>::value || is_cjet<B>::value || is_cjet<C>::value>::type>
ES_HD auto fma(const A& a, const B& b, const C& c_) -> decltype(a * b + c_) { return a * b + c_; }
// 1 / a: d(1/a) = -r^2 da
ES_CJET rcp(const CJet<ND>& a) {
  const cz r = 1.0 / a.v, d = -(r * r);
  return cjet_of<ND>(r, [&](int c) { return d * a.d[c]; });
}
// the principal root of the value; d sqrt(a) = da / (2 s)
ES_CJET sqrt(const CJet<ND>& a) {
  const cz s = cz_sqrt(a.v), r = 0.5 / s;
  return cjet_of<ND>(s, [&](int c) { return a.d[c] * r; });
}
ES_CJET exp(const CJet<ND>& a) {
  const cz e = cz_exp(a.v);
  return cjet_of<ND>(e, [&](int c) { return e * a.d[c]; });
}
// f(x) for a function known by its value f and derivative df at the value of x
ES_CJET lift(cz f, cz df, const CJet<ND>& x) { return cjet_of<ND>(f, [&](int c) { return df * x.d[c]; }); }
#undef ES_CJET
#undef ES_CJET_S

// ---- real functions of the wavenumber, for the flow slab's text (es_complex_shared.hpp) ---------------------------------------
// RealK: a real function of k alone -- k, k^2 c^2, k U' -- with its k-derivative, the wavenumber type K of an evaluation at
// CJet<2> = (value, d/d omega, d/dk).  Two doubles and the few operators against CJet<2> below: such a quantity has no
// imaginary part and no d/d omega, and carrying it as a CJet<2> multiplied those zeros through every node (the slab's slopes
// kernel took 14 % longer).  CJet<2>(a) is the explicit widening, for the quotient a / z.
struct RealK {
  double v, dk;
  ES_HDM explicit operator CJet<2>() const {
    CJet<2> r{cz(v)};
    r.d[1] = cz(dk);
    return r;
  }
};
ES_HD double val(RealK a) { return a.v; }
ES_HD RealK operator*(RealK a, double b) { return RealK{a.v * b, a.dk * b}; }
ES_HD RealK operator*(double a, RealK b) { return RealK{a * b.v, a * b.dk}; }
ES_HD CJet<2> operator-(RealK a, const CJet<2>& b) {
  CJet<2> r = -b;
  r.v = a.v - b.v;
  r.d[1] = a.dk - b.d[1];
  return r;
}
ES_HD CJet<2> operator-(const CJet<2>& a, RealK b) {
  CJet<2> r = a;
  r.v = a.v - b.v;
  r.d[1] = a.d[1] - b.dk;
  return r;
}
ES_HD CJet<2> operator*(RealK a, const CJet<2>& b) {
  CJet<2> r;
  r.v = a.v * b.v;
  r.d[0] = a.v * b.d[0];
  r.d[1] = a.v * b.d[1] + a.dk * b.v;
  return r;
}
// The real function of k with value v and k-derivative dv as the wavenumber type of `k` carries it: the value where k is a
// constant of the differentiation (double), the pair where it is the variable (RealK).  The formula text hands over such
// derivatives as it has always rounded them (R / k, not -R (1 / k)): no jet arithmetic is asked to derive them again.
ES_HD double real_of_k(double, double v, double) { return v; }
ES_HD RealK real_of_k(RealK, double v, double dv) { return RealK{v, dv}; }

// d/dz [e^z K_n] = e^z K_n - e^z K_{n+1} + (n/z) e^z K_n ;  d/dz [e^z K_{n+1}] = e^z K_{n+1} - e^z K_n - ((n+1)/z) e^z K_{n+1}
template <int ND> ES_HD void cke_pair(int n, const CJet<ND>& z, CJet<ND>& K, CJet<ND>& K1) {
  const double dn = (double)n;
  cz vK, vK1;
  cke_pair(n, z.v, vK, vK1);
  K = lift(vK, vK - vK1 + (dn / z.v) * vK, z);
  K1 = lift(vK1, vK1 - vK - ((dn + 1.0) / z.v) * vK1, z);
}
// d/dz [e^-z I_n] = -e^-z I_n + e^-z I_{n+1} + (n/z) e^-z I_n ;  d/dz [e^-z I_{n+1}] = -e^-z I_{n+1} + e^-z I_n - ((n+1)/z) e^-z I_{n+1}
template <int ND>
ES_HD void cie_pair_from_k(int n, const CJet<ND>& z, const CJet<ND>& K, const CJet<ND>& K1, CJet<ND>& I, CJet<ND>& I1) {
  const double dn = (double)n;
  cz vI, vI1;
  cie_pair_from_k(n, z.v, K.v, K1.v, vI, vI1);
  I = lift(vI, vI1 - vI + (dn / z.v) * vI, z);
  I1 = lift(vI1, vI - vI1 - ((dn + 1.0) / z.v) * vI1, z);
}

}  // namespace esb
