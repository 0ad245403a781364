// Forward-mode jets of the complex cylinder path (include/eigensolver_amd.h section 15).
//   CJet<ND>   an esb::cz value with ND esb::cz derivative components, and the operators and overloads the FAM_CYL0 formula
//              text of es_shoot_device.hpp and the exterior of es_cyl_complex_shared.hpp need of their scalar type (fma, rcp,
//              sqrt, exp, val, lift, cke_pair, cie_pair_from_k, all_finite).  ND = 2 is (value, d/d omega, d/dk); ND = 1 is
//              (value, d/d omega), what a Newton step in omega at fixed k needs -- k is then a constant.  Every operator is
//              written once, over the component index, as Jet<ND> of es_jet.hpp is.
//   * all derivatives are holomorphic in omega; k is real and is differentiated as a real parameter, so d/dk of a
//     holomorphic expression is again one complex number per component
//   * the value component of every operation is the one esb::cz operation the plain complex path takes, and the library is
//     built without contraction: component 0 of a jet evaluation is the cz evaluation
//   * the Bessel pairs of es_bessel_complex.hpp are evaluated at the VALUES of their arguments; a pair carries its own
//     argument derivative (lift) by the identities of es_jet.hpp, which hold unchanged at complex argument
// Builds for the host as well (ES_HD), as es_bessel_complex.hpp does.
#pragma once
#include "es_bessel_complex.hpp"

namespace esb {

// ---- the names the shared text uses for both scalars, for cz -----------------------------------------------------------------
ES_HD cz sqrt(cz a) { return cz_sqrt(a); }
ES_HD cz exp(cz a) { return cz_exp(a); }
ES_HD cz value_of(cz a) { return a; }
ES_HD bool all_finite(cz a) { return cz_finite(a); }

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
