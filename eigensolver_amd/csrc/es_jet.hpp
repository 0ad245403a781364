// Forward-mode jets of the real shooting path and the one-pair jet march (include/eigensolver_amd.h sections 11 and 13).
//   Jet<ND>    a value with ND derivative components, and the operators and overloads the formula text of es_shoot_device.hpp
//              needs of its scalar type (fma, sqrt, exp, fabs, ldexp, fast_rcp, rcp, ke_pair, ie_pair_from_k, val).  ND = 2 is
//              (value, d/d omega, d/dk), the Jet3 of es_shoot_root_slopes; ND = 1 is (value, d/d omega), what a Newton step in
//              omega at fixed k needs -- k is then a constant jet.  Every operator is written once, over the component index.
//   jet_march  the determinant's two sides at one (k, omega) pair in Jet<ND> (jet_march_of: the same in any jet type, the
//              second-order ones of es_jet2.hpp included): exterior, node entries by scalar loads (wave-uniform addresses,
//              as mode_signature_kernel), the adjoint march with one reciprocal per RK4 step, the rescaling at the chunk
//              ends and the boundary algebra.  Nothing is staged in LDS and there is no barrier: a lane may call it alone.
//   * the node entries of make_entry depend on k only; the base fields themselves are wave-uniform, so make_entry delivers
//     the k-dependent entries as jets and the others as plain doubles (its two output arrays)
//   * the Bessel pairs of es_bessel.hpp are evaluated at the VALUES of their arguments; a pair (e^x K_n, e^x K_{n+1}) resp.
//     e^-x (I_n, I_{n+1}) carries its own argument derivative (lift), the jet enters by the chain rule
// The value component is the arithmetic of the fp64 point march up to the grouping of the reciprocals (one per RK4 step here,
// one per two steps there for the families with fam_rcp4()).
#pragma once
#include "es_shoot_shared.hpp"

template <int ND> struct Jet {
  double v, d[ND];
  Jet() = default;
  __device__ explicit Jet(double v_) : v(v_) {                 // a constant
#pragma unroll
    for (int c = 0; c < ND; ++c) d[c] = 0.0;
  }
};
using Jet3 = Jet<2>;                                           // (value, d/d omega, d/dk)

// value v_, derivative component c = fd(c)
template <int ND, class FD> __device__ __forceinline__ Jet<ND> jet_of(double v_, FD fd) {
  Jet<ND> r;
  r.v = v_;
#pragma unroll
  for (int c = 0; c < ND; ++c) r.d[c] = fd(c);
  return r;
}
// the independent variable number `comp` at the value v_ (comp outside 0 .. ND - 1: a constant)
template <int ND> __device__ __forceinline__ Jet<ND> jet_variable(double v_, int comp) {
  return jet_of<ND>(v_, [&](int c) { return c == comp ? 1.0 : 0.0; });
}

template <int ND> __device__ __forceinline__ double val(const Jet<ND>& a) { return a.v; }
#define ES_JET template <int ND> __device__ __forceinline__ Jet<ND>
ES_JET operator-(const Jet<ND>& a) { return jet_of<ND>(-a.v, [&](int c) { return -a.d[c]; }); }
ES_JET operator+(const Jet<ND>& a, const Jet<ND>& b) { return jet_of<ND>(a.v + b.v, [&](int c) { return a.d[c] + b.d[c]; }); }
ES_JET operator-(const Jet<ND>& a, const Jet<ND>& b) { return jet_of<ND>(a.v - b.v, [&](int c) { return a.d[c] - b.d[c]; }); }
ES_JET operator+(const Jet<ND>& a, double b) { return jet_of<ND>(a.v + b, [&](int c) { return a.d[c]; }); }
ES_JET operator+(double a, const Jet<ND>& b) { return jet_of<ND>(a + b.v, [&](int c) { return b.d[c]; }); }
ES_JET operator-(const Jet<ND>& a, double b) { return jet_of<ND>(a.v - b, [&](int c) { return a.d[c]; }); }
ES_JET operator-(double a, const Jet<ND>& b) { return jet_of<ND>(a - b.v, [&](int c) { return -b.d[c]; }); }
ES_JET operator*(const Jet<ND>& a, double b) { return jet_of<ND>(a.v * b, [&](int c) { return a.d[c] * b; }); }
ES_JET operator*(double a, const Jet<ND>& b) { return jet_of<ND>(a * b.v, [&](int c) { return a * b.d[c]; }); }
template <int ND> __device__ __forceinline__ Jet<ND>& operator*=(Jet<ND>& a, double b) { a = a * b; return a; }
ES_JET operator*(const Jet<ND>& a, const Jet<ND>& b) {
  return jet_of<ND>(a.v * b.v, [&](int c) { return fma(a.v, b.d[c], a.d[c] * b.v); });
}
// a b + c, the value as the one fma the scalar code takes
ES_JET fma(const Jet<ND>& a, const Jet<ND>& b, const Jet<ND>& c_) {
  return jet_of<ND>(fma(a.v, b.v, c_.v), [&](int c) { return fma(a.v, b.d[c], fma(a.d[c], b.v, c_.d[c])); });
}
ES_JET fma(double a, const Jet<ND>& b, const Jet<ND>& c_) {
  return jet_of<ND>(fma(a, b.v, c_.v), [&](int c) { return fma(a, b.d[c], c_.d[c]); });
}
ES_JET fma(const Jet<ND>& a, const Jet<ND>& b, double c_) {
  return jet_of<ND>(fma(a.v, b.v, c_), [&](int c) { return fma(a.v, b.d[c], a.d[c] * b.v); });
}
ES_JET fma(double a, const Jet<ND>& b, double c_) { return jet_of<ND>(fma(a, b.v, c_), [&](int c) { return a * b.d[c]; }); }
ES_JET fma(const Jet<ND>& a, double b, const Jet<ND>& c_) {
  return jet_of<ND>(fma(a.v, b, c_.v), [&](int c) { return fma(a.d[c], b, c_.d[c]); });
}
ES_JET fma(const Jet<ND>& a, double b, double c_) { return jet_of<ND>(fma(a.v, b, c_), [&](int c) { return a.d[c] * b; }); }
// 1 / a from its value's reciprocal r: d(1/a) = -r^2 da
ES_JET rcp_from(const Jet<ND>& a, double r) {
  const double d = -(r * r);
  return jet_of<ND>(r, [&](int c) { return d * a.d[c]; });
}
ES_JET rcp(const Jet<ND>& a) { return rcp_from(a, 1.0 / a.v); }                  // IEEE quotient
ES_JET fast_rcp(const Jet<ND>& a) { return rcp_from(a, fast_rcp(a.v)); }         // the march's reciprocal
ES_JET operator/(const Jet<ND>& a, const Jet<ND>& b) {
  const double q = a.v / b.v, r = 1.0 / b.v;
  return jet_of<ND>(q, [&](int c) { return (a.d[c] - q * b.d[c]) * r; });
}
ES_JET operator/(double a, const Jet<ND>& b) {
  const double q = a / b.v, r = 1.0 / b.v;
  return jet_of<ND>(q, [&](int c) { return -(q * b.d[c]) * r; });
}
ES_JET operator/(const Jet<ND>& a, double b) { return jet_of<ND>(a.v / b, [&](int c) { return a.d[c] / b; }); }
ES_JET sqrt(const Jet<ND>& a) {
  const double s = sqrt(a.v), r = 0.5 / s;
  return jet_of<ND>(s, [&](int c) { return a.d[c] * r; });
}
ES_JET exp(const Jet<ND>& a) {
  const double e = exp(a.v);
  return jet_of<ND>(e, [&](int c) { return e * a.d[c]; });
}
ES_JET ldexp(const Jet<ND>& a, int ex) { return jet_of<ND>(ldexp(a.v, ex), [&](int c) { return ldexp(a.d[c], ex); }); }
// f(x) for a function known by its value f and derivative df at the value of x
ES_JET lift(double f, double df, const Jet<ND>& x) { return jet_of<ND>(f, [&](int c) { return df * x.d[c]; }); }
// |a|: differentiates as sign(a) da
ES_JET fabs(const Jet<ND>& a) {
  const double sg = (a.v < 0.0) ? -1.0 : 1.0;
  return jet_of<ND>(fabs(a.v), [&](int c) { return sg * a.d[c]; });
}
#undef ES_JET
// d/dx [e^x K_n] = e^x K_n - e^x K_{n+1} + (n/x) e^x K_n ;  d/dx [e^x K_{n+1}] = e^x K_{n+1} - e^x K_n - ((n+1)/x) e^x K_{n+1}
template <int ND> __device__ __forceinline__ void ke_pair(int n, const Jet<ND>& x, Jet<ND>& K, Jet<ND>& K1) {
  const double dn = (double)n;
  double vK, vK1;
  esb::ke_pair(n, x.v, vK, vK1);
  K = lift(vK, vK - vK1 + (dn / x.v) * vK, x);
  K1 = lift(vK1, vK1 - vK - ((dn + 1.0) / x.v) * vK1, x);
}
// d/dx [e^-x I_n] = -e^-x I_n + e^-x I_{n+1} + (n/x) e^-x I_n ;  d/dx [e^-x I_{n+1}] = -e^-x I_{n+1} + e^-x I_n - ((n+1)/x) e^-x I_{n+1}
template <int ND>
__device__ __forceinline__ void ie_pair_from_k(int n, const Jet<ND>& x, const Jet<ND>& K, const Jet<ND>& K1, Jet<ND>& I,
                                               Jet<ND>& I1) {
  const double dn = (double)n;
  double vI, vI1;
  esb::ie_pair_from_k(n, x.v, K.v, K1.v, vI, vI1);
  I = lift(vI, vI1 - vI + (dn / x.v) * vI, x);
  I1 = lift(vI1, vI - vI1 - ((dn + 1.0) / x.v) * vI1, x);
}
template <int ND> __device__ __forceinline__ bool jet_finite(const Jet<ND>& a) {
  bool f = isfinite(a.v);
#pragma unroll
  for (int c = 0; c < ND; ++c) f = f && isfinite(a.d[c]);
  return f;
}

// What jet_march returns: the two sides of the matching condition, the exterior status (ES_PT_OK / LEAKY / NONFINITE) and,
// with TRACK, whether a watched term of the coefficients took both signs over the nodes (SignTrack::crossed).
template <class J> struct JetMatchT {
  J outer, inner;
  int status;
  bool crossed;
};
template <int ND> using JetMatch = JetMatchT<Jet<ND>>;

// J's independent variable number `comp` at the value v_: what the march needs of a jet type besides its operators
// (es_jet2.hpp gives the second-order Jet2<NV> the same)
template <class J> struct JetVariable;
template <int ND> struct JetVariable<Jet<ND>> {
  static __device__ __forceinline__ Jet<ND> make(double v_, int comp) { return jet_variable<ND>(v_, comp); }
};

// One (k, omega) pair in the jet type J: omega is variable 0 of the jets, k variable 1 (a constant for a jet of one
// variable).  TRACK: coef_pre follows the signs of the watched terms through val(), as the value marches do.
template <int FAM, class J, bool TRACK>
__device__ __forceinline__ JetMatchT<J> jet_march_of(const ShootDev& P, double kv, double wv) {
  using namespace es_shoot_shared;
  constexpr int NB = FamTraits<FAM>::NB;
  constexpr int NE = FamTraits<FAM>::NE;
  const J w = JetVariable<J>::make(wv, 0);
  const KScalT<J> s = make_kscal(P, JetVariable<J>::make(kv, 1));
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  const ExteriorLiteT<J> X = exterior_lite<FAM>(P, s.k, w, w);
  SignTrack trk;
  double b[NB], cm[NE], c1[NE];                                // node entries: em, e1 depend on k (jets), cm, c1 do not
  J em[NE], e1[NE];
  CoefT<J> B0;
  load_base<FAM>(P, 2 * nsteps, b);
  make_entry<FAM, fam_scaled<FAM>()>(b, s, e1, c1);
  CoefPreT<J> C0;
  coef_pre<FAM, TRACK>(e1, c1, P, s, w, C0, trk);
  coef_finish<FAM>(C0, rcp(C0.den), B0);                       // first node of the traversal: its own division
  J zp, zq;
  adjoint_start<FAM>(P, B0, zp, zq);
  for (int j = nsteps - 1; j >= 0; --j) {
    CoefT<J> Bm, B1;
    CoefPreT<J> Cm, C1;
    // coefficients2 spelled out, each node's entries formed right before its coef_pre: 8 and 12 VGPRs less for the cylinders
    load_base<FAM>(P, 2 * j + 1, b);
    make_entry<FAM, fam_scaled<FAM>()>(b, s, em, cm);
    coef_pre<FAM, TRACK>(em, cm, P, s, w, Cm, trk);
    load_base<FAM>(P, 2 * j, b);
    make_entry<FAM, fam_scaled<FAM>()>(b, s, e1, c1);
    coef_pre<FAM, TRACK>(e1, c1, P, s, w, C1, trk);
    const J inv = fast_rcp(Cm.den * C1.den);
    coef_finish<FAM>(Cm, C1.den * inv, Bm);
    coef_finish<FAM>(C1, Cm.den * inv, B1);
    adjoint_step<FAM>(zp, zq, B0, Bm, B1, h, h2, h6, h3);
    B0 = B1;
    if ((j % CH) == 0) {
      // the power of two the point march takes at the end of its LDS chunk [j, j + nst): the scale P.bc_const carries
      const int nst = (nsteps - j < CH) ? (nsteps - j) : CH;
      adjoint_rescale<FAM>(zp, zq, nsteps - j - nst, nsteps - j);
    }
  }
  load_base<FAM>(P, 0, b);
  make_entry<FAM>(b, s, e1, c1);                               // the boundary node
  const MismatchT<J> M = boundary_algebra<FAM>(P, s, w, X, zp, zq, e1);
  JetMatchT<J> R;
  R.outer = M.outer;
  R.inner = M.inner;
  R.status = X.status;
  R.crossed = TRACK ? trk.crossed() : false;
  return R;
}

template <int FAM, int ND, bool TRACK>
__device__ __forceinline__ JetMatch<ND> jet_march(const ShootDev& P, double kv, double wv) {
  return jet_march_of<FAM, Jet<ND>, TRACK>(P, kv, wv);
}
