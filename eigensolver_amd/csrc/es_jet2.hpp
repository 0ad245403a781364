// Second-order forward-mode jets of the real shooting path (include/eigensolver_amd.h section 21).
//   Jet2<NV>   a first-order Jet<NV> of es_jet.hpp (value, NV first derivatives) and the NV (NV + 1) / 2 second derivatives
//              h[] of the same quantity, pairs (a, b) with a <= b in row order.  NV = 2: omega is variable 0, k variable 1 and
//              h = (d2/d omega2, d2/d omega dk, d2/dk2); NV = 1: omega alone, h = (d2/d omega2), what a Halley step needs.
//   * every operator and overload forms its value and first-order part BY CALLING the Jet<NV> one, so those components are
//     the arithmetic of Jet<NV> operation for operation, and adds the second-order part by the product and chain rules
//   * the scaled Bessel pairs are still evaluated once, at the value of their argument; their second argument derivative is
//     the recurrence identities of es_jet.hpp applied to their own result
//   * the march is jet_march_of<FAM, Jet2<NV>, TRACK> of es_jet.hpp: no formula is restated here
#pragma once
#include "es_jet.hpp"

template <int NV> struct Jet2 {
  static constexpr int NH = NV * (NV + 1) / 2;
  Jet<NV> j;
  double h[NH];
  Jet2() = default;
  __device__ explicit Jet2(double v_) : j(v_) {                // a constant
#pragma unroll
    for (int p = 0; p < NH; ++p) h[p] = 0.0;
  }
};

// first-order part j_, second derivative of the pair (a, b), a <= b, at index p of h[] = fh(a, b, p)
template <int NV, class FH> __device__ __forceinline__ Jet2<NV> jet2_of(const Jet<NV>& j_, FH fh) {
  Jet2<NV> r;
  r.j = j_;
  int p = 0;
#pragma unroll
  for (int a = 0; a < NV; ++a)
#pragma unroll
    for (int b = a; b < NV; ++b, ++p) r.h[p] = fh(a, b, p);
  return r;
}
template <int NV> struct JetVariable<Jet2<NV>> {
  static __device__ __forceinline__ Jet2<NV> make(double v_, int comp) {
    return jet2_of<NV>(jet_variable<NV>(v_, comp), [](int, int, int) { return 0.0; });
  }
};

template <int NV> __device__ __forceinline__ double val(const Jet2<NV>& a) { return a.j.v; }
#define ES_JET2 template <int NV> __device__ __forceinline__ Jet2<NV>
ES_JET2 operator-(const Jet2<NV>& x) { return jet2_of<NV>(-x.j, [&](int, int, int p) { return -x.h[p]; }); }
ES_JET2 operator+(const Jet2<NV>& x, const Jet2<NV>& y) { return jet2_of<NV>(x.j + y.j, [&](int, int, int p) { return x.h[p] + y.h[p]; }); }
ES_JET2 operator-(const Jet2<NV>& x, const Jet2<NV>& y) { return jet2_of<NV>(x.j - y.j, [&](int, int, int p) { return x.h[p] - y.h[p]; }); }
ES_JET2 operator+(const Jet2<NV>& x, double y) { return jet2_of<NV>(x.j + y, [&](int, int, int p) { return x.h[p]; }); }
ES_JET2 operator+(double x, const Jet2<NV>& y) { return jet2_of<NV>(x + y.j, [&](int, int, int p) { return y.h[p]; }); }
ES_JET2 operator-(const Jet2<NV>& x, double y) { return jet2_of<NV>(x.j - y, [&](int, int, int p) { return x.h[p]; }); }
ES_JET2 operator-(double x, const Jet2<NV>& y) { return jet2_of<NV>(x - y.j, [&](int, int, int p) { return -y.h[p]; }); }
ES_JET2 operator*(const Jet2<NV>& x, double y) { return jet2_of<NV>(x.j * y, [&](int, int, int p) { return x.h[p] * y; }); }
ES_JET2 operator*(double x, const Jet2<NV>& y) { return jet2_of<NV>(x * y.j, [&](int, int, int p) { return x * y.h[p]; }); }
template <int NV> __device__ __forceinline__ Jet2<NV>& operator*=(Jet2<NV>& x, double y) { x = x * y; return x; }
// (x y)_ab = x y_ab + x_ab y + x_a y_b + x_b y_a
template <int NV> __device__ __forceinline__ double jet2_cross(const Jet<NV>& x, const Jet<NV>& y, int a, int b) {
  return fma(x.d[a], y.d[b], x.d[b] * y.d[a]);
}
ES_JET2 operator*(const Jet2<NV>& x, const Jet2<NV>& y) {
  return jet2_of<NV>(x.j * y.j, [&](int a, int b, int p) { return fma(x.j.v, y.h[p], fma(x.h[p], y.j.v, jet2_cross(x.j, y.j, a, b))); });
}
ES_JET2 fma(const Jet2<NV>& x, const Jet2<NV>& y, const Jet2<NV>& z) {
  return jet2_of<NV>(fma(x.j, y.j, z.j), [&](int a, int b, int p) {
    return fma(x.j.v, y.h[p], fma(x.h[p], y.j.v, jet2_cross(x.j, y.j, a, b) + z.h[p]));
  });
}
ES_JET2 fma(double x, const Jet2<NV>& y, const Jet2<NV>& z) {
  return jet2_of<NV>(fma(x, y.j, z.j), [&](int, int, int p) { return fma(x, y.h[p], z.h[p]); });
}
ES_JET2 fma(const Jet2<NV>& x, const Jet2<NV>& y, double z) {
  return jet2_of<NV>(fma(x.j, y.j, z), [&](int a, int b, int p) { return fma(x.j.v, y.h[p], fma(x.h[p], y.j.v, jet2_cross(x.j, y.j, a, b))); });
}
ES_JET2 fma(double x, const Jet2<NV>& y, double z) { return jet2_of<NV>(fma(x, y.j, z), [&](int, int, int p) { return x * y.h[p]; }); }
ES_JET2 fma(const Jet2<NV>& x, double y, const Jet2<NV>& z) {
  return jet2_of<NV>(fma(x.j, y, z.j), [&](int, int, int p) { return fma(x.h[p], y, z.h[p]); });
}
ES_JET2 fma(const Jet2<NV>& x, double y, double z) { return jet2_of<NV>(fma(x.j, y, z), [&](int, int, int p) { return x.h[p] * y; }); }
// 1 / x from its value's reciprocal r: (1/x)_ab = -r^2 x_ab + 2 r^3 x_a x_b
ES_JET2 rcp_from(const Jet2<NV>& x, double r) {
  const double d1 = -(r * r), d2 = -2.0 * (d1 * r);
  return jet2_of<NV>(rcp_from(x.j, r), [&](int a, int b, int p) { return fma(d1, x.h[p], d2 * (x.j.d[a] * x.j.d[b])); });
}
ES_JET2 rcp(const Jet2<NV>& x) { return rcp_from(x, 1.0 / x.j.v); }                // IEEE quotient
ES_JET2 fast_rcp(const Jet2<NV>& x) { return rcp_from(x, fast_rcp(x.j.v)); }       // the march's reciprocal
// q = x / y from x = q y: q_ab = (x_ab - q y_ab - q_a y_b - q_b y_a) / y, with the first derivatives of the quotient itself
ES_JET2 operator/(const Jet2<NV>& x, const Jet2<NV>& y) {
  const Jet<NV> q = x.j / y.j;
  const double r = 1.0 / y.j.v;
  return jet2_of<NV>(q, [&](int a, int b, int p) { return (x.h[p] - fma(q.v, y.h[p], jet2_cross(q, y.j, a, b))) * r; });
}
ES_JET2 operator/(double x, const Jet2<NV>& y) {
  const Jet<NV> q = x / y.j;
  const double r = 1.0 / y.j.v;
  return jet2_of<NV>(q, [&](int a, int b, int p) { return -fma(q.v, y.h[p], jet2_cross(q, y.j, a, b)) * r; });
}
ES_JET2 operator/(const Jet2<NV>& x, double y) { return jet2_of<NV>(x.j / y, [&](int, int, int p) { return x.h[p] / y; }); }
// s = sqrt(x) from s^2 = x: s_ab = (x_ab - 2 s_a s_b) / (2 s)
ES_JET2 sqrt(const Jet2<NV>& x) {
  const Jet<NV> s = sqrt(x.j);
  const double r = 0.5 / s.v;
  return jet2_of<NV>(s, [&](int a, int b, int p) { return fma(-2.0 * s.d[a], s.d[b], x.h[p]) * r; });
}
ES_JET2 exp(const Jet2<NV>& x) {
  const Jet<NV> e = exp(x.j);
  return jet2_of<NV>(e, [&](int a, int b, int p) { return e.v * fma(x.j.d[a], x.j.d[b], x.h[p]); });
}
ES_JET2 ldexp(const Jet2<NV>& x, int ex) { return jet2_of<NV>(ldexp(x.j, ex), [&](int, int, int p) { return ldexp(x.h[p], ex); }); }
// f(x) for a function known by its derivatives df, d2f at the value of x, onto its first-order jet: f_ab = df x_ab + d2f x_a x_b
ES_JET2 lift_onto(const Jet<NV>& first, double df, double d2f, const Jet2<NV>& x) {
  return jet2_of<NV>(first, [&](int a, int b, int p) { return fma(df, x.h[p], d2f * (x.j.d[a] * x.j.d[b])); });
}
ES_JET2 lift(double f, double df, double d2f, const Jet2<NV>& x) { return lift_onto(lift(f, df, x.j), df, d2f, x); }
// |x|: differentiates as sign(x) dx
ES_JET2 fabs(const Jet2<NV>& x) {
  const double sg = (x.j.v < 0.0) ? -1.0 : 1.0;
  return jet2_of<NV>(fabs(x.j), [&](int, int, int p) { return sg * x.h[p]; });
}
#undef ES_JET2
// The pairs of es_jet.hpp, whose overloads deliver the value and first-order part, with the identities applied a second time
// for the second-order part (dK, dI below enter that part alone): with A = e^x K_n, B = e^x K_{n+1},
//   A' = A - B + (n/x) A,  B' = B - A - ((n+1)/x) B   =>   A'' = A' - B' + (n/x) A' - (n/x^2) A,
//                                                         B'' = B' - A' - ((n+1)/x) B' + ((n+1)/x^2) B
template <int NV> __device__ __forceinline__ void ke_pair(int n, const Jet2<NV>& x, Jet2<NV>& K, Jet2<NV>& K1) {
  Jet<NV> A, B;
  ke_pair(n, x.j, A, B);
  const double nx = (double)n / x.j.v, n1x = ((double)n + 1.0) / x.j.v;
  const double dK = A.v - B.v + nx * A.v, dK1 = B.v - A.v - n1x * B.v;
  K = lift_onto(A, dK, dK - dK1 + nx * dK - (nx / x.j.v) * A.v, x);
  K1 = lift_onto(B, dK1, dK1 - dK - n1x * dK1 + (n1x / x.j.v) * B.v, x);
}
// with A = e^-x I_n, B = e^-x I_{n+1}:  A' = B - A + (n/x) A,  B' = A - B - ((n+1)/x) B   =>
//   A'' = B' - A' + (n/x) A' - (n/x^2) A,  B'' = A' - B' - ((n+1)/x) B' + ((n+1)/x^2) B
template <int NV>
__device__ __forceinline__ void ie_pair_from_k(int n, const Jet2<NV>& x, const Jet2<NV>& K, const Jet2<NV>& K1, Jet2<NV>& I,
                                               Jet2<NV>& I1) {
  Jet<NV> A, B;
  ie_pair_from_k(n, x.j, K.j, K1.j, A, B);
  const double nx = (double)n / x.j.v, n1x = ((double)n + 1.0) / x.j.v;
  const double dI = B.v - A.v + nx * A.v, dI1 = A.v - B.v - n1x * B.v;
  I = lift_onto(A, dI, dI1 - dI + nx * dI - (nx / x.j.v) * A.v, x);
  I1 = lift_onto(B, dI1, dI - dI1 - n1x * dI1 + (n1x / x.j.v) * B.v, x);
}
template <int NV> __device__ __forceinline__ bool jet_finite(const Jet2<NV>& x) {
  bool f = jet_finite(x.j);
#pragma unroll
  for (int p = 0; p < Jet2<NV>::NH; ++p) f = f && isfinite(x.h[p]);
  return f;
}
