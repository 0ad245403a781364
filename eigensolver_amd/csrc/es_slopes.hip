// Dispersion slopes of a (k, omega) pair: the boundary determinant D = outer - inner of es_shoot_eval_points together with its
// exact partial derivatives in omega and k (include/eigensolver_amd.h section 11).  Tangent-linear (forward-mode) evaluation:
// the node entries, coefficient sets, adjoint RK4 steps, closed-form exterior and boundary algebra of es_shoot_device.hpp,
// instantiated over 3-component jets (value, d/d omega, d/d k) -- the text the value kernels instantiate over double.  This
// file holds the jet type with the operators and overloads that text needs, the kernel, the launcher and the ABI entry.  One
// pair per lane, node base fields by scalar loads (wave-uniform addresses, as mode_signature_kernel); nothing is staged in
// LDS and each lane stores once per output at the end.
//   * the node entries of make_entry depend on k only; the base fields themselves are wave-uniform, so make_entry delivers
//     the k-dependent entries as jets and the others as plain doubles (its two output arrays)
//   * the Bessel pairs of es_bessel.hpp are evaluated at the VALUES of their arguments; a pair (e^x K_n, e^x K_{n+1}) resp.
//     e^-x (I_n, I_{n+1}) carries its own argument derivative (lift), the jet enters by the chain rule
// The value component is the arithmetic of the fp64 point march up to the grouping of the reciprocals (one per RK4 step here,
// one per two steps there for the families with fam_rcp4()).
#include "es_shoot_shared.hpp"

namespace {
using namespace es_shoot_shared;

using ::fma;                                                   // the overloads below would hide the scalar functions
using ::ldexp;

struct Jet3 {
  double v, dw, dk;
  Jet3() = default;
  __device__ Jet3(double v_, double dw_, double dk_) : v(v_), dw(dw_), dk(dk_) {}
  __device__ explicit Jet3(double v_) : v(v_), dw(0.0), dk(0.0) {}   // a constant
};

__device__ __forceinline__ double val(const Jet3& a) { return a.v; }
__device__ __forceinline__ Jet3 operator-(const Jet3& a) { return {-a.v, -a.dw, -a.dk}; }
__device__ __forceinline__ Jet3 operator+(const Jet3& a, const Jet3& b) { return {a.v + b.v, a.dw + b.dw, a.dk + b.dk}; }
__device__ __forceinline__ Jet3 operator-(const Jet3& a, const Jet3& b) { return {a.v - b.v, a.dw - b.dw, a.dk - b.dk}; }
__device__ __forceinline__ Jet3 operator+(const Jet3& a, double b) { return {a.v + b, a.dw, a.dk}; }
__device__ __forceinline__ Jet3 operator+(double a, const Jet3& b) { return {a + b.v, b.dw, b.dk}; }
__device__ __forceinline__ Jet3 operator-(const Jet3& a, double b) { return {a.v - b, a.dw, a.dk}; }
__device__ __forceinline__ Jet3 operator-(double a, const Jet3& b) { return {a - b.v, -b.dw, -b.dk}; }
__device__ __forceinline__ Jet3 operator*(const Jet3& a, double b) { return {a.v * b, a.dw * b, a.dk * b}; }
__device__ __forceinline__ Jet3 operator*(double a, const Jet3& b) { return {a * b.v, a * b.dw, a * b.dk}; }
__device__ __forceinline__ Jet3& operator*=(Jet3& a, double b) { a = a * b; return a; }
__device__ __forceinline__ Jet3 operator*(const Jet3& a, const Jet3& b) {
  return {a.v * b.v, fma(a.v, b.dw, a.dw * b.v), fma(a.v, b.dk, a.dk * b.v)};
}
// a b + c, the value as the one fma the scalar code takes
__device__ __forceinline__ Jet3 fma(const Jet3& a, const Jet3& b, const Jet3& c) {
  return {fma(a.v, b.v, c.v), fma(a.v, b.dw, fma(a.dw, b.v, c.dw)), fma(a.v, b.dk, fma(a.dk, b.v, c.dk))};
}
__device__ __forceinline__ Jet3 fma(double a, const Jet3& b, const Jet3& c) {
  return {fma(a, b.v, c.v), fma(a, b.dw, c.dw), fma(a, b.dk, c.dk)};
}
__device__ __forceinline__ Jet3 fma(const Jet3& a, const Jet3& b, double c) {
  return {fma(a.v, b.v, c), fma(a.v, b.dw, a.dw * b.v), fma(a.v, b.dk, a.dk * b.v)};
}
__device__ __forceinline__ Jet3 fma(double a, const Jet3& b, double c) { return {fma(a, b.v, c), a * b.dw, a * b.dk}; }
__device__ __forceinline__ Jet3 fma(const Jet3& a, double b, const Jet3& c) {
  return {fma(a.v, b, c.v), fma(a.dw, b, c.dw), fma(a.dk, b, c.dk)};
}
__device__ __forceinline__ Jet3 fma(const Jet3& a, double b, double c) { return {fma(a.v, b, c), a.dw * b, a.dk * b}; }
// 1 / a from its value's reciprocal r: d(1/a) = -r^2 da
__device__ __forceinline__ Jet3 rcp_from(const Jet3& a, double r) {
  const double d = -(r * r);
  return {r, d * a.dw, d * a.dk};
}
__device__ __forceinline__ Jet3 rcp(const Jet3& a) { return rcp_from(a, 1.0 / a.v); }            // IEEE quotient
__device__ __forceinline__ Jet3 fast_rcp(const Jet3& a) { return rcp_from(a, ::fast_rcp(a.v)); } // the march's reciprocal
__device__ __forceinline__ Jet3 operator/(const Jet3& a, const Jet3& b) {
  const double q = a.v / b.v, r = 1.0 / b.v;
  return {q, (a.dw - q * b.dw) * r, (a.dk - q * b.dk) * r};
}
__device__ __forceinline__ Jet3 operator/(double a, const Jet3& b) {
  const double q = a / b.v, r = 1.0 / b.v;
  return {q, -(q * b.dw) * r, -(q * b.dk) * r};
}
__device__ __forceinline__ Jet3 operator/(const Jet3& a, double b) { return {a.v / b, a.dw / b, a.dk / b}; }
__device__ __forceinline__ Jet3 sqrt(const Jet3& a) {
  const double s = ::sqrt(a.v), r = 0.5 / s;
  return {s, a.dw * r, a.dk * r};
}
__device__ __forceinline__ Jet3 exp(const Jet3& a) {
  const double e = ::exp(a.v);
  return {e, e * a.dw, e * a.dk};
}
__device__ __forceinline__ Jet3 ldexp(const Jet3& a, int ex) { return {::ldexp(a.v, ex), ::ldexp(a.dw, ex), ::ldexp(a.dk, ex)}; }
// f(x) for a function known by its value f and derivative df at the value of x
__device__ __forceinline__ Jet3 lift(double f, double df, const Jet3& x) { return {f, df * x.dw, df * x.dk}; }
// |a|: differentiates as sign(a) da
__device__ __forceinline__ Jet3 fabs(const Jet3& a) {
  const double sg = (a.v < 0.0) ? -1.0 : 1.0;
  return {::fabs(a.v), sg * a.dw, sg * a.dk};
}
// d/dx [e^x K_n] = e^x K_n - e^x K_{n+1} + (n/x) e^x K_n ;  d/dx [e^x K_{n+1}] = e^x K_{n+1} - e^x K_n - ((n+1)/x) e^x K_{n+1}
__device__ __forceinline__ void ke_pair(int n, const Jet3& x, Jet3& K, Jet3& K1) {
  const double dn = (double)n;
  double vK, vK1;
  esb::ke_pair(n, x.v, vK, vK1);
  K = lift(vK, vK - vK1 + (dn / x.v) * vK, x);
  K1 = lift(vK1, vK1 - vK - ((dn + 1.0) / x.v) * vK1, x);
}
// d/dx [e^-x I_n] = -e^-x I_n + e^-x I_{n+1} + (n/x) e^-x I_n ;  d/dx [e^-x I_{n+1}] = -e^-x I_{n+1} + e^-x I_n - ((n+1)/x) e^-x I_{n+1}
__device__ __forceinline__ void ie_pair_from_k(int n, const Jet3& x, const Jet3& K, const Jet3& K1, Jet3& I, Jet3& I1) {
  const double dn = (double)n;
  double vI, vI1;
  esb::ie_pair_from_k(n, x.v, K.v, K1.v, vI, vI1);
  I = lift(vI, vI1 - vI + (dn / x.v) * vI, x);
  I1 = lift(vI1, vI - vI1 - ((dn + 1.0) / x.v) * vI1, x);
}
__device__ __forceinline__ bool finite3(const Jet3& a) { return isfinite(a.v) && isfinite(a.dw) && isfinite(a.dk); }

template <int FAM>
__global__ __launch_bounds__(64) void root_slopes_kernel(ShootDev P, const double* __restrict__ kv,
                                                         const double* __restrict__ wv, int n,
                                                         const int32_t* __restrict__ d_count, double* __restrict__ outer,
                                                         double* __restrict__ inner, uint8_t* __restrict__ status) {
  constexpr int NB = FamTraits<FAM>::NB;
  constexpr int NE = FamTraits<FAM>::NE;
  const int cnt = es_count_clamped(d_count, n);                // n stays the row length of the [3][n] outputs
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole wave lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < cnt;
  const Jet3 w = {in ? wv[i] : 1.0, 1.0, 0.0};
  const KScalT<Jet3> s = make_kscal(P, Jet3(in ? kv[i] : 1.0, 0.0, 1.0));
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  const ExteriorLiteT<Jet3> X = exterior_lite<FAM>(P, s.k, w, w);
  SignTrack trk;                                               // not tracked: ES_PT_CONTINUUM is not looked at
  double b[NB], cm[NE], c1[NE];                                // node entries: em, e1 depend on k (jets), cm, c1 do not
  Jet3 em[NE], e1[NE];
  CoefT<Jet3> B0;
  load_base<FAM>(P, 2 * nsteps, b);
  make_entry<FAM, fam_scaled<FAM>()>(b, s, e1, c1);
  CoefPreT<Jet3> C0;
  coef_pre<FAM, false>(e1, c1, P, s, w, C0, trk);
  coef_finish<FAM>(C0, rcp(C0.den), B0);                       // first node of the traversal: its own division
  Jet3 zp, zq;
  adjoint_start<FAM>(P, B0, zp, zq);
  for (int j = nsteps - 1; j >= 0; --j) {
    CoefT<Jet3> Bm, B1;
    CoefPreT<Jet3> Cm, C1;
    // coefficients2 spelled out, each node's entries formed right before its coef_pre: 8 and 12 VGPRs less for the cylinders
    load_base<FAM>(P, 2 * j + 1, b);
    make_entry<FAM, fam_scaled<FAM>()>(b, s, em, cm);
    coef_pre<FAM, false>(em, cm, P, s, w, Cm, trk);
    load_base<FAM>(P, 2 * j, b);
    make_entry<FAM, fam_scaled<FAM>()>(b, s, e1, c1);
    coef_pre<FAM, false>(e1, c1, P, s, w, C1, trk);
    const Jet3 inv = fast_rcp(Cm.den * C1.den);
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
  const MismatchT<Jet3> M = boundary_algebra<FAM>(P, s, w, X, zp, zq, e1);
  if (!in) return;
  const bool good = X.status == ES_PT_OK && finite3(M.outer) && finite3(M.inner);
  const Jet3 bad = {NAN, NAN, NAN};
  const Jet3 O = good ? M.outer : bad, J = good ? M.inner : bad;
  if (outer) {
    outer[i] = O.v;
    outer[(size_t)n + i] = O.dw;
    outer[2 * (size_t)n + i] = O.dk;
  }
  if (inner) {
    inner[i] = J.v;
    inner[(size_t)n + i] = J.dw;
    inner[2 * (size_t)n + i] = J.dk;
  }
  if (status) status[i] = (uint8_t)X.status;
}

template <int FAM>
int launch_slopes(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n, const int32_t* d_count,
                  double* d_outer, double* d_inner, uint8_t* d_status) {
  hipLaunchKernelGGL((root_slopes_kernel<FAM>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, d_k, d_w, n, d_count,
                     d_outer, d_inner, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace

extern "C" int es_shoot_root_slopes(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                                    const int32_t* d_count, double* d_outer, double* d_inner, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define ES_SLOPES(F) launch_slopes<F>(ctx, prob, d_k, d_w, n, d_count, d_outer, d_inner, d_status)
  ES_DISPATCH_FAMILY(prob->dev.family, ES_SLOPES)
#undef ES_SLOPES
}
