// Slopes and Newton tracing of complex roots of the flow slab (include/eigensolver_amd.h section 12): the two sides of the
// matching condition of es_complex_eval_points, outer and inner, with their exact derivatives in omega (holomorphic) and k.
// Tangent-linear (forward-mode) evaluation: cx_terms / cx_coef, the adjoint RK4 march, cx_exterior and cx_boundary of
// es_complex.hip restated, formula for formula, over jets of W complex components (value, d/d omega and, for W = 3, d/dk).
// omega is the complex variable (w, 1, 0); k is real and enters as the real pair (value, d/dk) `rk`.  The value component of
// every jet operation is the cx operation the value path takes, in the same order.
//
// One (k, omega) pair per lane, 64-thread workgroups, the profile table staged chunk by chunk in LDS as cx_adjoint does:
// every lane of a workgroup reaches every barrier.  Lanes past the count march on dummy inputs and store nothing.
#include "es_complex_shared.hpp"

namespace {
using namespace es_complex_shared;

// ---- jets ------------------------------------------------------------------------------------------------------------------
template <int W>
struct cj {
  cx c[W];                           // c[0] value, c[1] d/d omega, c[2] d/dk
};
struct rk {
  double v, dk;                      // a real function of k
};

template <int W>
__device__ __forceinline__ cj<W> operator+(const cj<W>& a, const cj<W>& b) {
  cj<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i) r.c[i] = a.c[i] + b.c[i];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator-(const cj<W>& a, const cj<W>& b) {
  cj<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i) r.c[i] = a.c[i] - b.c[i];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator-(const cj<W>& a) {
  cj<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i) r.c[i] = -a.c[i];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator*(const cj<W>& a, const cj<W>& b) {
  cj<W> r;
  r.c[0] = a.c[0] * b.c[0];
#pragma unroll
  for (int i = 1; i < W; ++i) r.c[i] = a.c[0] * b.c[i] + a.c[i] * b.c[0];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator*(double s, const cj<W>& a) {
  cj<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i) r.c[i] = s * a.c[i];
  return r;
}
// a / b: the value is the quotient of the value path, the derivatives (a' - q b') / b share one reciprocal
template <int W>
__device__ __forceinline__ cj<W> operator/(const cj<W>& a, const cj<W>& b) {
  cj<W> r;
  r.c[0] = a.c[0] / b.c[0];
  const cx rb = mk(1.0) / b.c[0];
#pragma unroll
  for (int i = 1; i < W; ++i) r.c[i] = (a.c[i] - r.c[0] * b.c[i]) * rb;
  return r;
}
// real functions of k against jets
template <int W>
__device__ __forceinline__ cj<W> operator-(rk s, const cj<W>& a) {
  cj<W> r;
  r.c[0] = s.v - a.c[0];
  r.c[1] = -a.c[1];
  if constexpr (W == 3) r.c[2] = s.dk - a.c[2];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator-(const cj<W>& a, rk s) {
  cj<W> r = a;
  r.c[0] = a.c[0] - mk(s.v);
  if constexpr (W == 3) r.c[2] = a.c[2] - mk(s.dk);
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator+(double s, const cj<W>& a) {
  cj<W> r = a;
  r.c[0] = s + a.c[0];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator-(double s, const cj<W>& a) {
  cj<W> r = -a;
  r.c[0] = s - a.c[0];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator*(rk s, const cj<W>& a) {
  cj<W> r;
  r.c[0] = s.v * a.c[0];
  r.c[1] = s.v * a.c[1];
  if constexpr (W == 3) r.c[2] = s.v * a.c[2] + s.dk * a.c[0];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator/(rk s, const cj<W>& b) {
  cj<W> r;
  r.c[0] = mk(s.v) / b.c[0];
  const cx rb = mk(1.0) / b.c[0];
  r.c[1] = -(r.c[0] * b.c[1]) * rb;
  if constexpr (W == 3) r.c[2] = (mk(s.dk) - r.c[0] * b.c[2]) * rb;
  return r;
}
__device__ __forceinline__ rk operator*(rk a, double s) { return rk{a.v * s, a.dk * s}; }
__device__ __forceinline__ rk operator*(double s, rk a) { return rk{s * a.v, s * a.dk}; }
template <int W>
__device__ __forceinline__ cj<W> jsqrt(const cj<W>& a) {
  cj<W> r;
  r.c[0] = csqrt_(a.c[0]);
  const cx h = mk(0.5) / r.c[0];
#pragma unroll
  for (int i = 1; i < W; ++i) r.c[i] = a.c[i] * h;
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> jexp(const cj<W>& a) {
  cj<W> r;
  r.c[0] = cexp_(a.c[0]);
#pragma unroll
  for (int i = 1; i < W; ++i) r.c[i] = r.c[0] * a.c[i];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> jconst(double v) {
  cj<W> r;
  r.c[0] = mk(v);
#pragma unroll
  for (int i = 1; i < W; ++i) r.c[i] = mk(0.0);
  return r;
}
// omega - k U for a real constant U: (w - k U, 1, -U)
template <int W>
__device__ __forceinline__ cj<W> doppler(cx w, double k, double U) {
  cj<W> r;
  r.c[0] = w - mk(k * U);
  r.c[1] = mk(1.0);
  if constexpr (W == 3) r.c[2] = mk(-U);
  return r;
}
template <int W>
__device__ __forceinline__ bool jfinite(const cj<W>& a) {
  bool f = true;
#pragma unroll
  for (int i = 0; i < W; ++i) f = f && cfinite(a.c[i]);
  return f;
}

// ---- the formulas of es_complex.hip over jets ------------------------------------------------------------------------------
struct KJ {                          // CxConsts with d/dk
  double k;
  rk k2, kc2, kvA2, kcT2, k4c;
  double S_i;
  int variant;
};

__device__ __forceinline__ KJ kj_consts(const ShootDev& P, int variant, double k) {
  const CxConsts C = cx_consts(P, variant, k);
  KJ J;
  J.k = k;
  J.k2 = rk{C.k2, 2.0 * k};
  J.kc2 = rk{C.kc2, 2.0 * k * P.c2_i};
  J.kvA2 = rk{C.kvA2, 2.0 * k * P.vA2_i};
  J.kcT2 = rk{C.kcT2, 2.0 * k * P.cT2_i};
  J.k4c = rk{C.k4c, 4.0 * k * C.k2 * P.cT2_i * P.c2_i};
  J.S_i = C.S_i;
  J.variant = variant;
  return J;
}

template <int W>
struct CoefJ {
  cj<W> a21, a22;
};

template <int W>
__device__ __forceinline__ void cxj_terms(const KJ& C, cx w, double U, double dU, cj<W>& Om, cj<W>& Om2, cj<W>& m0, cj<W>& D) {
  Om = doppler<W>(w, C.k, U);
  Om2 = Om * Om;
  const cj<W> n1 = C.kc2 - Om2, n3 = C.kvA2 - Om2, nT = C.kcT2 - Om2;
  m0 = (n1 * n3) / (C.S_i * nT);
  const rk kdU2 = rk{2.0 * C.k * dU, 2.0 * dU};
  if (C.variant == ES_CX_SFX) {
    D = kdU2 * ((Om2 / (Om2 - C.kc2) - C.kcT2 / (Om2 - C.kcT2)) / Om);
  } else {
    const cj<W> t = Om2 - C.kcT2;
    D = kdU2 * ((t + C.k4c / (C.S_i * t)) / (Om * (Om2 - C.kc2)));
  }
}

template <int W>
__device__ __forceinline__ CoefJ<W> cxj_coef(const KJ& C, cx w, double U, double dU, double ddU) {
  cj<W> Om, Om2, m0, D;
  cxj_terms<W>(C, w, U, dU, Om, Om2, m0, D);
  const cj<W> coeff = rk{C.k * ddU, ddU} / Om + rk{C.k * dU, dU} * (D / Om) - m0;
  return CoefJ<W>{-coeff, -D};
}

template <int W>
__device__ __forceinline__ void cxj_rhs(const CoefJ<W>& A, const cj<W>& p, const cj<W>& q, cj<W>& kp, cj<W>& kq) {
  kp = A.a21 * q;
  kq = p + A.a22 * q;
}

template <int W>
struct ExtJ {
  cj<W> Oe, outer;
  int status;
};

template <int W>
__device__ __forceinline__ ExtJ<W> cxj_exterior(const ShootDev& P, const KJ& C, double k, cx w) {
  ExtJ<W> X;
  X.Oe = doppler<W>(w, k, P.U_e);
  const cj<W> Oe2 = X.Oe * X.Oe;
  const cj<W> m_e = ((C.k2 * P.vAe2 - Oe2) * (C.k2 * P.ce2 - Oe2)) / (P.Se * (C.k2 * P.cTe2 - Oe2));
  const cj<W> p_e = (P.rho_e * P.Se) * ((C.k2 * P.cTe2 - Oe2) / (X.Oe * (C.k2 * P.ce2 - Oe2)));
  X.status = ES_PT_OK;
  if (m_e.c[0].re < 0.0) X.status = ES_PT_LEAKY;
  const cj<W> mu = jsqrt(m_e);
  const double R = P.R_factor / k;
  const rk m2R1 = rk{-2.0 * (R - 1.0), 2.0 * R / k};          // -2 (R - 1), R = R_factor / k
  const cj<W> E2 = jexp(m2R1 * mu);
  const cj<W> gq = rk{P.ic1, 0.0} / mu;
  const cj<W> gp = P.ic0 + gq, gm = P.ic0 - gq;
  const cj<W> y = mu * ((gp - E2 * gm) / (gp + E2 * gm));
  X.outer = p_e * y;
  if (X.status == ES_PT_OK && !cfinite(X.outer.c[0])) X.status = ES_PT_NONFINITE;
  return X;
}

// cx_adjoint over jets.  Every lane of the workgroup must call this (barriers of the staging).
template <int W>
__device__ __forceinline__ void cxj_adjoint(const ShootDev& P, const KJ& C, cx w, double* __restrict__ sb, cj<W>& zp, cj<W>& zq,
                                            double& Ub, double& dUb) {
  constexpr int NB = 3;
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  zp = jconst<W>(1.0); zq = jconst<W>(0.0);
  CoefJ<W> B0{jconst<W>(0.0), jconst<W>(0.0)};
  Ub = 0.0; dUb = 0.0;
  const int nchunks = (nsteps + CH - 1) / CH;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int c0 = c * CH;
    const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NB; ++f)
      for (int i = threadIdx.x; i < 2 * nst + 1; i += blockDim.x) sb[i * NB + f] = P.base[(size_t)f * P.npts + 2 * c0 + i];
    __syncthreads();
    if (c == nchunks - 1) B0 = cxj_coef<W>(C, w, sb[2 * nst * NB + SF_U], sb[2 * nst * NB + SF_DU], sb[2 * nst * NB + SF_DDU]);
    for (int j = nst - 1; j >= 0; --j) {
      const double* bm = sb + (2 * j + 1) * NB;
      const double* b1 = sb + (2 * j) * NB;
      cj<W> kp, kq, sp, sq;                                   // one stage at a time; sp, sq collect h/6 (k1 + k4) + h/3 (k2 + k3)
      cxj_rhs(B0, zp, zq, kp, kq);
      cj<W> ap = kp, aq = kq;                                 // k1 + k4
      const CoefJ<W> Bm = cxj_coef<W>(C, w, bm[SF_U], bm[SF_DU], bm[SF_DDU]);
      cxj_rhs(Bm, zp + h2 * kp, zq + h2 * kq, sp, sq);        // k2
      cxj_rhs(Bm, zp + h2 * sp, zq + h2 * sq, kp, kq);        // k3
      sp = sp + kp; sq = sq + kq;                             // k2 + k3
      B0 = cxj_coef<W>(C, w, b1[SF_U], b1[SF_DU], b1[SF_DDU]);
      cj<W> k4p, k4q;
      cxj_rhs(B0, zp + h * kp, zq + h * kq, k4p, k4q);
      ap = ap + k4p; aq = aq + k4q;
      zp = zp + h6 * ap + h3 * sp;
      zq = zq + h6 * aq + h3 * sq;
      if (c == 0 && j == 0) { Ub = b1[SF_U]; dUb = b1[SF_DU]; }
    }
  }
}

// one evaluation: both sides of the matching condition as jets, the status and rel of cx_boundary
template <int W>
struct EvalJ {
  cj<W> outer, inner;
  double rel;
  uint8_t st;
};

template <int W>
__device__ __forceinline__ EvalJ<W> cxj_eval(const ShootDev& P, int variant, double k, cx w, double* __restrict__ sb) {
  const KJ C = kj_consts(P, variant, k);
  const ExtJ<W> X = cxj_exterior<W>(P, C, k, w);
  cj<W> zp, zq;
  double Ub, dUb;
  cxj_adjoint<W>(P, C, w, sb, zp, zq, Ub, dUb);
  // cx_boundary
  const cj<W> Omb = doppler<W>(w, k, Ub);
  const cj<W> Omb2 = Omb * Omb;
  const cj<W> Vb = Omb / X.Oe;
  const cj<W> sv = ((P.slab_sign - zp) * Vb) / zq;
  const cj<W> PTi = (P.rho_i * P.S_i) * ((C.kcT2 - Omb2) / (Omb * (C.kc2 - Omb2)));
  EvalJ<W> E;
  E.outer = X.outer;
  if (variant == ES_CX_SFX) {
    const cj<W> add = -(rk{k * dUb, dUb} / Omb);
    E.inner = PTi * (sv - add * Vb);
  } else {
    E.inner = PTi * sv;                                       // add = 0
  }
  const cx d = E.outer.c[0] - E.inner.c[0];
  E.st = (uint8_t)X.status;
  E.rel = cabs_(d) * 100.0 / fmax(cabs_(E.outer.c[0]), cabs_(E.inner.c[0]));
  if (X.status != ES_PT_OK) E.rel = NAN;
  else if (!cfinite(d)) { E.st = ES_PT_NONFINITE; E.rel = NAN; }
  return E;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cx_slopes_kernel(ShootDev P, int variant, const double* __restrict__ kv,
                                                       const double* __restrict__ wre, const double* __restrict__ wim, int n,
                                                       const int32_t* __restrict__ d_count, double* __restrict__ outer,
                                                       double* __restrict__ inner, uint8_t* __restrict__ status) {
  __shared__ double sb[3 * (2 * CH + 1)];
  const int cnt = es_count_clamped(d_count, n);                // n stays the row length of the [3][n][2] outputs
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole workgroup lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < cnt;
  const double k = in ? kv[i] : 1.0;
  const cx w = in ? cx{wre[i], wim[i]} : cx{1.0, 0.1};
  const EvalJ<3> E = cxj_eval<3>(P, variant, k, w, sb);
  if (!in) return;
  const bool good = E.st == ES_PT_OK && jfinite(E.outer) && jfinite(E.inner);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t o = 2 * ((size_t)c * n + i);
    if (outer) {
      outer[o] = good ? E.outer.c[c].re : NAN;
      outer[o + 1] = good ? E.outer.c[c].im : NAN;
    }
    if (inner) {
      inner[o] = good ? E.inner.c[c].re : NAN;
      inner[o + 1] = good ? E.inner.c[c].im : NAN;
    }
  }
  if (status) status[i] = E.st;
}

// Newton in omega at fixed k, one guess per lane.  A lane that has stopped keeps evaluating at its frozen omega (the staging
// barriers need all 64 lanes); the workgroup leaves the loop together once no lane is active.
__global__ __launch_bounds__(64) void cx_newton_kernel(ShootDev P, int variant, const double* __restrict__ kv,
                                                       const double* __restrict__ gre, const double* __restrict__ gim, int n,
                                                       const int32_t* __restrict__ d_count, int max_iter, double step_cap,
                                                       double max_shift, double tol_percent, double* __restrict__ wre,
                                                       double* __restrict__ wim, double* __restrict__ resid,
                                                       double* __restrict__ dwdk, int32_t* __restrict__ iters_out,
                                                       int32_t* __restrict__ flag_out) {
  __shared__ double sb[3 * (2 * CH + 1)];
  const int cnt = es_count_clamped(d_count, n);
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole workgroup lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < cnt;
  const double k = in ? kv[i] : 1.0;
  const cx guess = in ? cx{gre[i], gim[i]} : cx{1.0, 0.1};
  cx w = guess;
  int iters = 0;
  bool ok = true, active = in;
  for (int it = 0; it < max_iter; ++it) {                      // max_iter is uniform: every lane reaches the vote
    const EvalJ<2> E = cxj_eval<2>(P, variant, k, w, sb);
    if (active) {
      const cx D = E.outer.c[0] - E.inner.c[0], Dw = E.outer.c[1] - E.inner.c[1];
      if (E.st != ES_PT_OK || !cfinite(D) || !cfinite(Dw) || (Dw.re == 0.0 && Dw.im == 0.0)) {
        ok = false;
        active = false;
      } else {
        cx s = -(D / Dw);
        const double a = cabs_(s);
        if (a > step_cap) s = (step_cap / a) * s;
        w = w + s;
        ++iters;
        if (cabs_(s) <= 1e-14 * fmax(1.0, cabs_(w))) active = false;
      }
    }
    if (!__syncthreads_or(active ? 1 : 0)) break;
  }
  const EvalJ<3> E = cxj_eval<3>(P, variant, k, w, sb);
  if (!in) return;
  const cx Dw = E.outer.c[1] - E.inner.c[1], Dk = E.outer.c[2] - E.inner.c[2];
  const bool good = E.st == ES_PT_OK;
  const cx slope = good ? -(Dk / Dw) : cx{NAN, NAN};
  wre[i] = w.re;
  wim[i] = w.im;
  resid[i] = E.rel;
  if (dwdk) {
    dwdk[2 * (size_t)i] = slope.re;
    dwdk[2 * (size_t)i + 1] = slope.im;
  }
  iters_out[i] = iters;
  flag_out[i] = (ok && good && E.rel < tol_percent && cabs_(w - guess) <= max_shift) ? 1 : 0;
}

}  // namespace

extern "C" int es_complex_root_slopes(es_context* ctx, const es_problem* prob, int variant, const double* d_k,
                                      const double* d_w_re, const double* d_w_im, int n, const int32_t* d_count,
                                      double* d_outer, double* d_inner, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cx(ctx, prob, variant);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cx_slopes_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, variant, d_k, d_w_re,
                     d_w_im, n, d_count, d_outer, d_inner, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_complex_newton(es_context* ctx, const es_problem* prob, int variant, const double* d_k,
                                 const double* d_guess_re, const double* d_guess_im, int n, const int32_t* d_count,
                                 int max_iter, double step_cap, double max_shift, double tol_percent, double* d_w_re,
                                 double* d_w_im, double* d_resid, double* d_dwdk, int32_t* d_iters, int32_t* d_flag) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cx(ctx, prob, variant);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  ES_REQUIRE(ctx, max_iter >= 0, "max_iter");
  ES_REQUIRE(ctx, step_cap > 0.0 && max_shift > 0.0 && tol_percent > 0.0, "step_cap, max_shift and tol_percent must be positive");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_guess_re && d_guess_im && d_w_re && d_w_im && d_resid && d_iters && d_flag, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cx_newton_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, variant, d_k, d_guess_re,
                     d_guess_im, n, d_count, max_iter, step_cap, max_shift, tol_percent, d_w_re, d_w_im, d_resid, d_dwdk,
                     d_iters, d_flag);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
