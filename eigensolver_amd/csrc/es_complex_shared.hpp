// Shared by the complex-frequency translation units (es_complex.hip: values, roots, eigenfunctions; es_complex_slopes.hip:
// slopes and Newton): the complex scalar `cx`, jets of it, the argument check and the complex-frequency evaluation of the
// flow slab (include/eigensolver_amd.h sections 6 and 12; the CPU restatement is oracle/slab_complex.py): closed-form
// exterior, adjoint RK4 on the reference's ix grid with mid-point coefficient sets, far-end condition by superposition.
// Every formula is written once, over jets of W complex components:
//   W = 1   the plain complex value: es_complex.hip (determinant, roots, eigenfunctions)
//   W = 2   value and d/d omega: the Newton steps of es_complex_slopes.hip
//   W = 3   value, d/d omega and d/dk: the slopes
// Tangent-linear (forward mode): omega is the complex variable (w, 1, 0); k is real and enters as the real pair (value,
// d/dk) `rk`.  The value component of every jet operation is one cx operation, the same at every W, and the library is built
// without contraction, so component 0 of a W = 2 or 3 evaluation is the W = 1 result bit for bit.  A one-component jet has no
// derivative arithmetic left once inlined.
//
// One (k, omega) point per lane.  The profile table (U, U', U'' at nodes and mid-points) is staged in LDS chunk by chunk
// (cx_stage_chunk) as in shoot_point; every lane forms its own complex coefficients.  This path is a handful of complex
// divisions per node and is not on the benchmark path: written for clarity, IEEE divisions throughout.
#pragma once
#include "es_shoot_shared.hpp"

namespace es_complex_shared {
using namespace es_shoot_shared;

// ---- the complex scalar ----------------------------------------------------------------------------------------------------
struct cx {
  double re, im;
};
__device__ __forceinline__ cx mk(double a, double b = 0.0) { return cx{a, b}; }
__device__ __forceinline__ cx operator+(cx a, cx b) { return cx{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cx operator-(cx a, cx b) { return cx{a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cx operator-(cx a) { return cx{-a.re, -a.im}; }
__device__ __forceinline__ cx operator*(cx a, cx b) { return cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cx operator*(double s, cx a) { return cx{s * a.re, s * a.im}; }
__device__ __forceinline__ cx operator/(cx a, cx b) {
  const double n = b.re * b.re + b.im * b.im;
  return cx{(a.re * b.re + a.im * b.im) / n, (a.im * b.re - a.re * b.im) / n};
}
__device__ __forceinline__ cx operator-(double s, cx a) { return cx{s - a.re, -a.im}; }
__device__ __forceinline__ cx operator+(double s, cx a) { return cx{s + a.re, a.im}; }
__device__ __forceinline__ double cabs2(cx a) { return a.re * a.re + a.im * a.im; }
__device__ __forceinline__ double cabs_(cx a) { return hypot(a.re, a.im); }
__device__ __forceinline__ bool cfinite(cx a) { return isfinite(a.re) && isfinite(a.im); }
// principal square root (Re >= 0)
__device__ __forceinline__ cx csqrt_(cx z) {
  const double r = hypot(z.re, z.im);
  if (r == 0.0) return cx{0.0, 0.0};
  double a = sqrt(0.5 * (r + fabs(z.re)));
  double b = 0.5 * z.im / a;
  if (z.re >= 0.0) return cx{a, b};
  return cx{fabs(b), copysign(a, z.im)};
}
__device__ __forceinline__ cx cexp_(cx z) {
  const double e = exp(z.re);
  double s, c;
  sincos(z.im, &s, &c);
  return cx{e * c, e * s};
}

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
// a / b: the derivatives (a' - q b') / b share one reciprocal
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
  if constexpr (W >= 2) r.c[1] = -a.c[1];
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
  if constexpr (W >= 2) r.c[1] = s.v * a.c[1];
  if constexpr (W == 3) r.c[2] = s.v * a.c[2] + s.dk * a.c[0];
  return r;
}
template <int W>
__device__ __forceinline__ cj<W> operator/(rk s, const cj<W>& b) {
  cj<W> r;
  r.c[0] = mk(s.v) / b.c[0];
  if constexpr (W >= 2) {
    const cx rb = mk(1.0) / b.c[0];
    r.c[1] = -(r.c[0] * b.c[1]) * rb;
    if constexpr (W == 3) r.c[2] = (mk(s.dk) - r.c[0] * b.c[2]) * rb;
  }
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
  if constexpr (W >= 2) r.c[1] = mk(1.0);
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

// ---- the k-dependent constants of a lane -----------------------------------------------------------------------------------
struct CxConsts {
  double k;
  rk k2, kc2, kvA2, kcT2, k4c;
  double S_i;
  int variant;
};

__device__ __forceinline__ CxConsts cx_consts(const ShootDev& P, int variant, double k) {
  CxConsts C;
  const double k2 = k * k;
  C.k = k;
  C.k2 = rk{k2, 2.0 * k};
  C.kc2 = rk{k2 * P.c2_i, 2.0 * k * P.c2_i};
  C.kvA2 = rk{k2 * P.vA2_i, 2.0 * k * P.vA2_i};
  C.kcT2 = rk{k2 * P.cT2_i, 2.0 * k * P.cT2_i};
  C.k4c = rk{k2 * k2 * P.cT2_i * P.c2_i, 4.0 * k * k2 * P.cT2_i * P.c2_i};
  C.S_i = P.S_i;
  C.variant = variant;
  return C;
}

// ---- interior --------------------------------------------------------------------------------------------------------------
// coefficients at one node: u' = v, v' = a21 u + a22 v  with  a21 = -coeff, a22 = -D
template <int W>
struct CxNode {
  cj<W> a21, a22;
};

template <int W>
__device__ __forceinline__ void cx_terms(const CxConsts& C, cx w, double U, double dU, cj<W>& Om, cj<W>& Om2, cj<W>& m0, cj<W>& D) {
  Om = doppler<W>(w, C.k, U);
  Om2 = Om * Om;
  const cj<W> n1 = C.kc2 - Om2, n3 = C.kvA2 - Om2, nT = C.kcT2 - Om2;
  m0 = (n1 * n3) / (C.S_i * nT);                                                     // SF-X:375
  const rk kdU2 = rk{2.0 * C.k * dU, 2.0 * dU};
  if (C.variant == ES_CX_SFX) {
    D = kdU2 * ((Om2 / (Om2 - C.kc2) - C.kcT2 / (Om2 - C.kcT2)) / Om);               // SF-X:382
  } else {
    const cj<W> t = Om2 - C.kcT2;
    D = kdU2 * ((t + C.k4c / (C.S_i * t)) / (Om * (Om2 - C.kc2)));                   // SF-G:421 as written
  }
}

template <int W>
__device__ __forceinline__ CxNode<W> cx_coef(const CxConsts& C, cx w, double U, double dU, double ddU) {
  cj<W> Om, Om2, m0, D;
  cx_terms<W>(C, w, U, dU, Om, Om2, m0, D);
  const cj<W> coeff = rk{C.k * ddU, ddU} / Om + rk{C.k * dU, dU} * (D / Om) - m0;    // SF-X:389
  return CxNode<W>{-coeff, -D};
}

// rhs of the transposed system: A^T z with A = [[0, 1], [a21, a22]]
template <int W>
__device__ __forceinline__ void cx_rhs(const CxNode<W>& A, const cj<W>& p, const cj<W>& q, cj<W>& kp, cj<W>& kq) {
  kp = A.a21 * q;
  kq = p + A.a22 * q;
}

// total pressure of the interior state (u, v) = (Vx, Vx') at a node with Omega = Om: P_Ti (v - add u), SF-X:395, :401, :455
template <int W>
__device__ __forceinline__ cj<W> cx_total_pressure(const ShootDev& P, const CxConsts& C, const cj<W>& Om, const cj<W>& Om2,
                                                   double dU, const cj<W>& u, const cj<W>& v) {
  const cj<W> PTi = (P.rho_i * P.S_i) * ((C.kcT2 - Om2) / (Om * (C.kc2 - Om2)));     // SF-X:395
  if (C.variant != ES_CX_SFX) return PTi * v;                                        // add = 0
  const cj<W> add = -(rk{C.k * dU, dU} / Om);                                        // SF-X:401
  return PTi * (v - add * u);
}

// ---- exterior (closed form, decaying branch), SF-X:369-371, :419-426:  Vx_e ~ gp e^{mu (x + R)} + gm e^{-mu (x + R)} --------
template <int W>
struct CxOutside {
  cj<W> Oe, p_e, mu, gp, gm, E2;   // E2 = e^{-2 mu (R - 1)}
  cj<W> outer;                     // p_e V_e'(-1) / V_e(-1)
  double R;
  int status;
};

template <int W>
__device__ __forceinline__ CxOutside<W> cx_exterior(const ShootDev& P, const CxConsts& C, double k, cx w) {
  CxOutside<W> X;
  X.Oe = doppler<W>(w, k, P.U_e);
  const cj<W> Oe2 = X.Oe * X.Oe;
  const cj<W> m_e = ((C.k2 * P.vAe2 - Oe2) * (C.k2 * P.ce2 - Oe2)) / (P.Se * (C.k2 * P.cTe2 - Oe2));
  X.p_e = (P.rho_e * P.Se) * ((C.k2 * P.cTe2 - Oe2) / (X.Oe * (C.k2 * P.ce2 - Oe2)));
  X.status = ES_PT_OK;
  if (m_e.c[0].re < 0.0) X.status = ES_PT_LEAKY;                                      // `if m_e.real < 0: pass`
  X.mu = jsqrt(m_e);
  X.R = P.R_factor / k;
  const rk m2R1 = rk{-2.0 * (X.R - 1.0), 2.0 * X.R / k};      // -2 (R - 1), R = R_factor / k
  X.E2 = jexp(m2R1 * X.mu);
  const cj<W> gq = rk{P.ic1, 0.0} / X.mu;
  X.gp = P.ic0 + gq; X.gm = P.ic0 - gq;
  const cj<W> y = X.mu * ((X.gp - X.E2 * X.gm) / (X.gp + X.E2 * X.gm));
  X.outer = X.p_e * y;
  if (X.status == ES_PT_OK && !cfinite(X.outer.c[0])) X.status = ES_PT_NONFINITE;
  return X;
}

// ---- the marches -----------------------------------------------------------------------------------------------------------
constexpr int CX_NB = 3;                                      // U, U', U'' per point of the table
constexpr int CX_LDS_DOUBLES = CX_NB * (2 * CH + 1);         // one chunk: nodes and mid-points of CH steps

// Copies the table of the nst steps from step c0 on (2 nst + 1 points, point-major) into the LDS buffer `sb`, between two
// barriers: every lane of the workgroup reaches every barrier, so every lane of a workgroup must make every call, in the
// same order (lanes past the count march on dummy inputs and store nothing).
__device__ __forceinline__ void cx_stage_chunk(const ShootDev& P, int c0, int nst, double* __restrict__ sb) {
  __syncthreads();
#pragma unroll
  for (int f = 0; f < CX_NB; ++f)
    for (int i = threadIdx.x; i < 2 * nst + 1; i += blockDim.x) sb[i * CX_NB + f] = P.base[(size_t)f * P.npts + 2 * c0 + i];
  __syncthreads();
}

// adjoint march of the functional Vx(+1) = (1, 0) . (u, v) from x = +1 back to x = -1: Vx(+1) = zp u(-1) + zq v(-1).
// Ub, dUb: the profile at the boundary node.  Every lane of the workgroup must call this (barriers of the staging).
template <int W>
__device__ __forceinline__ void cx_adjoint(const ShootDev& P, const CxConsts& C, cx w, double* __restrict__ sb, cj<W>& zp,
                                           cj<W>& zq, double& Ub, double& dUb) {
  constexpr int NB = CX_NB;
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  zp = jconst<W>(1.0); zq = jconst<W>(0.0);
  CxNode<W> B0{jconst<W>(0.0), jconst<W>(0.0)};
  Ub = 0.0; dUb = 0.0;
  const int nchunks = (nsteps + CH - 1) / CH;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int c0 = c * CH;
    const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
    cx_stage_chunk(P, c0, nst, sb);
    if (c == nchunks - 1) B0 = cx_coef<W>(C, w, sb[2 * nst * NB + SF_U], sb[2 * nst * NB + SF_DU], sb[2 * nst * NB + SF_DDU]);
    for (int j = nst - 1; j >= 0; --j) {
      const double* bm = sb + (2 * j + 1) * NB;
      const double* b1 = sb + (2 * j) * NB;
      cj<W> kp, kq, sp, sq;                                   // one stage at a time; sp, sq collect h/6 (k1 + k4) + h/3 (k2 + k3)
      cx_rhs(B0, zp, zq, kp, kq);
      cj<W> ap = kp, aq = kq;                                 // k1 + k4
      const CxNode<W> Bm = cx_coef<W>(C, w, bm[SF_U], bm[SF_DU], bm[SF_DDU]);
      cx_rhs(Bm, zp + h2 * kp, zq + h2 * kq, sp, sq);         // k2
      cx_rhs(Bm, zp + h2 * sp, zq + h2 * sq, kp, kq);         // k3
      sp = sp + kp; sq = sq + kq;                             // k2 + k3
      B0 = cx_coef<W>(C, w, b1[SF_U], b1[SF_DU], b1[SF_DDU]);
      cj<W> k4p, k4q;
      cx_rhs(B0, zp + h * kp, zq + h * kq, k4p, k4q);
      ap = ap + k4p; aq = aq + k4q;
      zp = zp + h6 * ap + h3 * sp;
      zq = zq + h6 * aq + h3 * sq;
      if (c == 0 && j == 0) { Ub = b1[SF_U]; dUb = b1[SF_DU]; }
    }
  }
}

// ---- boundary: continuity of the displacement, symmetry condition by superposition, total pressures (SF-X:422, :455) --------
template <int W>
struct CxMatch {
  cj<W> Vb, sv;        // interior state at x = -1 per unit V_e(-1): Vx, Vx'
  cj<W> outer, inner;  // the two sides of the matching condition; D_c = outer - inner
  double rel;          // |D_c| in percent of the larger side, NaN unless st == ES_PT_OK
  uint8_t st;
};

template <int W>
__device__ __forceinline__ CxMatch<W> cx_boundary(const ShootDev& P, const CxConsts& C, const CxOutside<W>& X, cx w,
                                                      const cj<W>& zp, const cj<W>& zq, double Ub, double dUb) {
  CxMatch<W> B;
  const cj<W> Omb = doppler<W>(w, C.k, Ub);
  B.Vb = Omb / X.Oe;
  B.sv = ((P.slab_sign - zp) * B.Vb) / zq;
  B.outer = X.outer;
  B.inner = cx_total_pressure<W>(P, C, Omb, Omb * Omb, dUb, B.Vb, B.sv);
  const cx d = B.outer.c[0] - B.inner.c[0];
  B.st = (uint8_t)X.status;
  B.rel = cabs_(d) * 100.0 / fmax(cabs_(B.outer.c[0]), cabs_(B.inner.c[0]));
  if (X.status != ES_PT_OK) B.rel = NAN;
  else if (!cfinite(d)) { B.st = ES_PT_NONFINITE; B.rel = NAN; }
  return B;
}

// one evaluation at (k, w): exterior, adjoint march, boundary.  Every lane of the workgroup must call this.
template <int W>
__device__ __forceinline__ CxMatch<W> cx_eval(const ShootDev& P, int variant, double k, cx w, double* __restrict__ sb) {
  const CxConsts C = cx_consts(P, variant, k);
  const CxOutside<W> X = cx_exterior<W>(P, C, k, w);
  cj<W> zp, zq;
  double Ub, dUb;
  cx_adjoint<W>(P, C, w, sb, zp, zq, Ub, dUb);
  return cx_boundary<W>(P, C, X, w, zp, zq, Ub, dUb);
}

// ---- host: the argument check of every entry point -------------------------------------------------------------------------
inline int check_cx(es_context* ctx, const es_problem* prob, int variant) {
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, variant == ES_CX_SFX || variant == ES_CX_SFG, "variant");
  if (prob->dev.family != FAM_SLABF) {
    ctx->last_error = "complex frequencies are implemented for ES_GEOM_SLAB_FLOW problems only";
    return ES_ERR_UNSUPPORTED;
  }
  return ES_SUCCESS;
}

}  // namespace es_complex_shared
