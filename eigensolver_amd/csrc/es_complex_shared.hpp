// Shared by the complex-frequency translation units (es_complex.hip: values, roots, eigenfunctions; es_complex_slopes.hip:
// slopes and Newton): the argument check and the complex-frequency evaluation of the flow slab (include/eigensolver_amd.h
// sections 6 and 12; the CPU restatement is oracle/slab_complex.py): closed-form exterior, adjoint RK4 on the reference's ix
// grid with mid-point coefficient sets, far-end condition by superposition.
// Every formula is written once, over the scalar Z and the wavenumber type K, as the cylinder's text is
// (es_cyl_complex_shared.hpp); the scalars are the library's one complex scalar and one complex jet (es_cjet.hpp):
//   Z = esb::cz        K = double   the plain complex value: es_complex.hip (determinant, roots, eigenfunctions)
//   Z = esb::CJet<1>   K = double   value and d/d omega: the Newton steps of es_complex_slopes.hip
//   Z = esb::CJet<2>   K = RealK    value, d/d omega and d/dk: the slopes
// Tangent-linear (forward mode): omega is the complex variable (w, 1, 0); k is real, a constant where K is double and the
// variable (k, d/dk = 1) where it is esb::RealK, the real pair (value, d/dk).  What the text knows as a real function of k
// with its k-derivative -- k^2 c^2, k U', -2 (R - 1) -- it hands over through real_of_k, derivative as written here.  The
// value component of every jet operation is the cz operation of the plain path and the library is built without
// contraction: the value of a jet evaluation is the cz result bit for bit.
//
// One (k, omega) point per lane.  The profile table (U, U', U'' at nodes and mid-points) is staged in LDS chunk by chunk
// (cx_stage_chunk) as in shoot_point; every lane forms its own complex coefficients.  This path is a handful of complex
// divisions per node and is not on the benchmark path: written for clarity, IEEE divisions throughout.
#pragma once
#include "es_cjet.hpp"
#include "es_shoot_shared.hpp"

namespace es_complex_shared {
using namespace es_shoot_shared;
using esb::cz;
using esb::cz_abs;
using esb::cz_abs2;
using esb::cz_finite;
using esb::real_of_k;

// ---- the k-dependent constants of a lane -----------------------------------------------------------------------------------
template <class K>
struct CxConsts {
  double k;                          // the value
  K kj;                              // k as the differentiation sees it
  K k2, kc2, kvA2, kcT2, k4c;
  double S_i;
  int variant;
};

template <class K>
__device__ __forceinline__ CxConsts<K> cx_consts(const ShootDev& P, int variant, const K& kj) {
  CxConsts<K> C;
  const double k = val(kj), k2 = k * k;
  C.k = k;
  C.kj = kj;
  C.k2 = real_of_k(kj, k2, 2.0 * k);
  C.kc2 = real_of_k(kj, k2 * P.c2_i, 2.0 * k * P.c2_i);
  C.kvA2 = real_of_k(kj, k2 * P.vA2_i, 2.0 * k * P.vA2_i);
  C.kcT2 = real_of_k(kj, k2 * P.cT2_i, 2.0 * k * P.cT2_i);
  C.k4c = real_of_k(kj, k2 * k2 * P.cT2_i * P.c2_i, 4.0 * k * k2 * P.cT2_i * P.c2_i);
  C.S_i = P.S_i;
  C.variant = variant;
  return C;
}

// ---- interior --------------------------------------------------------------------------------------------------------------
// coefficients at one node: u' = v, v' = a21 u + a22 v  with  a21 = -coeff, a22 = -D
template <class Z>
struct CxNode {
  Z a21, a22;
};

// A real function of k over a complex quantity is taken as the complex quotient of re + 0 i: Z(.) / x.
template <class Z, class K>
__device__ __forceinline__ void cx_terms(const CxConsts<K>& C, const Z& w, double U, double dU, Z& Om, Z& Om2, Z& m0, Z& D) {
  Om = w - C.kj * U;                                                                 // omega - k U
  Om2 = Om * Om;
  const Z n1 = C.kc2 - Om2, n3 = C.kvA2 - Om2, nT = C.kcT2 - Om2;
  m0 = (n1 * n3) / (C.S_i * nT);                                                     // SF-X:375
  const K kdU2 = real_of_k(C.kj, 2.0 * C.k * dU, 2.0 * dU);
  if (C.variant == ES_CX_SFX) {
    D = kdU2 * ((Om2 / (Om2 - C.kc2) - Z(C.kcT2) / (Om2 - C.kcT2)) / Om);            // SF-X:382
  } else {
    const Z t = Om2 - C.kcT2;
    D = kdU2 * ((t + Z(C.k4c) / (C.S_i * t)) / (Om * (Om2 - C.kc2)));                // SF-G:421 as written
  }
}

template <class Z, class K>
__device__ __forceinline__ CxNode<Z> cx_coef(const CxConsts<K>& C, const Z& w, double U, double dU, double ddU) {
  Z Om, Om2, m0, D;
  cx_terms(C, w, U, dU, Om, Om2, m0, D);
  const K kdU = real_of_k(C.kj, C.k * dU, dU);
  const Z coeff = Z(real_of_k(C.kj, C.k * ddU, ddU)) / Om + kdU * (D / Om) - m0;     // SF-X:389
  return CxNode<Z>{-coeff, -D};
}

// rhs of the transposed system: A^T z with A = [[0, 1], [a21, a22]]
template <class Z>
__device__ __forceinline__ void cx_rhs(const CxNode<Z>& A, const Z& p, const Z& q, Z& kp, Z& kq) {
  kp = A.a21 * q;
  kq = p + A.a22 * q;
}

// total pressure of the interior state (u, v) = (Vx, Vx') at a node with Omega = Om: P_Ti (v - add u), SF-X:395, :401, :455
template <class Z, class K>
__device__ __forceinline__ Z cx_total_pressure(const ShootDev& P, const CxConsts<K>& C, const Z& Om, const Z& Om2, double dU,
                                               const Z& u, const Z& v) {
  const Z PTi = (P.rho_i * P.S_i) * ((C.kcT2 - Om2) / (Om * (C.kc2 - Om2)));         // SF-X:395
  if (C.variant != ES_CX_SFX) return PTi * v;                                        // add = 0
  const Z add = -(Z(real_of_k(C.kj, C.k * dU, dU)) / Om);                            // SF-X:401
  return PTi * (v - add * u);
}

// ---- exterior (closed form, decaying branch), SF-X:369-371, :419-426:  Vx_e ~ gp e^{mu (x + R)} + gm e^{-mu (x + R)} --------
template <class Z>
struct CxOutside {
  Z Oe, p_e, mu, gp, gm, E2;       // E2 = e^{-2 mu (R - 1)}
  Z outer;                         // p_e V_e'(-1) / V_e(-1)
  double R;
  int status;
};

template <class Z, class K>
__device__ __forceinline__ CxOutside<Z> cx_exterior(const ShootDev& P, const CxConsts<K>& C, const Z& w) {
  CxOutside<Z> X;
  const double k = C.k;
  X.Oe = w - C.kj * P.U_e;
  const Z Oe2 = X.Oe * X.Oe;
  const Z m_e = ((C.k2 * P.vAe2 - Oe2) * (C.k2 * P.ce2 - Oe2)) / (P.Se * (C.k2 * P.cTe2 - Oe2));
  X.p_e = (P.rho_e * P.Se) * ((C.k2 * P.cTe2 - Oe2) / (X.Oe * (C.k2 * P.ce2 - Oe2)));
  X.status = ES_PT_OK;
  if (val(m_e) < 0.0) X.status = ES_PT_LEAKY;                                         // `if m_e.real < 0: pass`
  X.mu = sqrt(m_e);
  X.R = P.R_factor / k;
  const K m2R1 = real_of_k(C.kj, -2.0 * (X.R - 1.0), 2.0 * X.R / k);   // -2 (R - 1), R = R_factor / k
  const Z xE = m2R1 * X.mu;
  const cz vE = esb::cz_exp_sincos(value_of(xE));                     // the slab's exponential; d e^x = e^x dx
  X.E2 = lift(vE, vE, xE);
  const Z gq = Z(P.ic1) / X.mu;
  X.gp = P.ic0 + gq; X.gm = P.ic0 - gq;
  const Z y = X.mu * ((X.gp - X.E2 * X.gm) / (X.gp + X.E2 * X.gm));
  X.outer = X.p_e * y;
  if (X.status == ES_PT_OK && !cz_finite(value_of(X.outer))) X.status = ES_PT_NONFINITE;
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
template <class Z, class K>
__device__ __forceinline__ void cx_adjoint(const ShootDev& P, const CxConsts<K>& C, const Z& w, double* __restrict__ sb, Z& zp,
                                           Z& zq, double& Ub, double& dUb) {
  constexpr int NB = CX_NB;
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  zp = Z(1.0); zq = Z(0.0);
  CxNode<Z> B0{Z(0.0), Z(0.0)};
  Ub = 0.0; dUb = 0.0;
  const int nchunks = (nsteps + CH - 1) / CH;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int c0 = c * CH;
    const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
    cx_stage_chunk(P, c0, nst, sb);
    if (c == nchunks - 1) B0 = cx_coef(C, w, sb[2 * nst * NB + SF_U], sb[2 * nst * NB + SF_DU], sb[2 * nst * NB + SF_DDU]);
    for (int j = nst - 1; j >= 0; --j) {
      const double* bm = sb + (2 * j + 1) * NB;
      const double* b1 = sb + (2 * j) * NB;
      Z kp, kq, sp, sq;                                       // one stage at a time; sp, sq collect h/6 (k1 + k4) + h/3 (k2 + k3)
      cx_rhs(B0, zp, zq, kp, kq);
      Z ap = kp, aq = kq;                                     // k1 + k4
      const CxNode<Z> Bm = cx_coef(C, w, bm[SF_U], bm[SF_DU], bm[SF_DDU]);
      cx_rhs(Bm, zp + h2 * kp, zq + h2 * kq, sp, sq);         // k2
      cx_rhs(Bm, zp + h2 * sp, zq + h2 * sq, kp, kq);         // k3
      sp = sp + kp; sq = sq + kq;                             // k2 + k3
      B0 = cx_coef(C, w, b1[SF_U], b1[SF_DU], b1[SF_DDU]);
      Z k4p, k4q;
      cx_rhs(B0, zp + h * kp, zq + h * kq, k4p, k4q);
      ap = ap + k4p; aq = aq + k4q;
      zp = zp + h6 * ap + h3 * sp;
      zq = zq + h6 * aq + h3 * sq;
      if (c == 0 && j == 0) { Ub = b1[SF_U]; dUb = b1[SF_DU]; }
    }
  }
}

// ---- boundary: continuity of the displacement, symmetry condition by superposition, total pressures (SF-X:422, :455) --------
template <class Z>
struct CxMatch {
  Z Vb, sv;            // interior state at x = -1 per unit V_e(-1): Vx, Vx'
  Z outer, inner;      // the two sides of the matching condition; D_c = outer - inner
  double rel;          // |D_c| in percent of the larger side, NaN unless st == ES_PT_OK
  uint8_t st;
};

template <class Z, class K>
__device__ __forceinline__ CxMatch<Z> cx_boundary(const ShootDev& P, const CxConsts<K>& C, const CxOutside<Z>& X, const Z& w,
                                                  const Z& zp, const Z& zq, double Ub, double dUb) {
  CxMatch<Z> B;
  const Z Omb = w - C.kj * Ub;
  B.Vb = Omb / X.Oe;
  B.sv = ((P.slab_sign - zp) * B.Vb) / zq;
  B.outer = X.outer;
  B.inner = cx_total_pressure(P, C, Omb, Omb * Omb, dUb, B.Vb, B.sv);
  const cz d = value_of(B.outer) - value_of(B.inner);
  B.st = (uint8_t)X.status;
  B.rel = cz_abs(d) * 100.0 / fmax(cz_abs(value_of(B.outer)), cz_abs(value_of(B.inner)));
  if (X.status != ES_PT_OK) B.rel = NAN;
  else if (!cz_finite(d)) { B.st = ES_PT_NONFINITE; B.rel = NAN; }
  return B;
}

// one evaluation at (k, w): exterior, adjoint march, boundary.  Every lane of the workgroup must call this.
template <class Z, class K>
__device__ __forceinline__ CxMatch<Z> cx_eval(const ShootDev& P, int variant, const K& k, const Z& w, double* __restrict__ sb) {
  const CxConsts<K> C = cx_consts(P, variant, k);
  const CxOutside<Z> X = cx_exterior(P, C, w);
  Z zp, zq;
  double Ub, dUb;
  cx_adjoint(P, C, w, sb, zp, zq, Ub, dUb);
  return cx_boundary(P, C, X, w, zp, zq, Ub, dUb);
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
