// The complex-frequency evaluation of the cylinder, written once over the scalar Z and the family F
// (include/eigensolver_amd.h sections 14, 15, 17 and 18; the CPU restatements are tests/cyl_complex_model.py,
// tests/cyl_complex_slope_model.py, tests/cylt_complex_model.py and tests/cylt_complex_slope_model.py):
//   Z = esb::cz        the plain complex value: es_cyl_complex.hip (determinant, roots; both families)
//   Z = esb::CJet<1>   value and d/d omega: the Newton steps of es_cyl_complex_slopes.hip (both families)
//   Z = esb::CJet<2>   value, d/d omega and d/dk: the slopes
// The wavenumber comes as K: a plain double where it is a constant of the differentiation (cz, CJet<1>), the jet (k, 0, 1)
// for CJet<2>.  F defaults to FAM_CYL0, the untwisted cylinder.  The eigenfunction march of sections 16 and 19
// (es_cyl_complex_eigen.hip) uses cyl_exterior, cyl_stage_chunk and cyl_node of this text at Z = esb::cz, over F.
//
// Interior: the formula text of es_shoot_device.hpp for the family (make_entry, coef_pre, coef_finish, adjoint_start,
// rk4_step_adjoint<SHAPE>, boundary_algebra) instantiated with Z, TRACK = false, the plain (not scaled, normalised) RK4 step, one
// IEEE complex division per node.  Nothing of the coefficient formulas is restated here.
// Exterior, written for the complex case (cyl_exterior): m_e and xi_e_const as exterior_cylinder, mu = principal sqrt(m_e),
// K_n and I_n at complex argument (es_bessel_complex.hpp), the same far-field initial values and I-admixture.  The solution is
// normalised by its own complex boundary value, P_e(boundary) = 1, where the real path divides by |P_v| and keeps the sign yb:
// on the real axis D_c = yb D.
// Every decision is taken on the value component: ES_PT_LEAKY where Re m_e < 0 (the rule of the slab's complex path, and of
// the real path on the real axis; it keeps mu in the sector |arg mu| <= pi/4 the Bessel routines support); ES_PT_NONFINITE
// where m_e, xi_e_const or the result is not finite -- in the jet instantiations a non-finite derivative of outer or inner
// counts too; the branch on the gap of the two Bessel arguments; the sign of the boundary.  There is no continuum status: off
// the real axis the coefficients have no zero on the grid; on it, callers have the real path (es_shoot_eval_*).
// One (k, omega) point per lane; the base table is staged in LDS chunk by chunk (CH steps) and every lane forms its own
// node entries.  Every lane of a workgroup makes every barrier call: lanes past the count march on dummy inputs and store
// nothing.  Not on the benchmark path: written for clarity.
#pragma once
#include "es_cjet.hpp"
#include "es_complex_roots.hpp"

namespace es_cyl_complex_shared {
using namespace es_complex_shared;
using esb::cz;
constexpr int FAM = FAM_CYL0;                               // the family of sections 14 - 16
// No NB / NE at this level: every function takes the sizes of its own family from FamTraits<F>.
template <int F> constexpr int cyl_lds_doubles() { return FamTraits<F>::NB * (2 * CH + 1); }   // one chunk: nodes and mid-points of CH steps
constexpr int CYLC_LDS_DOUBLES = cyl_lds_doubles<FAM>();

// what boundary_algebra reads of an exterior
template <class Z> struct CylcExterior {
  Z outer;           // xi_e = xi_e_const P_e'(boundary) / P_e(boundary)
  double yb;         // P_e(boundary) after the normalisation: 1
  Z Oe;              // (flow slab only)
  int status;
};

// The exterior solution itself, before the boundary ratio is taken: what cyl_exterior reduces to xi_e and the eigenfunction
// kernel of es_cyl_complex_eigen.hip evaluates at every exterior point.  Up to the common factor dropped below,
//   P_e(x) = [b_s Ke_n(mu |x|) + e^{-2 (xR - mu |x|)} a_s Ie_n(mu |x|)] e^{-(mu |x| - xb)},     P_e(boundary) = Pv;
// with `near` false the I part is dropped (a_s is not formed, b_s = 1).  Fields past `status` are set only for ES_PT_OK.
template <class Z> struct CylcExteriorSolution {
  int status;        // ES_PT_OK, ES_PT_LEAKY or ES_PT_NONFINITE by m_e and xi_e_const alone
  bool near;         // Re(xR - xb) < 40: the I-admixture is kept
  double sgn;        // sign of the boundary radius
  Z cst;             // xi_e_const
  Z mu, xR, xb;      // principal sqrt(m_e); the Bessel arguments of the far field and the boundary
  Z a_s, b_s;
  Z Pv, dPv;         // P_e and dP_e/dr at the boundary
};

template <class Z, class K>
__device__ __forceinline__ CylcExteriorSolution<Z> cyl_exterior_solution(const ShootDev& P, const K& k, const Z& w) {
  CylcExteriorSolution<Z> S;
  const K k2 = k * k;
  const Z w2 = w * w;
  const Z m_e = ((k2 * P.vAe2 - w2) * (k2 * P.ce2 - w2)) / (P.Se * (k2 * P.cTe2 - w2));       // CF:699
  S.cst = -1.0 / (P.rho_e * (k2 * P.vAe2 - w2));                                              // CF:702
  if (val(m_e) < 0.0) { S.status = ES_PT_LEAKY; return S; }
  if (!esb::cz_finite(value_of(m_e)) || !esb::cz_finite(value_of(S.cst))) { S.status = ES_PT_NONFINITE; return S; }
  S.status = ES_PT_OK;
  const Z mu = sqrt(m_e);
  const double sgn = (P.xb < 0.0) ? -1.0 : 1.0;
  const Z xR = mu * (P.R_factor / k), xb = mu;
  S.mu = mu; S.sgn = sgn; S.xR = xR; S.xb = xb;
  const int n = P.m_ext;
  const double dn = (double)n;
  Z Kb, Kb1, KR, KR1;
  cke_pair(n, xb, Kb, Kb1);
  cke_pair(n, xR, KR, KR1);
  const Z dKb = (dn / xb) * Kb - Kb1;                // e^z K_n'(z)
  const Z dKR = (dn / xR) * KR - KR1;
  const Z g = P.ic1 / (sgn * mu);
  // P = a I + b K with (a, b) from the far-field values; common factor xR e^{xR - xb} dropped
  const Z gap = xR - xb;
  S.near = val(gap) < 40.0;
  if (S.near) {
    Z Ib, Ib1, IR, IR1;
    cie_pair_from_k(n, xb, Kb, Kb1, Ib, Ib1);
    cie_pair_from_k(n, xR, KR, KR1, IR, IR1);
    const Z dIb = Ib1 + (dn / xb) * Ib;              // e^-z I_n'(z)
    const Z dIR = IR1 + (dn / xR) * IR;
    const Z a_s = -(P.ic0 * dKR - g * KR);
    const Z b_s = -(g * IR - P.ic0 * dIR);
    const Z E2 = exp(-2.0 * gap);
    S.a_s = a_s; S.b_s = b_s;
    S.Pv = b_s * Kb + E2 * a_s * Ib;
    S.dPv = (sgn * mu) * (b_s * dKb + E2 * a_s * dIb);
  } else {
    // I-admixture below e^-80: only the K part is left and b cancels in the normalisation
    S.a_s = Z(cz(0.0, 0.0)); S.b_s = Z(cz(1.0, 0.0));
    S.Pv = Kb;
    S.dPv = (sgn * mu) * dKb;
  }
  return S;
}

template <class Z, class K> __device__ __forceinline__ CylcExterior<Z> cyl_exterior(const ShootDev& P, const K& k, const Z& w) {
  CylcExterior<Z> X;
  X.Oe = w;
  X.yb = 1.0;
  X.outer = Z(cz(NAN, NAN));
  const CylcExteriorSolution<Z> S = cyl_exterior_solution<Z, K>(P, k, w);
  X.status = S.status;
  if (S.status != ES_PT_OK) return X;
  X.outer = S.cst * (S.dPv / S.Pv);
  if (!all_finite(X.outer)) X.status = ES_PT_NONFINITE;
  return X;
}

// Copies the base table of the nst steps from step c0 on (2 nst + 1 points, point-major) into the LDS buffer `sb`, between two
// barriers: every lane of the workgroup makes every call.
// The twisted family's 20 fields are walked with one running row pointer: unrolled, their 19 row offsets are formed once per
// kernel and held in scalar registers through every inlined copy of the evaluation (the refinement kernel has four), 38 of
// the 61 scalar registers that kernel then spilled to vector lanes.  Same copies either way.
template <int F = FAM>
__device__ __forceinline__ void cyl_stage_chunk(const ShootDev& P, int c0, int nst, double* __restrict__ sb) {
  constexpr int NB = FamTraits<F>::NB;
  __syncthreads();
  if constexpr (NB > 8) {
    const double* __restrict__ row = P.base + 2 * c0;
#pragma nounroll
    for (int f = 0; f < NB; ++f, row += P.npts)
      for (int i = threadIdx.x; i < 2 * nst + 1; i += blockDim.x) sb[i * NB + f] = row[i];
  } else {
#pragma unroll
    for (int f = 0; f < NB; ++f)
      for (int i = threadIdx.x; i < 2 * nst + 1; i += blockDim.x) sb[i * NB + f] = P.base[(size_t)f * P.npts + 2 * c0 + i];
  }
  __syncthreads();
}

// coefficients of the node whose base fields are at b
template <class Z, int F = FAM>
__device__ __forceinline__ CoefT<Z> cyl_node(const ShootDev& P, const KScalT<Z>& s, const Z& w, const double* __restrict__ bn, Z* e) {
  constexpr int NB = FamTraits<F>::NB, NE = FamTraits<F>::NE;
  double b[NB], c[NE];
#pragma unroll
  for (int f = 0; f < NB; ++f) b[f] = bn[f];
  make_entry<F, false>(b, s, e, c);
  SignTrack trk;
  CoefPreT<Z> C;
  coef_pre<F, false>(e, c, P, s, w, C, trk);
  CoefT<Z> A;
  coef_finish<F>(C, 1.0 / C.den, A);
  return A;
}

// The two sides of the matching condition at (k, w): D_c = outer - inner.  rel (percent) and st are formed from the values;
// unless st == ES_PT_OK, outer and inner are not to be used and rel is NaN.
template <class Z> struct CylcMatch {
  Z outer, inner;
  double rel;
  uint8_t st;
};

// P carries bc_const at its true scale (the launches pass bc_const_raw).  Every lane of the workgroup must call this.
template <class Z, class K, int F = FAM>
__device__ __forceinline__ CylcMatch<Z> cyl_shoot_point(const ShootDev& P, const K& k, const Z& w, double* __restrict__ sb) {
  constexpr int NB = FamTraits<F>::NB, NE = FamTraits<F>::NE;
  const KScalT<Z> s = make_kscal(P, Z(k));
  const CylcExterior<Z> X = cyl_exterior<Z, K>(P, k, w);
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  Z e[NE];
  CoefT<Z> B0;
  Z zp(0.0), zq(0.0);
  const int nchunks = (nsteps + CH - 1) / CH;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int c0 = c * CH;
    const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
    cyl_stage_chunk<F>(P, c0, nst, sb);
    if (c == nchunks - 1) {                            // last node: start vector of the march
      B0 = cyl_node<Z, F>(P, s, w, sb + 2 * nst * NB, e);
      adjoint_start<F>(P, B0, zp, zq);
    }
    for (int j = nst - 1; j >= 0; --j) {
      const CoefT<Z> Bm = cyl_node<Z, F>(P, s, w, sb + (2 * j + 1) * NB, e);
      const CoefT<Z> B1 = cyl_node<Z, F>(P, s, w, sb + (2 * j) * NB, e);
      rk4_step_adjoint<FamTraits<F>::SHAPE>(zp, zq, B0, Bm, B1, h, h2, h6, h3);
      B0 = B1;
    }
  }
  // e: the entries of the boundary node (read by the slab branches of boundary_algebra only)
  const MismatchT<Z> M = boundary_algebra<F>(P, s, w, X, zp, zq, e);
  CylcMatch<Z> R;
  R.outer = M.outer;
  R.inner = M.inner;
  R.st = (uint8_t)X.status;
  const cz o = value_of(M.outer), in = value_of(M.inner), d = value_of(M.d);
  const double sc = P.accept_norm ? esb::cz_abs(o) : fmax(esb::cz_abs(o), esb::cz_abs(in));
  R.rel = esb::cz_abs(d) * 100.0 / sc;
  if (X.status == ES_PT_OK && !(esb::cz_finite(d) && all_finite(M.outer) && all_finite(M.inner))) R.st = ES_PT_NONFINITE;
  if (R.st != ES_PT_OK) R.rel = NAN;
  return R;
}

// the family check of every entry point of sections 14 - 19
template <int F = FAM> int check_cyl_cx(es_context* ctx, const es_problem* prob) {
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  if (prob->dev.family != F) {
    ctx->last_error = F == FAM_CYLT
                          ? "es_cylt_complex_* is implemented for ES_GEOM_CYLINDER_TWIST problems only (the twisted cylinder)"
                          : "es_cyl_complex_* is implemented for ES_GEOM_CYLINDER problems only (the untwisted cylinder)";
    return ES_ERR_UNSUPPORTED;
  }
  return ES_SUCCESS;
}

// the problem as the complex march takes it: z at its true scale, so the target of the axis condition as given
inline ShootDev cyl_cx_dev(const es_problem* prob) {
  ShootDev P = prob->dev;
  P.bc_const = P.bc_const_raw;
  return P;
}

// The kernels that inline the evaluation more than once -- the refinement kernel of es_cyl_complex.hip (four copies) and the
// Newton kernel of es_cyl_complex_slopes.hip (two) -- keep their wave-uniform arguments in vector registers for the families
// named here: with the 20-field table of FAM_CYLT what the copies share would otherwise be spilled from scalar registers.
// The comments at the two kernels say what is done and why; the evaluation and slopes kernels carry no remedy.
template <int F> constexpr bool cyl_uniforms_in_vgprs = F == FAM_CYLT;
#define ES_V(x) asm volatile("" : "+v"(x))
__device__ __forceinline__ void vector_resident(ShootDev& P) {
  ES_V(P.xb); ES_V(P.h); ES_V(P.rho_e); ES_V(P.vAe2); ES_V(P.ce2); ES_V(P.cTe2); ES_V(P.Se); ES_V(P.R_factor);
  ES_V(P.ic0); ES_V(P.ic1); ES_V(P.bc_const); ES_V(P.base); ES_V(P.npts); ES_V(P.m); ES_V(P.m_ext); ES_V(P.axis_bc);
  ES_V(P.c1_power); ES_V(P.accept_norm);
}
// The problem as one inlined copy of the evaluation takes it: for those families a copy with a scalar n_nodes of its own, from
// which the copy derives its chunk and step counts; P itself otherwise.
template <int F> __device__ __forceinline__ decltype(auto) cyl_own_counts(const ShootDev& P) {
  if constexpr (cyl_uniforms_in_vgprs<F>) {
    ShootDev Q = P;
    asm volatile("" : "+s"(Q.n_nodes));
    return Q;
  } else {
    return (P);
  }
}

}  // namespace es_cyl_complex_shared
