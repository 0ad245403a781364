// Dispersion slopes of a (k, omega) pair: the boundary determinant D = outer - inner of es_shoot_eval_points together with its
// exact partial derivatives in omega and k (include/eigensolver_amd.h section 11).  Tangent-linear (forward-mode) evaluation:
// the adjoint march, the closed-form exterior and the boundary algebra of es_shoot_device.hpp restated, formula for formula,
// over 3-component jets (value, d/d omega, d/d k).  One pair per lane, node base fields by scalar loads (wave-uniform
// addresses, as mode_signature_kernel); nothing is staged in LDS and each lane stores once per output at the end.
//   * the node entries of make_entry depend on k only; the base fields themselves are wave-uniform, so a node's entries are
//     formed from them inside node_pre (make_entry and coef_pre in one) and only the k-dependent ones are ever jets
//   * the Bessel pairs of es_bessel.hpp are evaluated at the VALUES of their arguments; a pair (e^x K_n, e^x K_{n+1}) resp.
//     e^-x (I_n, I_{n+1}) carries its own argument derivative (lift), the jet enters by the chain rule
// The value component is the arithmetic of the fp64 point march up to the grouping of the reciprocals (one per RK4 step here,
// one per two steps there for the families with fam_rcp4()).
#include "es_shoot_shared.hpp"

namespace {
using namespace es_shoot_shared;

using ::fma;                                                   // the overloads below would hide the scalar functions
using ::ldexp;

struct Jet3 { double v, dw, dk; };

__device__ __forceinline__ Jet3 jet(double v) { return {v, 0.0, 0.0}; }
__device__ __forceinline__ Jet3 operator-(const Jet3& a) { return {-a.v, -a.dw, -a.dk}; }
__device__ __forceinline__ Jet3 operator+(const Jet3& a, const Jet3& b) { return {a.v + b.v, a.dw + b.dw, a.dk + b.dk}; }
__device__ __forceinline__ Jet3 operator-(const Jet3& a, const Jet3& b) { return {a.v - b.v, a.dw - b.dw, a.dk - b.dk}; }
__device__ __forceinline__ Jet3 operator+(const Jet3& a, double b) { return {a.v + b, a.dw, a.dk}; }
__device__ __forceinline__ Jet3 operator+(double a, const Jet3& b) { return {a + b.v, b.dw, b.dk}; }
__device__ __forceinline__ Jet3 operator-(const Jet3& a, double b) { return {a.v - b, a.dw, a.dk}; }
__device__ __forceinline__ Jet3 operator-(double a, const Jet3& b) { return {a - b.v, -b.dw, -b.dk}; }
__device__ __forceinline__ Jet3 operator*(const Jet3& a, double b) { return {a.v * b, a.dw * b, a.dk * b}; }
__device__ __forceinline__ Jet3 operator*(double a, const Jet3& b) { return {a * b.v, a * b.dw, a * b.dk}; }
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
// 1 / a from its value's reciprocal r: d(1/a) = -r^2 da
__device__ __forceinline__ Jet3 rcp_from(const Jet3& a, double r) {
  const double d = -(r * r);
  return {r, d * a.dw, d * a.dk};
}
__device__ __forceinline__ Jet3 rcp(const Jet3& a) { return rcp_from(a, 1.0 / a.v); }            // IEEE quotient
__device__ __forceinline__ Jet3 rcp_fast(const Jet3& a) { return rcp_from(a, fast_rcp(a.v)); }   // the march's reciprocal
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
__device__ __forceinline__ bool finite3(const Jet3& a) { return isfinite(a.v) && isfinite(a.dw) && isfinite(a.dk); }

// make_kscal over jets: k is the jet (k, 0, 1)
struct KJet { Jet3 k, k2, kc2, kvA2, kcT2, k4c; double m2, h2; };

__device__ __forceinline__ KJet make_kjet(const ShootDev& P, double k) {
  KJet s;
  s.k = {k, 0.0, 1.0};
  s.k2 = s.k * s.k;
  const double m = (double)P.m;
  s.m2 = m * m;
  s.kc2 = s.k2 * P.c2_i; s.kvA2 = s.k2 * P.vA2_i; s.kcT2 = s.k2 * P.cT2_i;
  s.k4c = s.k2 * s.k2 * P.cT2_i * P.c2_i;
  s.h2 = 0.5 * P.h;
  return s;
}

// coefficient sets: only the entries the family's SHAPE reads are ever formed (a11 = -a22 for the twisted cylinder)
struct CoefJ { Jet3 a12, a21, a22; };
struct CoefPreJ { Jet3 n12, n21, n22, den; double c22; };

// make_entry (the scaled form for the untwisted cylinder, as its fp64 marches take it) followed by coef_pre, over jets:
// b holds the node's base fields (wave-uniform), the entries that do not depend on k stay plain doubles
template <int FAM>
__device__ __forceinline__ void node_pre(const double* b, const ShootDev& P, const KJet& s, const Jet3& w, CoefPreJ& C) {
  if (FAM == FAM_CYL0) {
    const Jet3 wA = s.k * b[C0_BA];
    const Jet3 e1 = wA * wA;                                  // omega_A^2
    const Jet3 e0 = s.k * b[C0_VZ];                           // Doppler shift k v_z
    const Jet3 e2 = e1 * b[C0_Q];                             // omega_c^2
    const double Bq = b[C0_B1];
    const Jet3 g = s.m2 * b[C0_E1] + s.k2 * b[C0_E2];
    const double e3 = b[C0_A1] * s.h2;
    const double e4 = -Bq * s.h2;
    const Jet3 e5 = (g - Bq * (e1 + e2)) * s.h2;
    const Jet3 e6 = (-(Bq * (e2 * e2))) * s.h2;
    const Jet3 Om = w - e0;
    const Jet3 t1 = fma(Om, Om, -e1);
    const Jet3 t2 = fma(Om, Om, -e2);
    C.n12 = e3 * t1;
    C.n21 = fma(e5, t2, e6);
    C.c22 = e4;                                               // -B, added after the division
    C.den = t1 * t2;
  } else if (FAM == FAM_CYLT) {
    const Jet3 kb = fma(b[CT_BZ], s.k, b[CT_MB]);
    const Jet3 wA = fma(b[CT_BA], s.k, b[CT_MB]);
    const Jet3 e1 = wA * wA;
    const Jet3 e0 = fma(b[CT_VZ], s.k, b[CT_MV]);
    const Jet3 e2 = e1 * b[CT_Q];
    const Jet3 e7 = b[CT_C7] * kb * b[CT_INVR];
    const Jet3 e8 = kb * b[CT_BPHI];
    const Jet3 e11 = b[CT_S] * (b[CT_M2R2] + s.k2);
    const Jet3 Om = w - e0;
    const Jet3 Om2 = Om * Om;
    const Jet3 t1 = Om2 - e1;
    const Jet3 t2 = Om2 - e2;
    const Jet3 D = b[CT_E3] * t1 * t2;
    const Jet3 Q = fma(Om, e7, fma(b[CT_E6], Om2, -(t1 * b[CT_E5])));
    const Jet3 T = fma(b[CT_E9], Om, e8);
    const Jet3 OmP = (P.c1_power == 2) ? Om2 : Om;
    const Jet3 t2T = t2 * T;
    const Jet3 C1 = fma(Q, OmP, -(b[CT_E10] * t2T));
    const Jet3 C2 = fma(Om2, Om2, -(e11 * t2));
    const Jet3 C3 = fma(D, fma(b[CT_RHO], t1, b[CT_RDC3]), fma(Q, Q, -((b[CT_E13] * t2T) * T)));
    C.n22 = C1;                                               // n11 = -n22
    C.n12 = C3 * b[CT_INVR];
    C.n21 = -(b[CT_R] * C2);
    C.den = D;
  } else if (FAM == FAM_SLABD) {
    const double rho = b[SD_RHO], c2 = b[SD_C2], vA2 = b[SD_VA2];
    const double S = c2 + vA2;
    const double cT2 = c2 * vA2 / S;
    const Jet3 w2 = w * w;
    const Jet3 n1 = s.k2 * c2 - w2;
    const Jet3 n2 = s.k2 * cT2 - w2;
    const Jet3 n3 = s.k2 * vA2 - w2;
    C.n12 = n1;
    C.n21 = rho * n3;
    C.den = (rho * S) * n2;
  } else {
    const Jet3 e0 = s.k * b[SF_U];
    const Jet3 e1 = s.k * b[SF_DU];
    const Jet3 e2 = s.k * b[SF_DDU];
    const Jet3 e3 = 2.0 * e1;
    const Jet3 Om = w - e0;
    const Jet3 Om2 = Om * Om;
    const Jet3 t = Om2 - s.kcT2;
    const Jet3 n1 = s.kc2 - Om2;
    const Jet3 n3 = s.kvA2 - Om2;
    const Jet3 St = P.S_i * t;
    const Jet3 G = fma(St, t, s.k4c);
    const Jet3 X = Om * n1;
    const Jet3 OX = Om * X;
    const Jet3 g2 = e3 * G;
    C.n22 = g2 * Om;
    C.n21 = -fma(e2, St * X, fma(-g2, e1, (n1 * n3) * OX));
    C.den = St * OX;
  }
}

template <int FAM>
__device__ __forceinline__ void node_finish(const CoefPreJ& C, const Jet3& inv, CoefJ& A) {
  if (FAM == FAM_CYL0) {
    A.a12 = C.n12; A.a21 = fma(C.n21, inv, C.c22);
  } else if (FAM == FAM_CYLT) {
    A.a22 = C.n22 * inv; A.a12 = C.n12 * inv; A.a21 = C.n21 * inv;
  } else if (FAM == FAM_SLABD) {
    A.a12 = C.n12 * inv; A.a21 = C.n21;
  } else {
    A.a21 = C.n21 * inv; A.a22 = C.n22 * inv;
  }
}

// rk4_step_adjoint over jets
template <int SHAPE>
__device__ __forceinline__ void rk4_step_adjoint_jet(Jet3& p, Jet3& q, const CoefJ& B0, const CoefJ& Bm, const CoefJ& B1,
                                                     double h, double h2, double h6, double h3) {
#define ES_RHS_TJ(A, pp, qq, kp, kq)                                                         \
  if (SHAPE == 1)      { kp = fma(-A.a22, pp, A.a21 * qq); kq = fma(A.a22, qq, A.a12 * pp); } \
  else if (SHAPE == 2) { kp = A.a21 * qq;                 kq = fma(A.a22, qq, pp); }         \
  else                 { kp = A.a21 * qq;                 kq = A.a12 * pp; }
  Jet3 k1p, k1q, k2p, k2q, k3p, k3q, k4p, k4q, tp, tq;
  ES_RHS_TJ(B0, p, q, k1p, k1q);
  tp = fma(h2, k1p, p); tq = fma(h2, k1q, q);
  ES_RHS_TJ(Bm, tp, tq, k2p, k2q);
  tp = fma(h2, k2p, p); tq = fma(h2, k2q, q);
  ES_RHS_TJ(Bm, tp, tq, k3p, k3q);
  tp = fma(h, k3p, p); tq = fma(h, k3q, q);
  ES_RHS_TJ(B1, tp, tq, k4p, k4q);
  p = fma(h6, k1p + k4p, fma(h3, k2p + k3p, p));
  q = fma(h6, k1q + k4q, fma(h3, k2q + k3q, q));
#undef ES_RHS_TJ
}

// rk4_step_adjoint_scaled0_x3 over jets: 3 z' of the untwisted cylinder, entries pre-multiplied by h/2
__device__ __forceinline__ void rk4_step_adjoint_x3_jet(Jet3& p, Jet3& q, const CoefJ& B0, const CoefJ& Bm, const CoefJ& B1) {
  const Jet3 tp1 = fma(B0.a21, q, p),   tq1 = fma(B0.a12, p, q);
  const Jet3 tp2 = fma(Bm.a21, tq1, p), tq2 = fma(Bm.a12, tp1, q);
  const Jet3 am2 = Bm.a21 + Bm.a21,     bm2 = Bm.a12 + Bm.a12;
  const Jet3 tp3 = fma(am2, tq2, p),    tq3 = fma(bm2, tp2, q);
  const Jet3 sp = fma(am2, tq2, fma(2.0, tp2, tp1));
  const Jet3 sq = fma(bm2, tp2, fma(2.0, tq2, tq1));
  p = fma(B1.a21, tq3, sp);
  q = fma(B1.a12, tp3, sq);
}

// exterior_lite over jets; yb = P_v / |P_v| is +-1 and constant: |P_v| differentiates as sign(P_v) dP_v
struct ExteriorJ {
  Jet3 outer, Oe;
  double yb;
  int status;
};

__device__ __forceinline__ ExteriorJ exterior_cylinder_jet(const ShootDev& P, const Jet3& k, const Jet3& w) {
  ExteriorJ X;
  const Jet3 k2 = k * k, w2 = w * w;
  X.Oe = w;
  const Jet3 m_e = ((k2 * P.vAe2 - w2) * (k2 * P.ce2 - w2)) / (P.Se * (k2 * P.cTe2 - w2));
  const Jet3 cst = -1.0 / (P.rho_e * (k2 * P.vAe2 - w * w));                         // w_cst = w
  X.outer = jet(NAN);
  X.yb = NAN;
  if (m_e.v < 0.0) { X.status = ES_PT_LEAKY; return X; }
  if (!(m_e.v > 0.0) || !isfinite(m_e.v) || !isfinite(cst.v)) { X.status = ES_PT_NONFINITE; return X; }
  X.status = ES_PT_OK;
  const Jet3 mu = sqrt(m_e);
  const double sgn = (P.xb < 0.0) ? -1.0 : 1.0;
  const Jet3 xR = mu * (P.R_factor / k), xb = mu;
  const int n = P.m_ext;
  const double dn = (double)n;
  double vKb, vKb1, vKR, vKR1;
  esb::ke_pair(n, xb.v, vKb, vKb1);
  esb::ke_pair(n, xR.v, vKR, vKR1);
  // d/dx [e^x K_n] = e^x K_n - e^x K_{n+1} + (n/x) e^x K_n ;  d/dx [e^x K_{n+1}] = e^x K_{n+1} - e^x K_n - ((n+1)/x) e^x K_{n+1}
  const Jet3 Kb = lift(vKb, vKb - vKb1 + (dn / xb.v) * vKb, xb), Kb1 = lift(vKb1, vKb1 - vKb - ((dn + 1.0) / xb.v) * vKb1, xb);
  const Jet3 KR = lift(vKR, vKR - vKR1 + (dn / xR.v) * vKR, xR), KR1 = lift(vKR1, vKR1 - vKR - ((dn + 1.0) / xR.v) * vKR1, xR);
  const Jet3 dKb = -Kb1 + (dn / xb) * Kb;
  const Jet3 dKR = -KR1 + (dn / xR) * KR;
  const Jet3 g = P.ic1 / (sgn * mu);
  Jet3 Pv, dPv;
  const double gap = xR.v - xb.v;
  if (gap < 40.0) {
    double vIb, vIb1, vIR, vIR1;
    esb::ie_pair_from_k(n, xb.v, vKb, vKb1, vIb, vIb1);
    esb::ie_pair_from_k(n, xR.v, vKR, vKR1, vIR, vIR1);
    // d/dx [e^-x I_n] = -e^-x I_n + e^-x I_{n+1} + (n/x) e^-x I_n ;  d/dx [e^-x I_{n+1}] = -e^-x I_{n+1} + e^-x I_n - ((n+1)/x) e^-x I_{n+1}
    const Jet3 Ib = lift(vIb, vIb1 - vIb + (dn / xb.v) * vIb, xb), Ib1 = lift(vIb1, vIb - vIb1 - ((dn + 1.0) / xb.v) * vIb1, xb);
    const Jet3 IR = lift(vIR, vIR1 - vIR + (dn / xR.v) * vIR, xR), IR1 = lift(vIR1, vIR - vIR1 - ((dn + 1.0) / xR.v) * vIR1, xR);
    const Jet3 dIb = Ib1 + (dn / xb) * Ib;
    const Jet3 dIR = IR1 + (dn / xR) * IR;
    const Jet3 a_s = -(P.ic0 * dKR - g * KR);
    const Jet3 b_s = -(g * IR - P.ic0 * dIR);
    const Jet3 E2 = exp(-2.0 * (xR - xb));
    Pv = b_s * Kb + E2 * a_s * Ib;
    dPv = sgn * mu * (b_s * dKb + E2 * a_s * dIb);
  } else {
    // only sign(b_s) survives the normalisation: b_s enters as a constant
    const double rI = 1.0 - 0.5 / xR.v - (4.0 * dn * dn - 1.0) / (8.0 * xR.v * xR.v);
    const double b_s = -(g.v - P.ic0 * rI);
    Pv = b_s * Kb;
    dPv = sgn * mu * (b_s * dKb);
  }
  const double sP = (Pv.v < 0.0) ? -1.0 : 1.0;
  const Jet3 nrm = {fabs(Pv.v), sP * Pv.dw, sP * Pv.dk};
  X.yb = Pv.v / nrm.v;
  const Jet3 dyb = dPv / nrm;
  X.outer = cst * dyb;
  if (!isfinite(X.yb) || !isfinite(dyb.v)) X.status = ES_PT_NONFINITE;
  return X;
}

__device__ __forceinline__ ExteriorJ exterior_slab_jet(const ShootDev& P, const Jet3& k, const Jet3& w) {
  ExteriorJ X;
  const Jet3 k2 = k * k;
  const Jet3 Oe = w - k * P.U_e;
  const Jet3 Oe2 = Oe * Oe;
  X.Oe = Oe;
  const Jet3 m_e = ((k2 * P.vAe2 - Oe2) * (k2 * P.ce2 - Oe2)) / (P.Se * (k2 * P.cTe2 - Oe2));
  const Jet3 cst = P.rho_e * P.Se * (k2 * P.cTe2 - Oe2) / (Oe * (k2 * P.ce2 - Oe2));
  X.outer = jet(NAN);
  X.yb = NAN;
  if (m_e.v < 0.0) { X.status = ES_PT_LEAKY; return X; }
  if (!(m_e.v > 0.0) || !isfinite(m_e.v) || !isfinite(cst.v)) { X.status = ES_PT_NONFINITE; return X; }
  X.status = ES_PT_OK;
  const Jet3 mu = sqrt(m_e);
  const Jet3 R = P.R_factor / k;
  const Jet3 E2 = exp(-2.0 * mu * (R - 1.0));
  const Jet3 gp = P.ic0 + P.ic1 / mu, gm = P.ic0 - P.ic1 / mu;
  const Jet3 V = gp + E2 * gm;
  const Jet3 dV = mu * (gp - E2 * gm);
  const double sV = (V.v < 0.0) ? -1.0 : 1.0;
  const Jet3 nrm = {fabs(V.v), sV * V.dw, sV * V.dk};
  X.yb = V.v / nrm.v;
  const Jet3 dyb = dV / nrm;
  X.outer = cst * dyb;
  if (!isfinite(X.yb) || !isfinite(dyb.v)) X.status = ES_PT_NONFINITE;
  return X;
}

// boundary_algebra over jets: the inner part from the row (r1, r2); Om_first = omega - k U_i(-1) (flow slab)
template <int FAM>
__device__ __forceinline__ Jet3 inner_jet(const ShootDev& P, const KJet& s, const Jet3& w, const ExteriorJ& X, const Jet3& r1,
                                          const Jet3& r2, const Jet3& Om_first) {
  if (FAM == FAM_CYL0 || FAM == FAM_CYLT) {
    const double Pb = X.yb;
    Jet3 Xb;
    if (P.axis_bc == ES_AXIS_KINK) Xb = (P.bc_const * X.outer - r1 * Pb) / r2;
    else if (P.axis_bc == ES_AXIS_ROTATION_KINK) Xb = (-(P.bc_const * X.outer) - r1 * Pb) / r2;
    else Xb = -(r1 * Pb) / r2;
    return Xb / P.xb;
  } else if (FAM == FAM_SLABD) {
    const Jet3 sv = (P.slab_sign - r1) * X.yb / r2;
    return sv / w;
  } else {
    const Jet3 Omb = Om_first;
    const Jet3 Vb = X.yb * Omb / X.Oe;
    const Jet3 sv = (P.slab_sign - r1) * Vb / r2;
    const Jet3 Omb2 = Omb * Omb;
    const Jet3 PTi = (P.rho_i * P.S_i) * (s.kcT2 - Omb2) / (Omb * (s.kc2 - Omb2));
    return PTi * sv;
  }
}

template <int FAM>
__global__ __launch_bounds__(64) void root_slopes_kernel(ShootDev P, const double* __restrict__ kv,
                                                         const double* __restrict__ wv, int n,
                                                         const int32_t* __restrict__ d_count, double* __restrict__ outer,
                                                         double* __restrict__ inner, uint8_t* __restrict__ status) {
  constexpr int NB = FamTraits<FAM>::NB;
  constexpr bool CYL = (FAM == FAM_CYL0 || FAM == FAM_CYLT);
  const int cnt = es_count_clamped(d_count, n);                // n stays the row length of the [3][n] outputs
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole wave lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < cnt;
  const double k = in ? kv[i] : 1.0;
  const Jet3 w = {in ? wv[i] : 1.0, 1.0, 0.0};
  const KJet s = make_kjet(P, k);
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  const ExteriorJ X = CYL ? exterior_cylinder_jet(P, s.k, w) : exterior_slab_jet(P, s.k, w);
  double b[NB];
  CoefPreJ C0;
  CoefJ B0;
  load_base<FAM>(P, 2 * nsteps, b);
  node_pre<FAM>(b, P, s, w, C0);
  node_finish<FAM>(C0, rcp(C0.den), B0);                       // first node of the traversal: its own division
  Jet3 zp = jet(1.0), zq = jet(0.0);                           // adjoint_start
  if (CYL && P.axis_bc == ES_AXIS_SAUSAGE) {
    zp = (FAM == FAM_CYLT) ? -B0.a22 : jet(0.0);               // a11
    zq = B0.a12;
  }
  for (int j = nsteps - 1; j >= 0; --j) {
    CoefPreJ Cm, C1;
    CoefJ Bm, B1;
    load_base<FAM>(P, 2 * j + 1, b);
    node_pre<FAM>(b, P, s, w, Cm);
    load_base<FAM>(P, 2 * j, b);
    node_pre<FAM>(b, P, s, w, C1);
    const Jet3 inv = rcp_fast(Cm.den * C1.den);                // one reciprocal per step (coefficients2)
    node_finish<FAM>(Cm, C1.den * inv, Bm);
    node_finish<FAM>(C1, Cm.den * inv, B1);
    if (fam_unnormalised<FAM>()) rk4_step_adjoint_x3_jet(zp, zq, B0, Bm, B1);
    else rk4_step_adjoint_jet<FamTraits<FAM>::SHAPE>(zp, zq, B0, Bm, B1, h, h2, h6, h3);
    B0 = B1;
    if (fam_unnormalised<FAM>() && (j % CH) == 0) {
      // the power of two the point march takes at the end of its LDS chunk [j, j + nst): the scale P.bc_const carries
      const int nst = (nsteps - j < CH) ? (nsteps - j) : CH;
      const int ex = adjoint_rescale_exp(nsteps - j - nst, nsteps - j);
      zp = ldexp(zp, ex);
      zq = ldexp(zq, ex);
    }
  }
  Jet3 Om_first = w;
  if (FAM == FAM_SLABF) Om_first = w - s.k * P.base[(size_t)SF_U * P.npts];
  const Jet3 I = inner_jet<FAM>(P, s, w, X, zp, zq, Om_first);
  if (!in) return;
  const bool good = X.status == ES_PT_OK && finite3(X.outer) && finite3(I);
  const Jet3 bad = {NAN, NAN, NAN};
  const Jet3 O = good ? X.outer : bad, J = good ? I : bad;
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
