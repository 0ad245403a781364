// The interior eigenfunction of one (k, omega) pair, node by node: the two RK4 marches that es_eigenfunction.hip writes out
// and es_signature.hip reduces.  One copy, so what the one stores is what the other labels.
//   slabs      adjoint march to get the boundary flux from the far-end condition, then a forward march from x = -1 that
//              visits the nodes 0 ... N-1;
//   cylinders  both marches run from the axis point OUT to the boundary.  Towards the axis the singular solution grows
//              like r^-m in P and r^-(m+1) in xi_r (1e9 and 1e12 over the interval for m = 3), and a march in that direction
//              amplifies its own rounding and truncation error by as much: xi_r near the axis came out wrong by a sixth of
//              its maximum for m = 3.  Outwards the singular part decays.  The first march carries
//              the two columns e = (1, 0) and d of the axis state to the boundary (d = (0, 1) for the kink conditions
//              P(r_ax) = target, d = (a12, -a11) with target = 0 for the sausage condition P'(r_ax) = 0), beta follows
//              from P(r_b) = P_b, and the second march visits the nodes N-1 ... 0 with the state target e + beta d.
#pragma once
#include "es_shoot_shared.hpp"

namespace es_shoot_shared {

// sink(int node, double value, double flux) once per node, in the order of the march.  Every lane marches, whatever the
// status of its exterior: the caller decides what a pair that is not ES_PT_OK reports.
template <int FAM, class Sink>
__device__ __forceinline__ void interior_rows(const ShootDev& P, double k, double w, const ExteriorLite& X, Sink&& sink) {
  constexpr int NE = FamTraits<FAM>::NE;
  constexpr int NB = FamTraits<FAM>::NB;
  constexpr bool DIAG = FamTraits<FAM>::DIAG;
  constexpr bool CYL = (FAM == FAM_CYL0 || FAM == FAM_CYLT);
  const KScal s = make_kscal(P, k);
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  SignTrack trk;
  double b[NB], e[NE], e2[NE];
  double u, v, flux_scale = 1.0;     // flux = v * flux_scale (density slab) ; see emit
  auto emit = [&](int node, const double* en) {                 // value and flux of a node from the marched state (u, v)
    double f;
    if (CYL) {
      const double x = P.xb + (double)node * P.h;
      f = v / x;                                                  // xi_r = Xi / r
    } else if (FAM == FAM_SLABD) {
      f = v * flux_scale;
    } else {
      const double Om = w - en[0];
      const double Om2 = Om * Om;
      f = P.rho_i * P.S_i * (s.kcT2 - Om2) / (Om * (s.kc2 - Om2)) * v;    // P_Ti(x) Vx', SF-G:433
    }
    sink(node, u, f);
  };
  if (CYL) {
    // axis node: coefficient set and the two columns of the axis state
    load_base<FAM>(P, 2 * nsteps, b);
    make_entry<FAM>(b, s, e);
    Coef Aax;
    coefficients<FAM>(e, P, s, w, Aax, trk);
    double target = 0.0, d0 = 0.0, d1 = 1.0;
    if (P.axis_bc == ES_AXIS_KINK) target = P.bc_const_raw * X.outer;                  // P(r_ax) = c xi_e, CF:795
    else if (P.axis_bc == ES_AXIS_ROTATION_KINK) target = -(P.bc_const_raw * X.outer);  // CR-KF:695-698
    else { d0 = Aax.a12; d1 = -Aax.a11; }                                              // P'(r_ax) = 0, CD-C:1082-1085
    // (1) columns e = (1, 0) and d to the boundary: steps of -h over the same node and mid-point entries
    double p1 = 1.0, x1 = 0.0, p2 = d0, x2 = d1;
    Coef A0 = Aax;
    for (int j = nsteps - 1; j >= 0; --j) {
      Coef Am, A1;
      load_base<FAM>(P, 2 * j + 1, b);
      make_entry<FAM>(b, s, e);
      load_base<FAM>(P, 2 * j, b);
      make_entry<FAM>(b, s, e2);
      coefficients2<FAM>(e, e2, P, s, w, Am, A1, trk);
      rk4_step_forward<DIAG>(p1, x1, A0, Am, A1, -h, -h2, -h6, -h3);
      rk4_step_forward<DIAG>(p2, x2, A0, Am, A1, -h, -h2, -h6, -h3);
      A0 = A1;
    }
    const double beta = (X.yb - target * p1) / p2;                                     // P(r_b) = P_b
    // (2) the axis state marched out again, emitting every node
    u = target + beta * d0;
    v = beta * d1;
    A0 = Aax;
    emit(nsteps, e);
    for (int j = nsteps - 1; j >= 0; --j) {
      Coef Am, A1;
      load_base<FAM>(P, 2 * j + 1, b);
      make_entry<FAM>(b, s, e);
      load_base<FAM>(P, 2 * j, b);
      make_entry<FAM>(b, s, e2);
      coefficients2<FAM>(e, e2, P, s, w, Am, A1, trk);
      rk4_step_forward<DIAG>(u, v, A0, Am, A1, -h, -h2, -h6, -h3);
      A0 = A1;
      emit(j, e2);
    }
    return;
  }
  // (1) adjoint march: the row of the transfer matrix picked by the far-end condition -> boundary state (u_b, v_b)
  load_base<FAM>(P, 2 * nsteps, b);
  make_entry<FAM, fam_scaled<FAM>()>(b, s, e);
  Coef B0;
  coefficients<FAM>(e, P, s, w, B0, trk);
  double zp, zq;
  adjoint_start(P, B0, zp, zq);
  for (int j = nsteps - 1; j >= 0; --j) {
    Coef Bm, B1;
    load_base<FAM>(P, 2 * j + 1, b);
    make_entry<FAM, fam_scaled<FAM>()>(b, s, e);
    load_base<FAM>(P, 2 * j, b);
    make_entry<FAM, fam_scaled<FAM>()>(b, s, e2);
    coefficients2<FAM>(e, e2, P, s, w, Bm, B1, trk);
    adjoint_step_normalised<FAM>(zp, zq, B0, Bm, B1, h, h2, h6, h3);      // z at its true scale
    B0 = B1;
  }
  // boundary state from the same algebra as the determinant
  if (FAM == FAM_SLABD) {
    u = X.yb;
    v = (P.slab_sign - zp) * u / zq;         // v = F Vx' ; P_T = v / w
    flux_scale = 1.0 / w;
  } else {
    const double Omb = w - e2[0];
    u = X.yb * Omb / X.Oe;
    v = (P.slab_sign - zp) * u / zq;         // v = Vx' ; P_T = P_Ti(x) v
  }
  // (2) forward march from the boundary, emitting every node
  load_base<FAM>(P, 0, b);
  make_entry<FAM>(b, s, e);
  Coef A0;
  coefficients<FAM>(e, P, s, w, A0, trk);
  emit(0, e);
  for (int j = 0; j < nsteps; ++j) {
    Coef Am, A1;
    load_base<FAM>(P, 2 * j + 1, b);
    make_entry<FAM>(b, s, e);
    load_base<FAM>(P, 2 * j + 2, b);
    make_entry<FAM>(b, s, e2);
    coefficients2<FAM>(e, e2, P, s, w, Am, A1, trk);
    rk4_step_forward<DIAG>(u, v, A0, Am, A1, h, h2, h6, h3);
    A0 = A1;
    emit(j + 1, e2);
  }
}

}  // namespace es_shoot_shared
