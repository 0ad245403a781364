// K16a, K19: eigenfunctions of the cylinder at complex (k, omega) -- P(r) and xi_r(r) of an unstable (Kelvin-Helmholtz) mode --
// for the untwisted cylinder (FAM_CYL0, include/eigensolver_amd.h section 16, es_cyl_complex_eigenfunction; the CPU
// restatement is tests/cyl_complex_eigen_model.py) and the twisted, rotating one (FAM_CYLT, section 19,
// es_cylt_complex_eigenfunction, cylteig_interior_kernel below; tests/cylt_complex_eigen_model.py).  Untwisted cylinder:
//
// Interior: the algorithm of interior_rows (es_interior_march.hpp, cylinder branch) in complex arithmetic.  Both marches run
// from the axis node out to the boundary: the first carries the columns e = (1, 0) and d of the axis state, beta follows from
// P(r_b) = P_b = 1, the second writes every node.  The node coefficients are cyl_node<cz> of es_cyl_complex_shared.hpp (the one
// FAM_CYL0 text, one complex division per node) on the base table staged in LDS chunk by chunk as cyl_shoot_point stages it,
// the chunks in the same order -- axis end first -- twice; the step is rk4_step_forward<DIAG, cz> of es_shoot_shared.hpp.
// The adjoint step of the determinant is J (this outward step) J^-1 for the trace-free coefficient matrix, so the jump of the
// flux at the boundary equals D_c of section 14 to rounding where the axis target is zero (ES_AXIS_SAUSAGE, bc_const = 0:
// every untwisted reference problem).
// Exterior: cyl_exterior_solution, the solution cyl_exterior reduces to xi_e, evaluated at every exterior point; one lane per
// (pair, point).
// One (k, omega) pair per lane in the interior kernel; every lane of a workgroup makes every barrier call: lanes past the count
// march on dummy inputs and store nothing.  Not on the benchmark path: written for clarity.
#include "es_cyl_complex_shared.hpp"

namespace {
using namespace es_cyl_complex_shared;

__device__ __forceinline__ void store_cz(double* __restrict__ a, size_t o, cz v) {
  a[2 * o] = v.re;
  a[2 * o + 1] = v.im;
}

// value / flux [n x N] interleaved complex; stout [n]: the status section 14 gives the pair
__global__ __launch_bounds__(64) void cyleig_interior_kernel(ShootDev P, const double* __restrict__ kv,
                                                             const double* __restrict__ wre,
                                                             const double* __restrict__ wim, int n,
                                                             double* __restrict__ value, double* __restrict__ flux,
                                                             uint8_t* __restrict__ stout) {
  constexpr bool DIAG = FamTraits<FAM>::DIAG;
  constexpr int NB = FamTraits<FAM>::NB, NE = FamTraits<FAM>::NE;
  __shared__ double sb[CYLC_LDS_DOUBLES];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const double k = in ? kv[i] : 1.0;
  const cz w = in ? cz(wre[i], wim[i]) : cz(1.0, 0.1);
  const KScalT<cz> s = make_kscal(P, cz(k));
  const CylcExterior<cz> X = cyl_exterior<cz, double>(P, k, w);
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  const int nchunks = (nsteps + CH - 1) / CH;
  const cz nan(NAN, NAN);
  cz e[NE];
  CoefT<cz> A0;
  cz target(0.0), d0(0.0), d1(1.0);                    // axis state target e + beta d
  cz p1(1.0), x1(0.0), p2, x2;                         // the columns e and d on their way to the boundary
  cz u, v;                                             // the state of the writing march
  bool ok = X.status == ES_PT_OK;
  uint8_t st = (uint8_t)X.status;
  const size_t row = (size_t)i * P.n_nodes;
  auto emit = [&](int node) {
    if (!in) return;
    const double x = P.xb + (double)node * P.h;
    store_cz(value, row + node, ok ? u : nan);
    store_cz(flux, row + node, ok ? v / x : nan);      // xi_r = Xi / r
  };
  for (int pass = 0; pass < 2; ++pass) {
    for (int c = nchunks - 1; c >= 0; --c) {
      const int c0 = c * CH;
      const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
      cyl_stage_chunk(P, c0, nst, sb);
      if (c == nchunks - 1) {                          // axis node: its coefficient set starts either march
        A0 = cyl_node(P, s, w, sb + 2 * nst * NB, e);
        if (pass == 0) {
          if (P.axis_bc == ES_AXIS_KINK) target = P.bc_const_raw * X.outer;      // P(r_ax) = c xi_e, CF:795
          else { d0 = A0.a12; d1 = -A0.a11; }                                    // P'(r_ax) = 0, CD-C:1082-1085
          p2 = d0; x2 = d1;
        } else {
          const cz beta = (X.yb - target * p1) / p2;                             // P(r_b) = P_b
          // the status of section 14: the mismatch of the two columns' boundary state has to be finite
          const cz inner = (target * x1 + beta * x2) / P.xb;
          if (ok && !(esb::cz_finite(inner) && esb::cz_finite(X.outer - inner))) { ok = false; st = ES_PT_NONFINITE; }
          u = target + beta * d0;
          v = beta * d1;
          emit(nsteps);
        }
      }
      for (int j = nst - 1; j >= 0; --j) {             // steps of -h over the node and mid-point entries of the chunk
        const CoefT<cz> Am = cyl_node(P, s, w, sb + (2 * j + 1) * NB, e);
        const CoefT<cz> A1 = cyl_node(P, s, w, sb + (2 * j) * NB, e);
        if (pass == 0) {
          rk4_step_forward<DIAG>(p1, x1, A0, Am, A1, -h, -h2, -h6, -h3);
          rk4_step_forward<DIAG>(p2, x2, A0, Am, A1, -h, -h2, -h6, -h3);
        } else {
          rk4_step_forward<DIAG>(u, v, A0, Am, A1, -h, -h2, -h6, -h3);
          emit(c0 + j);
        }
        A0 = A1;
      }
    }
  }
  if (in) stout[i] = st;
}

// The twisted cylinder (section 19).  The eigenfunction is the solution of the same discrete problem -- one outward RK4 step
// y_j = S_j y_{j+1} per interval (rk4_step_forward<true>, steps of -h, the coefficient sets cyl_node<cz, FAM_CYLT>), the axis
// condition at node N-1, P = 1 at node 0 -- but it is not formed as section 16 forms it.  Every ES_AXIS_ROTATION_KINK problem
// has a non-zero axis target; then the solution is O(1) at both ends while any state marched outwards grows like the regular
// solution r^m, and P(r_b) = 1 comes out of a cancellation that left 1e-9 (m = 3) to 1e-6 (m = 4) of rounding in fp64
// (DESIGN.md section 8n).  Instead each part is marched in the direction in which it does not lose to the other:
//   pass 0  g, from g_{N-1} = d at the axis outwards (d = (0, 1); sausage: (a12, -a11)); the raw (P, Xi) of every node is
//           parked in the lane's own output rows;
//   pass 1  s, from s_0 = (0, 1) at the boundary inwards by the exact inverse of the same step, s_{j+1} = S_j^-1 s_j, S_j from
//           the step applied to (1, 0) and (0, 1); it yields s_{N-1};
//   pass 2  s again, and every node written: y_j = a s_j + b g_j, b = 1 / P(g_0) (so P(r_b) = 1: s_0 has no P), a from the
//           axis condition, a = target / P(s_{N-1}) for the kink conditions (d has no P) and a = 0 for the sausage condition.
// The chunks are staged axis end first in pass 0 and boundary end first in passes 1 and 2.  value / flux [n x N] interleaved
// complex; stout [n]: the status section 17 gives the pair, plus the non-finite check on the boundary state.
__global__ __launch_bounds__(64) void cylteig_interior_kernel(ShootDev P, const double* __restrict__ kv,
                                                              const double* __restrict__ wre,
                                                              const double* __restrict__ wim, int n,
                                                              double* value, double* flux, uint8_t* __restrict__ stout) {
  constexpr int F = FAM_CYLT;
  constexpr bool DIAG = FamTraits<F>::DIAG;
  constexpr int NB = FamTraits<F>::NB, NE = FamTraits<F>::NE;
  __shared__ double sb[cyl_lds_doubles<F>()];               // 20 (2 CH + 1) doubles: 41 120 B
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const double k = in ? kv[i] : 1.0;
  const cz w = in ? cz(wre[i], wim[i]) : cz(1.0, 0.1);
  const KScalT<cz> s = make_kscal(P, cz(k));
  const CylcExterior<cz> X = cyl_exterior<cz, double>(P, k, w);
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  const int nchunks = (nsteps + CH - 1) / CH;
  const cz nan(NAN, NAN);
  cz e[NE];
  CoefT<cz> A0;
  cz target(0.0);
  cz u(0.0), v(1.0);                                   // g on its way out (pass 0), s on its way in (passes 1, 2)
  cz a(0.0), b(0.0), gx(0.0);                          // y = a s + b g; gx: Xi of g at the boundary
  bool ok = X.status == ES_PT_OK;
  uint8_t st = (uint8_t)X.status;
  const size_t row = (size_t)i * P.n_nodes;
  auto park = [&](int node) {                          // pass 0: the raw state of g
    if (!in) return;
    store_cz(value, row + node, u);
    store_cz(flux, row + node, v);
  };
  auto emit = [&](int node) {                          // pass 2: y = a s + b g of the node, xi_r = Xi / r
    if (!in) return;
    const size_t o = row + node;
    const cz gp(value[2 * o], value[2 * o + 1]), gv(flux[2 * o], flux[2 * o + 1]);
    const double x = P.xb + (double)node * P.h;
    store_cz(value, o, ok ? a * u + b * gp : nan);
    store_cz(flux, o, ok ? (a * v + b * gv) / x : nan);
  };
  for (int pass = 0; pass < 3; ++pass) {
    const bool outward = pass == 0;
    for (int cc = 0; cc < nchunks; ++cc) {
      const int c = outward ? nchunks - 1 - cc : cc;
      const int c0 = c * CH;
      const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
      cyl_stage_chunk<F>(P, c0, nst, sb);
      if (cc == 0) {                                   // the node the march of this pass starts at
        if (outward) {                                 // axis node
          A0 = cyl_node<cz, F>(P, s, w, sb + 2 * nst * NB, e);
          if (P.axis_bc == ES_AXIS_KINK) target = P.bc_const_raw * X.outer;                   // P(r_ax) = c xi_e, CF:795
          else if (P.axis_bc == ES_AXIS_ROTATION_KINK) target = -(P.bc_const_raw * X.outer);  // CR-KF:695-698
          else { u = A0.a12; v = -A0.a11; }                                                   // P'(r_ax) = 0, CD-C:1082-1085
          park(nsteps);
        } else {                                       // boundary node
          A0 = cyl_node<cz, F>(P, s, w, sb, e);
          u = cz(0.0); v = cz(1.0);
          if (pass == 2) emit(0);
        }
      }
      for (int jj = 0; jj < nst; ++jj) {
        const int j = outward ? nst - 1 - jj : jj;     // the interval between the nodes c0 + j and c0 + j + 1
        const CoefT<cz> Am = cyl_node<cz, F>(P, s, w, sb + (2 * j + 1) * NB, e);
        if (outward) {
          const CoefT<cz> A1 = cyl_node<cz, F>(P, s, w, sb + (2 * j) * NB, e);
          rk4_step_forward<DIAG>(u, v, A0, Am, A1, -h, -h2, -h6, -h3);
          park(c0 + j);
          A0 = A1;
        } else {
          const CoefT<cz> A1 = cyl_node<cz, F>(P, s, w, sb + (2 * j + 2) * NB, e);
          cz m11(1.0), m21(0.0), m12(0.0), m22(1.0);   // S_j: the outward step from node c0 + j + 1 to node c0 + j
          rk4_step_forward<DIAG>(m11, m21, A1, Am, A0, -h, -h2, -h6, -h3);
          rk4_step_forward<DIAG>(m12, m22, A1, Am, A0, -h, -h2, -h6, -h3);
          const cz idet = 1.0 / (m11 * m22 - m12 * m21);
          const cz nu = (m22 * u - m12 * v) * idet, nv = (m11 * v - m21 * u) * idet;
          u = nu; v = nv;
          if (pass == 2) emit(c0 + j + 1);
          A0 = A1;
        }
      }
    }
    if (pass == 0) {
      b = X.yb / u;                                    // P(r_b) = P_b
      gx = v;
    } else if (pass == 1) {
      if (P.axis_bc != ES_AXIS_SAUSAGE) a = target / u;
      // the status of section 17: the mismatch at the boundary has to be finite
      const cz inner = (a + b * gx) / P.xb;
      if (ok && !(esb::cz_finite(inner) && esb::cz_finite(X.outer - inner))) { ok = false; st = ES_PT_NONFINITE; }
    }
  }
  if (in) stout[i] = st;
}

// P_e and xi_e = xi_e_const P_e' on linspace(sgn R, sgn 1, n_ext), per unit P_e(boundary); stin: what the interior kernel found
__global__ __launch_bounds__(256) void cyleig_exterior_kernel(ShootDev P, const double* __restrict__ kv,
                                                              const double* __restrict__ wre,
                                                              const double* __restrict__ wim, int n, int n_ext,
                                                              const uint8_t* __restrict__ stin, double* __restrict__ xs,
                                                              double* __restrict__ value, double* __restrict__ flux) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)n * n_ext) return;
  const int i = (int)(t / n_ext), j = (int)(t - (long)i * n_ext);
  const double k = kv[i];
  const cz w(wre[i], wim[i]);
  const double sgn = (P.xb < 0.0) ? -1.0 : 1.0;
  const double R = P.R_factor / k;
  // np.linspace(sgn*R, sgn*1, n_ext)[j]
  const double step = (sgn * 1.0 - sgn * R) / (double)(n_ext - 1);
  const double x = (j == n_ext - 1) ? sgn * 1.0 : sgn * R + (double)j * step;
  cz pv(NAN, NAN), f(NAN, NAN);
  if (stin[i] == ES_PT_OK) {
    const CylcExteriorSolution<cz> S = cyl_exterior_solution<cz, double>(P, k, w);
    const int m = P.m_ext;
    const double dn = (double)m;
    const cz xx = S.mu * fabs(x);
    cz Kx, Kx1;
    cke_pair(m, xx, Kx, Kx1);
    const cz dKx = (dn / xx) * Kx - Kx1;               // e^z K_n'(z)
    const cz dec = exp(-(xx - S.xb));
    cz Pe = S.b_s * Kx, dPe = S.b_s * dKx;
    if (S.near) {
      cz Ix, Ix1;
      cie_pair_from_k(m, xx, Kx, Kx1, Ix, Ix1);
      const cz dIx = Ix1 + (dn / xx) * Ix;             // e^-z I_n'(z)
      const cz E2x = exp(-2.0 * (S.xR - xx));
      Pe = S.b_s * Kx + E2x * S.a_s * Ix;
      dPe = S.b_s * dKx + E2x * S.a_s * dIx;
    }
    pv = (dec * Pe) / S.Pv;
    f = S.cst * (((S.sgn * S.mu) * (dec * dPe)) / S.Pv);        // xi_e = xi_e_const P_e'
  }
  xs[t] = x;
  store_cz(value, (size_t)t, pv);
  store_cz(flux, (size_t)t, f);
}

// both entry points: the interior kernel of the family, then the one exterior kernel (the medium outside is the same)
template <int F>
int eigenfunction(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                  double* d_int_value, double* d_int_flux, int n_ext, double* d_ext_x, double* d_ext_value, double* d_ext_flux,
                  uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx<F>(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0 && n_ext >= 0, "negative size");
  ES_REQUIRE(ctx, n_ext == 0 || n_ext >= 2, "n_ext must be 0 or >= 2");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_int_value && d_int_flux, "null pointer");
  ES_REQUIRE(ctx, n_ext == 0 || (d_ext_x && d_ext_value && d_ext_flux), "null exterior arrays");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  uint8_t* st = d_status;
  if (!st) {                                           // the exterior kernel reads the status the interior kernel found
    rc = es_ensure_scratch(ctx, (size_t)n);
    if (rc) return rc;
    st = static_cast<uint8_t*>(ctx->d_scratch);
  }
  hipLaunchKernelGGL(F == FAM_CYLT ? cylteig_interior_kernel : cyleig_interior_kernel, dim3((n + 63) / 64), dim3(64), 0,
                     ctx->stream, cyl_cx_dev(prob), d_k, d_w_re, d_w_im, n, d_int_value, d_int_flux, st);
  ES_HIP_CHECK(ctx, hipGetLastError());
  if (n_ext > 0) {
    const long tot = (long)n * n_ext;
    hipLaunchKernelGGL(cyleig_exterior_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream,
                       cyl_cx_dev(prob), d_k, d_w_re, d_w_im, n, n_ext, st, d_ext_x, d_ext_value, d_ext_flux);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  return ES_SUCCESS;
}

}  // namespace

extern "C" int es_cyl_complex_eigenfunction(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                                            const double* d_w_im, int n, double* d_int_value, double* d_int_flux, int n_ext,
                                            double* d_ext_x, double* d_ext_value, double* d_ext_flux, uint8_t* d_status) {
  return eigenfunction<FAM_CYL0>(ctx, prob, d_k, d_w_re, d_w_im, n, d_int_value, d_int_flux, n_ext, d_ext_x, d_ext_value,
                                 d_ext_flux, d_status);
}

extern "C" int es_cylt_complex_eigenfunction(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                                             const double* d_w_im, int n, double* d_int_value, double* d_int_flux, int n_ext,
                                             double* d_ext_x, double* d_ext_value, double* d_ext_flux, uint8_t* d_status) {
  return eigenfunction<FAM_CYLT>(ctx, prob, d_k, d_w_re, d_w_im, n, d_int_value, d_int_flux, n_ext, d_ext_x, d_ext_value,
                                 d_ext_flux, d_status);
}
