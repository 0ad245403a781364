// K14: complex-frequency determinant of the untwisted cylinder (FAM_CYL0: CylinderDensity, CylinderFlow; any m, both axis
// conditions, both r_sign) and its root search -- the unstable (Kelvin-Helmholtz) modes of a cylinder with axial flow.
// See include/eigensolver_amd.h section (14); the CPU restatement is tests/cyl_complex_model.py.
//
// Interior: the FAM_CYL0 formula text of es_shoot_device.hpp (make_entry, coef_pre, coef_finish, adjoint_start,
// rk4_step_adjoint<0>, boundary_algebra) instantiated with the complex scalar esb::cz, TRACK = false, the plain (not scaled,
// normalised) RK4 step, one IEEE complex division per node.  Nothing of the coefficient formulas is restated here.
// Exterior, written for the complex case (cyl_exterior): m_e and xi_e_const as exterior_cylinder, mu = principal sqrt(m_e),
// K_n and I_n at complex argument (es_bessel_complex.hpp), the same far-field initial values and I-admixture.  The solution is
// normalised by its own complex boundary value, P_e(boundary) = 1, where the real path divides by |P_v| and keeps the sign yb:
// on the real axis D_c = yb D.
// Status: ES_PT_LEAKY where Re m_e < 0 (the rule of the slab's complex path, and of the real path on the real axis; it keeps mu
// in the sector |arg mu| <= pi/4 the Bessel routines support); ES_PT_NONFINITE where m_e, xi_e_const or the result is not
// finite.  There is no continuum status: off the real axis the coefficients have no zero on the grid; on it, callers have
// the real path (es_shoot_eval_*).
// One (k, omega) point per lane; the base table is staged in LDS chunk by chunk (CH steps) and every lane forms its own
// node entries.  Every lane of a workgroup makes every barrier call: lanes past the count march on dummy inputs and store
// nothing.  Not on the benchmark path: written for clarity.
#include "es_bessel_complex.hpp"
#include "es_complex_roots.hpp"

namespace {
using namespace es_complex_shared;
using esb::cz;
constexpr int FAM = FAM_CYL0;
constexpr int NB = FamTraits<FAM>::NB;
constexpr int NE = FamTraits<FAM>::NE;
constexpr int CYLC_LDS_DOUBLES = NB * (2 * CH + 1);         // one chunk: nodes and mid-points of CH steps

// what boundary_algebra reads of an exterior
struct CylcExterior {
  cz outer;          // xi_e = xi_e_const P_e'(boundary) / P_e(boundary)
  double yb;         // P_e(boundary) after the normalisation: 1
  cz Oe;             // (flow slab only)
  int status;
};

__device__ __forceinline__ CylcExterior cyl_exterior(const ShootDev& P, double k, cz w) {
  CylcExterior X;
  const double k2 = k * k;
  const cz w2 = w * w;
  X.Oe = w;
  X.yb = 1.0;
  X.outer = cz(NAN, NAN);
  const cz m_e = ((k2 * P.vAe2 - w2) * (k2 * P.ce2 - w2)) / (P.Se * (k2 * P.cTe2 - w2));      // CF:699
  const cz cst = -1.0 / (P.rho_e * (k2 * P.vAe2 - w2));                                       // CF:702
  if (m_e.re < 0.0) { X.status = ES_PT_LEAKY; return X; }
  if (!esb::cz_finite(m_e) || !esb::cz_finite(cst)) { X.status = ES_PT_NONFINITE; return X; }
  X.status = ES_PT_OK;
  const cz mu = esb::cz_sqrt(m_e);
  const double sgn = (P.xb < 0.0) ? -1.0 : 1.0;
  const cz xR = mu * (P.R_factor / k), xb = mu;
  const int n = P.m_ext;
  const double dn = (double)n;
  cz Kb, Kb1, KR, KR1;
  esb::cke_pair(n, xb, Kb, Kb1);
  esb::cke_pair(n, xR, KR, KR1);
  const cz dKb = (dn / xb) * Kb - Kb1;               // e^z K_n'(z)
  const cz dKR = (dn / xR) * KR - KR1;
  const cz g = P.ic1 / (sgn * mu);
  // P = a I + b K with (a, b) from the far-field values; common factor xR e^{xR - xb} dropped
  cz Pv, dPv;
  const cz gap = xR - xb;
  if (gap.re < 40.0) {
    cz Ib, Ib1, IR, IR1;
    esb::cie_pair_from_k(n, xb, Kb, Kb1, Ib, Ib1);
    esb::cie_pair_from_k(n, xR, KR, KR1, IR, IR1);
    const cz dIb = Ib1 + (dn / xb) * Ib;             // e^-z I_n'(z)
    const cz dIR = IR1 + (dn / xR) * IR;
    const cz a_s = -(P.ic0 * dKR - g * KR);
    const cz b_s = -(g * IR - P.ic0 * dIR);
    const cz E2 = esb::cz_exp(-2.0 * gap);
    Pv = b_s * Kb + E2 * a_s * Ib;
    dPv = (sgn * mu) * (b_s * dKb + E2 * a_s * dIb);
  } else {
    // I-admixture below e^-80: only the K part is left and b cancels in the normalisation
    Pv = Kb;
    dPv = (sgn * mu) * dKb;
  }
  X.outer = cst * (dPv / Pv);
  if (!esb::cz_finite(X.outer)) X.status = ES_PT_NONFINITE;
  return X;
}

// Copies the base table of the nst steps from step c0 on (2 nst + 1 points, point-major) into the LDS buffer `sb`, between two
// barriers: every lane of the workgroup makes every call.
__device__ __forceinline__ void cyl_stage_chunk(const ShootDev& P, int c0, int nst, double* __restrict__ sb) {
  __syncthreads();
#pragma unroll
  for (int f = 0; f < NB; ++f)
    for (int i = threadIdx.x; i < 2 * nst + 1; i += blockDim.x) sb[i * NB + f] = P.base[(size_t)f * P.npts + 2 * c0 + i];
  __syncthreads();
}

// coefficients of the node whose base fields are at b
__device__ __forceinline__ CoefT<cz> cyl_node(const ShootDev& P, const KScalT<cz>& s, cz w, const double* __restrict__ bn, cz* e) {
  double b[NB], c[NE];
#pragma unroll
  for (int f = 0; f < NB; ++f) b[f] = bn[f];
  make_entry<FAM, false>(b, s, e, c);
  SignTrack trk;
  CoefPreT<cz> C;
  coef_pre<FAM, false>(e, c, P, s, w, C, trk);
  CoefT<cz> A;
  coef_finish<FAM>(C, 1.0 / C.den, A);
  return A;
}

// The two sides of the matching condition at (k, w): D_c = outer - inner, NaN unless st == ES_PT_OK.  P carries bc_const at
// its true scale (the launches pass bc_const_raw).  Every lane of the workgroup must call this.
__device__ __forceinline__ void cyl_shoot_point(const ShootDev& P, double k, cx wc, cx& D, cx& outer, cx& inner, double& rel,
                                                uint8_t& st, double* __restrict__ sb) {
  const cz w(wc.re, wc.im);
  const KScalT<cz> s = make_kscal(P, cz(k));
  const CylcExterior X = cyl_exterior(P, k, w);
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  cz e[NE];
  CoefT<cz> B0;
  cz zp(0.0), zq(0.0);
  const int nchunks = (nsteps + CH - 1) / CH;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int c0 = c * CH;
    const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
    cyl_stage_chunk(P, c0, nst, sb);
    if (c == nchunks - 1) {                            // last node: start vector of the march
      B0 = cyl_node(P, s, w, sb + 2 * nst * NB, e);
      adjoint_start<FAM>(P, B0, zp, zq);
    }
    for (int j = nst - 1; j >= 0; --j) {
      const CoefT<cz> Bm = cyl_node(P, s, w, sb + (2 * j + 1) * NB, e);
      const CoefT<cz> B1 = cyl_node(P, s, w, sb + (2 * j) * NB, e);
      rk4_step_adjoint<FamTraits<FAM>::SHAPE>(zp, zq, B0, Bm, B1, h, h2, h6, h3);
      B0 = B1;
    }
  }
  // e: the entries of the boundary node (read by the slab branches of boundary_algebra only)
  const MismatchT<cz> M = boundary_algebra<FAM>(P, s, w, X, zp, zq, e);
  st = (uint8_t)X.status;
  outer = cx{M.outer.re, M.outer.im};
  inner = cx{M.inner.re, M.inner.im};
  D = cx{M.d.re, M.d.im};
  const double sc = P.accept_norm ? cabs_(outer) : fmax(cabs_(outer), cabs_(inner));
  rel = cabs_(D) * 100.0 / sc;
  if (X.status == ES_PT_OK && !cfinite(D)) st = ES_PT_NONFINITE;
  if (st != ES_PT_OK) { D = cx{NAN, NAN}; outer = D; inner = D; rel = NAN; }
}

// grid (n_re > 0: index -> (row, i_im, i_re)) or point list (n_re == 0); outer_o / inner_o: interleaved complex, may be null
__global__ __launch_bounds__(256) void cylc_eval_kernel(ShootDev P, const double* __restrict__ kv,
                                                        const double* __restrict__ wre, const double* __restrict__ wim,
                                                        long n, int n_re, int n_im, int w_mode,
                                                        double* __restrict__ Dre, double* __restrict__ Dim,
                                                        double* __restrict__ relout, uint8_t* __restrict__ stout,
                                                        double* __restrict__ outer_o, double* __restrict__ inner_o) {
  __shared__ double sb[CYLC_LDS_DOUBLES];
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  double k = 1.0;
  cx w = cx{1.0, 0.1};
  if (in) {
    if (n_re > 0) {
      const long row = i / ((long)n_re * n_im);
      const long r = i - row * (long)n_re * n_im;
      const int iim = (int)(r / n_re), ire = (int)(r - (long)iim * n_re);
      k = kv[row];
      w = cx_pick_w(w_mode, k, wre[ire], wim[iim]);
    } else {
      k = kv[i];
      w = cx{wre[i], wim[i]};
    }
  }
  cx D, outer, inner; double rel; uint8_t st;
  cyl_shoot_point(P, k, w, D, outer, inner, rel, st, sb);
  if (in) {
    Dre[i] = D.re;
    Dim[i] = D.im;
    stout[i] = st;
    if (relout) relout[i] = rel;
    if (outer_o) { outer_o[2 * i] = outer.re; outer_o[2 * i + 1] = outer.im; }
    if (inner_o) { inner_o[2 * i] = inner.re; inner_o[2 * i + 1] = inner.im; }
  }
}

// complex secant iteration (cx_refine_candidate), one candidate per lane
__global__ __launch_bounds__(64) void cylc_refine_kernel(ShootDev P, es_complex_root_table tab,
                                                         const double* __restrict__ half_re,
                                                         const double* __restrict__ half_im, int n, int n_iter,
                                                         double tol_percent) {
  __shared__ double sb[CYLC_LDS_DOUBLES];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  cx_refine_candidate(
      [&](double k, cx w, cx& f, double& rel, uint8_t& st) {
        cx outer, inner;
        cyl_shoot_point(P, k, w, f, outer, inner, rel, st, sb);
      },
      tab, half_re, half_im, i, n, n_iter, tol_percent);
}

int check_cyl_cx(es_context* ctx, const es_problem* prob) {
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  if (prob->dev.family != FAM_CYL0) {
    ctx->last_error = "es_cyl_complex_* is implemented for ES_GEOM_CYLINDER problems only (the untwisted cylinder)";
    return ES_ERR_UNSUPPORTED;
  }
  return ES_SUCCESS;
}

// the problem as the complex march takes it: z at its true scale, so the target of the axis condition as given
ShootDev cyl_cx_dev(const es_problem* prob) {
  ShootDev P = prob->dev;
  P.bc_const = P.bc_const_raw;
  return P;
}

}  // namespace

extern "C" int es_cyl_complex_eval_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                        const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                                        double* d_D_re, double* d_D_im, double* d_rel, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, nk >= 0 && n_re >= 0 && n_im >= 0, "negative size");
  ES_REQUIRE(ctx, w_mode == ES_W_ABSOLUTE || w_mode == ES_W_PHASE_SPEED, "w_mode");
  const long n = (long)nk * n_re * n_im;
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_D_re && d_D_im && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cylc_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, cyl_cx_dev(prob), d_k,
                     d_w_re, d_w_im, n, n_re, n_im, w_mode, d_D_re, d_D_im, d_rel, d_status, (double*)nullptr,
                     (double*)nullptr);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_cyl_complex_eval_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                                          const double* d_w_im, int n, double* d_D_re, double* d_D_im, double* d_rel,
                                          uint8_t* d_status, double* d_outer, double* d_inner) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_D_re && d_D_im && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cylc_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, cyl_cx_dev(prob), d_k,
                     d_w_re, d_w_im, (long)n, 0, 0, ES_W_ABSOLUTE, d_D_re, d_D_im, d_rel, d_status, d_outer, d_inner);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_cyl_complex_find_roots(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                         const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                                         const double* d_D_re, const double* d_D_im, const uint8_t* d_status, int n_iter,
                                         double tol_percent, es_complex_root_table* table, int* out_count) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx(ctx, prob);
  if (rc) return rc;
  return cx_find_roots_host(ctx, d_k, nk, d_w_re, n_re, d_w_im, n_im, w_mode, d_D_re, d_D_im, d_status, n_iter, table, out_count,
                            [&](const es_complex_root_table& tab, const double* half_re, const double* half_im, int n) {
                              hipLaunchKernelGGL(cylc_refine_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream,
                                                 cyl_cx_dev(prob), tab, half_re, half_im, n, n_iter, tol_percent);
                            });
}
