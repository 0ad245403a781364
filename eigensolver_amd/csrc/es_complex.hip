// K6: complex-frequency determinant of the flow slab, winding-number cell detection and complex secant refinement,
// eigenfunctions at given complex (k, omega).
// See include/eigensolver_amd.h section (6) for the reference lines this replaces and oracle/slab_complex.py for the
// CPU restatement.  The formulas (coefficients, exterior, adjoint march, boundary) are the text of es_complex_shared.hpp at
// the plain complex scalar esb::cz, the text es_complex_slopes.hip runs over jets; here are the kernels around them: one
// (k, omega) point per lane, the forward march of the eigenfunction, the winding-number flags and the secant refinement.
// The search is shared with the cylinder (es_cyl_complex.hip) through es_complex_roots.hpp: the flag and emit kernels live
// here behind cx_candidates, the refinement loop and the host side of a find_roots call are the header's.
#include "es_complex_roots.hpp"

namespace {
using namespace es_complex_shared;

// D_c = outer - inner at one point, NaN unless st == ES_PT_OK.  Every lane of the workgroup must call this.
__device__ __forceinline__ void cx_shoot_point(const ShootDev& P, int variant, double k, cz w, cz& D, double& rel,
                                               uint8_t& st, double* __restrict__ sb) {
  const CxMatch<cz> B = cx_eval(P, variant, k, w, sb);
  D = (B.st == ES_PT_OK) ? B.outer - B.inner : cz(NAN, NAN);
  rel = B.rel; st = B.st;
}

// grid (n_re > 0: index -> (row, i_im, i_re)) or point list (n_re == 0)
__global__ __launch_bounds__(256) void cx_eval_kernel(ShootDev P, int variant, const double* __restrict__ kv,
                                                      const double* __restrict__ wre, const double* __restrict__ wim,
                                                      long n, int n_re, int n_im, int w_mode,
                                                      double* __restrict__ Dre, double* __restrict__ Dim,
                                                      double* __restrict__ relout, uint8_t* __restrict__ stout) {
  __shared__ double sb[CX_LDS_DOUBLES];
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  double k = 1.0;
  cz w = cz(1.0, 0.1);
  if (in) {
    if (n_re > 0) {
      const long row = i / ((long)n_re * n_im);
      const long r = i - row * (long)n_re * n_im;
      const int iim = (int)(r / n_re), ire = (int)(r - (long)iim * n_re);
      k = kv[row];
      w = cx_pick_w(w_mode, k, wre[ire], wim[iim]);
    } else {
      k = kv[i];
      w = cz(wre[i], wim[i]);
    }
  }
  cz D; double rel; uint8_t st;
  cx_shoot_point(P, variant, k, w, D, rel, st, sb);
  if (in) {
    Dre[i] = D.re;
    Dim[i] = D.im;
    stout[i] = st;
    if (relout) relout[i] = rel;
  }
}

// ---- eigenfunctions at given (k, omega) -----------------------------------------------------------------------------
// rhs of the forward system: A y with A = [[0, 1], [a21, a22]]
__device__ __forceinline__ void cx_rhs_fwd(const CxNode<cz>& A, const cz& u, const cz& v, cz& ku, cz& kv) {
  ku = v;
  kv = A.a21 * u + A.a22 * v;
}

// One (k, omega) pair per lane: the adjoint march of cx_shoot_point gives the boundary state (Vb, sv) that meets the
// far-end condition, a forward RK4 march with the same coefficient sets writes (Vx, P_T) at every node.  val / flux are
// interleaved (re, im) pairs, [i * N + node].  Lanes with i >= n march on dummy inputs (barriers) and store nothing.
__global__ __launch_bounds__(64) void cx_eigen_interior_kernel(ShootDev P, int variant, const double* __restrict__ kv,
                                                               const double* __restrict__ wre,
                                                               const double* __restrict__ wim, int n,
                                                               double* __restrict__ val, double* __restrict__ flux,
                                                               uint8_t* __restrict__ stout) {
  constexpr int NB = CX_NB;
  __shared__ double sb[CX_LDS_DOUBLES];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const double k = in ? kv[i] : 1.0;
  const cz w = in ? cz(wre[i], wim[i]) : cz(1.0, 0.1);
  const CxConsts<double> C = cx_consts(P, variant, k);
  const CxOutside<cz> X = cx_exterior(P, C, w);
  // (1) the row of the transfer matrix picked by the far-end condition -> boundary state and status
  cz zp, zq;
  double Ub, dUb;
  cx_adjoint(P, C, w, sb, zp, zq, Ub, dUb);
  const CxMatch<cz> B = cx_boundary(P, C, X, w, zp, zq, Ub, dUb);
  const bool ok = B.st == ES_PT_OK;
  if (in) stout[i] = B.st;
  // (2) forward march from the boundary, writing every node
  cz u = B.Vb, v = B.sv;
  auto store = [&](int node, double U, double dU) {
    if (!in) return;
    const cz Om = w - k * U;
    const cz pt = cx_total_pressure(P, C, Om, Om * Om, dU, u, v);
    const size_t o = 2 * ((size_t)i * P.n_nodes + node);
    val[o] = ok ? u.re : NAN;
    val[o + 1] = ok ? u.im : NAN;
    flux[o] = ok ? pt.re : NAN;
    flux[o + 1] = ok ? pt.im : NAN;
  };
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  CxNode<cz> A0{cz(0.0), cz(0.0)};
  const int nchunks = (nsteps + CH - 1) / CH;
  for (int c = 0; c < nchunks; ++c) {
    const int c0 = c * CH;
    const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
    cx_stage_chunk(P, c0, nst, sb);
    if (c == 0) {
      A0 = cx_coef(C, w, sb[SF_U], sb[SF_DU], sb[SF_DDU]);
      store(0, sb[SF_U], sb[SF_DU]);
    }
    for (int j = 0; j < nst; ++j) {
      const double* bm = sb + (2 * j + 1) * NB;
      const double* b1 = sb + (2 * j + 2) * NB;
      const CxNode<cz> Am = cx_coef(C, w, bm[SF_U], bm[SF_DU], bm[SF_DDU]);
      const CxNode<cz> A1 = cx_coef(C, w, b1[SF_U], b1[SF_DU], b1[SF_DDU]);
      cz k1u, k1v, k2u, k2v, k3u, k3v, k4u, k4v;
      cx_rhs_fwd(A0, u, v, k1u, k1v);
      cx_rhs_fwd(Am, u + h2 * k1u, v + h2 * k1v, k2u, k2v);
      cx_rhs_fwd(Am, u + h2 * k2u, v + h2 * k2v, k3u, k3v);
      cx_rhs_fwd(A1, u + h * k3u, v + h * k3v, k4u, k4v);
      u = u + h6 * (k1u + k4u) + h3 * (k2u + k3u);
      v = v + h6 * (k1v + k4v) + h3 * (k2v + k3v);
      A0 = A1;
      store(c0 + j + 1, b1[SF_U], b1[SF_DU]);
    }
  }
}

// One (pair, exterior point) per lane: Vx_e and p_e Vx_e' in closed form per unit V_e(-1), so that the last point of a
// row is 1 + 0i and cx_exterior's `outer`.  st: the status the interior kernel wrote for the pair.
__global__ __launch_bounds__(256) void cx_eigen_exterior_kernel(ShootDev P, int variant, const double* __restrict__ kv,
                                                                const double* __restrict__ wre,
                                                                const double* __restrict__ wim, int n, int n_ext,
                                                                const uint8_t* __restrict__ st, double* __restrict__ xs,
                                                                double* __restrict__ val, double* __restrict__ flux) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)n * n_ext) return;
  const int i = (int)(t / n_ext), j = (int)(t - (long)i * n_ext);
  const double k = kv[i];
  const cz w = cz(wre[i], wim[i]);
  const CxOutside<cz> X = cx_exterior(P, cx_consts(P, variant, k), w);
  const cz mu = X.mu, gp = X.gp, gm = X.gm;
  // np.linspace(-R, -1, n_ext)[j]
  const double step = (-1.0 + X.R) / (double)(n_ext - 1);
  const double x = (j == n_ext - 1) ? -1.0 : -X.R + (double)j * step;
  const double ax = fabs(x);
  cz v = cz(NAN, NAN), f = cz(NAN, NAN);
  if (st[i] == ES_PT_OK) {
    const cz E2x = esb::cz_exp_sincos((-2.0 * (X.R - ax)) * mu);
    const cz dec = esb::cz_exp_sincos((-(ax - 1.0)) * mu);
    const cz den = gp + X.E2 * gm;
    v = dec * ((gp + E2x * gm) / den);
    f = X.p_e * (mu * (dec * ((gp - E2x * gm) / den)));                           // left_P = p_e_const * Vx'
  }
  xs[t] = x;
  val[2 * t] = v.re;
  val[2 * t + 1] = v.im;
  flux[2 * t] = f.re;
  flux[2 * t + 1] = f.im;
}

// ---- cells with a zero of D_c inside: winding number of D around the four corners ------------------------------
__device__ __forceinline__ int quadrant(double re, double im) { return (re >= 0.0) ? (im >= 0.0 ? 0 : 3) : (im >= 0.0 ? 1 : 2); }
// change of quadrant between consecutive corners as a signed quarter-turn count; +-2 is ambiguous -> reported as 8
__device__ __forceinline__ int quarter_turns(int qa, int qb) {
  const int d = (qb - qa) & 3;
  return d == 0 ? 0 : (d == 1 ? 1 : (d == 3 ? -1 : 8));
}

__global__ __launch_bounds__(256) void cx_flag_kernel(const double* __restrict__ Dre, const double* __restrict__ Dim,
                                                      const uint8_t* __restrict__ st, int n_re, int n_im, long cells,
                                                      uint64_t* __restrict__ masks, int* __restrict__ block_counts) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  bool flag = false;
  if (c < cells) {
    const long per_row = (long)n_re * n_im;
    const long r = c % per_row;
    const int iim = (int)(r / n_re), ire = (int)(r - (long)iim * n_re);
    if (ire < n_re - 1 && iim < n_im - 1) {
      const long c00 = c, c10 = c + 1, c11 = c + n_re + 1, c01 = c + n_re;      // counter-clockwise in (re, im)
      if (st[c00] == ES_PT_OK && st[c10] == ES_PT_OK && st[c11] == ES_PT_OK && st[c01] == ES_PT_OK) {
        const int q0 = quadrant(Dre[c00], Dim[c00]), q1 = quadrant(Dre[c10], Dim[c10]);
        const int q2 = quadrant(Dre[c11], Dim[c11]), q3 = quadrant(Dre[c01], Dim[c01]);
        const int t0 = quarter_turns(q0, q1), t1 = quarter_turns(q1, q2), t2 = quarter_turns(q2, q3), t3 = quarter_turns(q3, q0);
        const int total = t0 + t1 + t2 + t3;
        // +-4: one full turn (a simple zero / pole inside); an ambiguous half-turn edge: refine and let the secant decide
        flag = (total == 4 || total == -4 || total >= 6);
      }
    }
  }
  es_flag_block(flag, c, masks, block_counts);
}

__global__ __launch_bounds__(256) void cx_emit_kernel(const double* __restrict__ kv, const double* __restrict__ wre,
                                                      const double* __restrict__ wim, int n_re, int n_im, int w_mode,
                                                      long cells, const uint64_t* __restrict__ masks,
                                                      const int* __restrict__ block_off, es_complex_root_table tab,
                                                      double* __restrict__ half_re, double* __restrict__ half_im) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int pos = es_flagged_pos(masks, block_off, c, cells, tab.capacity);
  if (pos < 0) return;
  const long per_row = (long)n_re * n_im;
  const long row = c / per_row;
  const long r = c - row * per_row;
  const int iim = (int)(r / n_re), ire = (int)(r - (long)iim * n_re);
  const double k = kv[row];
  const cz a = cx_pick_w(w_mode, k, wre[ire], wim[iim]);
  const cz b = cx_pick_w(w_mode, k, wre[ire + 1], wim[iim + 1]);
  tab.d_k[pos] = k;
  tab.d_row[pos] = (int32_t)row;
  tab.d_w_re[pos] = 0.5 * (a.re + b.re);                   // cell centre: start of the refinement
  tab.d_w_im[pos] = 0.5 * (a.im + b.im);
  half_re[pos] = 0.5 * (b.re - a.re);
  half_im[pos] = 0.5 * (b.im - a.im);
}

// complex secant iteration (cx_refine_candidate), one candidate per lane
__global__ __launch_bounds__(64) void cx_refine_kernel(ShootDev P, int variant, es_complex_root_table tab,
                                                       const double* __restrict__ half_re,
                                                       const double* __restrict__ half_im, int n, int n_iter,
                                                       double tol_percent) {
  __shared__ double sb[CX_LDS_DOUBLES];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  cx_refine_candidate([&](double k, cz w, cz& f, double& rel, uint8_t& st) { cx_shoot_point(P, variant, k, w, f, rel, st, sb); },
                      tab, half_re, half_im, i, n, n_iter, tol_percent);
}

}  // namespace

int es_complex_shared::cx_candidates(es_context* ctx, const double* d_k, const double* d_w_re, int n_re, const double* d_w_im,
                                     int n_im, int w_mode, long cells, const double* d_D_re, const double* d_D_im,
                                     const uint8_t* d_status, const es_complex_root_table& table, int* total) {
  int rc = es_ensure_scan_scratch(ctx, (size_t)cells);
  if (rc) return rc;
  const int nblocks = (int)((cells + 255) / 256);
  hipLaunchKernelGGL(cx_flag_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, d_D_re, d_D_im, d_status, n_re, n_im,
                     cells, ctx->d_masks, ctx->d_block_counts);
  ES_HIP_CHECK(ctx, hipGetLastError());
  rc = es_scan_block_counts(ctx, nblocks, total);
  if (rc) return rc;
  const int n = *total < table.capacity ? *total : table.capacity;
  if (n > 0) {
    rc = es_ensure_scratch(ctx, 2 * (size_t)n * sizeof(double));
    if (rc) return rc;
    double* half = (double*)ctx->d_scratch;
    hipLaunchKernelGGL(cx_emit_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, d_k, d_w_re, d_w_im, n_re, n_im,
                       w_mode, cells, ctx->d_masks, ctx->d_block_counts, table, half, half + n);
  }
  return ES_SUCCESS;
}

extern "C" int es_complex_eval_grid(es_context* ctx, const es_problem* prob, int variant, const double* d_k, int nk,
                                    const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                                    double* d_D_re, double* d_D_im, double* d_rel, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cx(ctx, prob, variant);
  if (rc) return rc;
  ES_REQUIRE(ctx, nk >= 0 && n_re >= 0 && n_im >= 0, "negative size");
  ES_REQUIRE(ctx, w_mode == ES_W_ABSOLUTE || w_mode == ES_W_PHASE_SPEED, "w_mode");
  const long n = (long)nk * n_re * n_im;
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_D_re && d_D_im && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cx_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, prob->dev, variant,
                     d_k, d_w_re, d_w_im, n, n_re, n_im, w_mode, d_D_re, d_D_im, d_rel, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_complex_eval_points(es_context* ctx, const es_problem* prob, int variant, const double* d_k,
                                      const double* d_w_re, const double* d_w_im, int n, double* d_D_re,
                                      double* d_D_im, double* d_rel, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cx(ctx, prob, variant);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_D_re && d_D_im && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cx_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, prob->dev, variant,
                     d_k, d_w_re, d_w_im, (long)n, 0, 0, ES_W_ABSOLUTE, d_D_re, d_D_im, d_rel, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_complex_find_roots(es_context* ctx, const es_problem* prob, int variant, const double* d_k, int nk,
                                     const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                                     const double* d_D_re, const double* d_D_im, const uint8_t* d_status, int n_iter,
                                     double tol_percent, es_complex_root_table* table, int* out_count) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cx(ctx, prob, variant);
  if (rc) return rc;
  return cx_find_roots_host(ctx, d_k, nk, d_w_re, n_re, d_w_im, n_im, w_mode, d_D_re, d_D_im, d_status, n_iter, table, out_count,
                            [&](const es_complex_root_table& tab, const double* half_re, const double* half_im, int n) {
                              hipLaunchKernelGGL(cx_refine_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev,
                                                 variant, tab, half_re, half_im, n, n_iter, tol_percent);
                            });
}

extern "C" int es_complex_eigenfunction(es_context* ctx, const es_problem* prob, int variant, const double* d_k,
                                        const double* d_w_re, const double* d_w_im, int n, double* d_int_value,
                                        double* d_int_flux, int n_ext, double* d_ext_x, double* d_ext_value,
                                        double* d_ext_flux, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cx(ctx, prob, variant);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0 && n_ext >= 0, "negative size");
  ES_REQUIRE(ctx, n_ext == 0 || n_ext >= 2, "n_ext must be 0 or >= 2");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_int_value && d_int_flux, "null pointer");
  ES_REQUIRE(ctx, n_ext == 0 || (d_ext_x && d_ext_value && d_ext_flux), "null exterior arrays");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!d_status) {                                          // the exterior kernel reads the status of the interior march
    rc = es_ensure_scratch(ctx, (size_t)n);
    if (rc) return rc;
    d_status = (uint8_t*)ctx->d_scratch;
  }
  hipLaunchKernelGGL(cx_eigen_interior_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, variant, d_k,
                     d_w_re, d_w_im, n, d_int_value, d_int_flux, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  if (n_ext > 0) {
    const long tot = (long)n * n_ext;
    hipLaunchKernelGGL(cx_eigen_exterior_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream,
                       prob->dev, variant, d_k, d_w_re, d_w_im, n, n_ext, d_status, d_ext_x, d_ext_value, d_ext_flux);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  return ES_SUCCESS;
}
