// K14: complex-frequency determinant of the untwisted cylinder (FAM_CYL0: CylinderDensity, CylinderFlow; any m, both axis
// conditions, both r_sign) and its root search -- the unstable (Kelvin-Helmholtz) modes of a cylinder with axial flow.
// See include/eigensolver_amd.h section (14); the CPU restatement is tests/cyl_complex_model.py.
//
// The evaluation itself -- interior, exterior, statuses, LDS staging -- is the text of es_cyl_complex_shared.hpp, here at the
// plain complex scalar esb::cz; es_cyl_complex_slopes.hip runs the same text over jets (section 15).  One (k, omega) point per
// lane; every lane of a workgroup makes every barrier call: lanes past the count march on dummy inputs and store nothing.
// Not on the benchmark path: written for clarity.
#include "es_cyl_complex_shared.hpp"

namespace {
using namespace es_cyl_complex_shared;

// The evaluation at the plain complex scalar, as the kernels below take it: D_c = outer - inner, NaN unless st == ES_PT_OK.
// Every lane of the workgroup must call this.
__device__ __forceinline__ void cyl_shoot_point(const ShootDev& P, double k, cx wc, cx& D, cx& outer, cx& inner, double& rel,
                                                uint8_t& st, double* __restrict__ sb) {
  const CylcMatch<cz> M = es_cyl_complex_shared::cyl_shoot_point<cz, double>(P, k, cz(wc.re, wc.im), sb);
  const cz d = M.outer - M.inner;
  st = M.st;
  rel = M.rel;
  outer = cx{M.outer.re, M.outer.im};
  inner = cx{M.inner.re, M.inner.im};
  D = cx{d.re, d.im};
  if (st != ES_PT_OK) { D = cx{NAN, NAN}; outer = D; inner = D; }
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
