// K14, K17: complex-frequency determinant of the cylinder and its root search -- the unstable (Kelvin-Helmholtz) modes of a
// cylinder with axial flow (FAM_CYL0: CylinderDensity, CylinderFlow; any m, both axis conditions, both r_sign; section 14 of
// include/eigensolver_amd.h, es_cyl_complex_*) and of a tube with azimuthal shear (FAM_CYLT: CylinderRotation; m >= 0, all
// three axis conditions, both values of c1_power; section 17, es_cylt_complex_*).  The CPU restatements are
// tests/cyl_complex_model.py and tests/cylt_complex_model.py.
//
// The evaluation itself -- interior, exterior, statuses, LDS staging -- is the text of es_cyl_complex_shared.hpp, here at the
// plain complex scalar esb::cz with the family as the kernels' template parameter: the seven fields and the off-diagonal RK4
// step of FAM_CYL0, the 20-field base table, 16 node entries and the full-shape step of FAM_CYLT.  The exterior is the same
// uniform medium for both: cyl_exterior as it is.  c1_power is read from the problem at run time (coef_pre, C1P = 0).
// es_cyl_complex_slopes.hip runs the same text over jets (sections 15 and 18).  One (k, omega) point per lane; every lane of a
// workgroup makes every barrier call: lanes past the count march on dummy inputs and store nothing.
// Not on the benchmark path: written for clarity.
#include "es_cyl_complex_shared.hpp"

namespace {
using namespace es_cyl_complex_shared;

// The evaluation at the plain complex scalar, as the kernels below take it: D_c = outer - inner, NaN unless st == ES_PT_OK.
// Every lane of the workgroup must call this.
template <int F>
__device__ __forceinline__ void cylc_point(const ShootDev& P, double k, cz w, cz& D, cz& outer, cz& inner, double& rel,
                                           uint8_t& st, double* __restrict__ sb) {
  const CylcMatch<cz> M = cyl_shoot_point<cz, double, F>(P, k, w, sb);
  st = M.st;
  rel = M.rel;
  outer = M.outer;
  inner = M.inner;
  D = M.outer - M.inner;
  if (st != ES_PT_OK) { D = cz(NAN, NAN); outer = D; inner = D; }
}

// grid (n_re > 0: index -> (row, i_im, i_re)) or point list (n_re == 0); outer_o / inner_o: interleaved complex, may be null
template <int F>
__global__ __launch_bounds__(256) void cylc_eval_kernel(ShootDev P, const double* __restrict__ kv,
                                                        const double* __restrict__ wre, const double* __restrict__ wim,
                                                        long n, int n_re, int n_im, int w_mode,
                                                        double* __restrict__ Dre, double* __restrict__ Dim,
                                                        double* __restrict__ relout, uint8_t* __restrict__ stout,
                                                        double* __restrict__ outer_o, double* __restrict__ inner_o) {
  __shared__ double sb[cyl_lds_doubles<F>()];                  // 7 (2 CH + 1) doubles: 14 392 B; FAM_CYLT 20 (2 CH + 1): 41 120 B
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
  cz D, outer, inner; double rel; uint8_t st;
  cylc_point<F>(P, k, w, D, outer, inner, rel, st, sb);
  if (in) {
    Dre[i] = D.re;
    Dim[i] = D.im;
    stout[i] = st;
    if (relout) relout[i] = rel;
    if (outer_o) { outer_o[2 * i] = outer.re; outer_o[2 * i + 1] = outer.im; }
    if (inner_o) { inner_o[2 * i] = inner.re; inner_o[2 * i + 1] = inner.im; }
  }
}

// Complex secant iteration (cx_refine_candidate), one candidate per lane.
// cylc_refine_kernel<FAM_CYLT> must spill no register, vector or scalar (tests/test_cyl_complex_codeobj.py).  It holds four
// inlined copies of the evaluation -- cx_refine_candidate calls it at four places -- and what they share would stay in scalar
// registers through all of them.  So (cyl_uniforms_in_vgprs) the wave-uniform arguments that count no barrier-carrying loop
// live in vector registers (one wave per SIMD: there is room), each copy derives its chunk and step counts from a scalar
// n_nodes of its own (cyl_own_counts), and lanes past the count evaluate one fixed dummy point, which keeps the mask of
// `i < n` in use in every copy.  Same operations on the same values.  n_nodes, n_iter and tol_percent stay scalar.  How the
// counts moved: DESIGN.md section 8l.
template <int F>
__global__ __launch_bounds__(64) void cylc_refine_kernel(ShootDev P, es_complex_root_table tab,
                                                         const double* __restrict__ half_re,
                                                         const double* __restrict__ half_im, int n, int n_iter,
                                                         double tol_percent) {
  __shared__ double sb[cyl_lds_doubles<F>()];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (cyl_uniforms_in_vgprs<F>) {
    vector_resident(P);
    ES_V(tab.d_k); ES_V(tab.d_w_re); ES_V(tab.d_w_im); ES_V(tab.d_resid); ES_V(tab.d_row); ES_V(tab.d_flag);
    ES_V(half_re); ES_V(half_im); ES_V(n);
  }
  cx_refine_candidate(
      [&](double k, cz w, cz& f, double& rel, uint8_t& st) {
        cz outer, inner;
        decltype(auto) Q = cyl_own_counts<F>(P);
        if constexpr (cyl_uniforms_in_vgprs<F>)
          if (!(i < n)) w = cz(1.0, 0.1);                      // past the count: the dummy point
        cylc_point<F>(Q, k, w, f, outer, inner, rel, st, sb);
      },
      tab, half_re, half_im, i, n, n_iter, tol_percent);
}

template <int F>
int eval_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk, const double* d_w_re, int n_re,
              const double* d_w_im, int n_im, int w_mode, double* d_D_re, double* d_D_im, double* d_rel, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx<F>(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, nk >= 0 && n_re >= 0 && n_im >= 0, "negative size");
  ES_REQUIRE(ctx, w_mode == ES_W_ABSOLUTE || w_mode == ES_W_PHASE_SPEED, "w_mode");
  const long n = (long)nk * n_re * n_im;
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_D_re && d_D_im && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cylc_eval_kernel<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, cyl_cx_dev(prob), d_k,
                     d_w_re, d_w_im, n, n_re, n_im, w_mode, d_D_re, d_D_im, d_rel, d_status, (double*)nullptr,
                     (double*)nullptr);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

template <int F>
int eval_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                double* d_D_re, double* d_D_im, double* d_rel, uint8_t* d_status, double* d_outer, double* d_inner) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx<F>(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_D_re && d_D_im && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cylc_eval_kernel<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, cyl_cx_dev(prob), d_k,
                     d_w_re, d_w_im, (long)n, 0, 0, ES_W_ABSOLUTE, d_D_re, d_D_im, d_rel, d_status, d_outer, d_inner);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

template <int F>
int find_roots(es_context* ctx, const es_problem* prob, const double* d_k, int nk, const double* d_w_re, int n_re,
               const double* d_w_im, int n_im, int w_mode, const double* d_D_re, const double* d_D_im, const uint8_t* d_status,
               int n_iter, double tol_percent, es_complex_root_table* table, int* out_count) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx<F>(ctx, prob);
  if (rc) return rc;
  return cx_find_roots_host(ctx, d_k, nk, d_w_re, n_re, d_w_im, n_im, w_mode, d_D_re, d_D_im, d_status, n_iter, table, out_count,
                            [&](const es_complex_root_table& tab, const double* half_re, const double* half_im, int n) {
                              hipLaunchKernelGGL(cylc_refine_kernel<F>, dim3((n + 63) / 64), dim3(64), 0, ctx->stream,
                                                 cyl_cx_dev(prob), tab, half_re, half_im, n, n_iter, tol_percent);
                            });
}

}  // namespace

extern "C" int es_cyl_complex_eval_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                        const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                                        double* d_D_re, double* d_D_im, double* d_rel, uint8_t* d_status) {
  return eval_grid<FAM_CYL0>(ctx, prob, d_k, nk, d_w_re, n_re, d_w_im, n_im, w_mode, d_D_re, d_D_im, d_rel, d_status);
}

extern "C" int es_cylt_complex_eval_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                         const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                                         double* d_D_re, double* d_D_im, double* d_rel, uint8_t* d_status) {
  return eval_grid<FAM_CYLT>(ctx, prob, d_k, nk, d_w_re, n_re, d_w_im, n_im, w_mode, d_D_re, d_D_im, d_rel, d_status);
}

extern "C" int es_cyl_complex_eval_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                                          const double* d_w_im, int n, double* d_D_re, double* d_D_im, double* d_rel,
                                          uint8_t* d_status, double* d_outer, double* d_inner) {
  return eval_points<FAM_CYL0>(ctx, prob, d_k, d_w_re, d_w_im, n, d_D_re, d_D_im, d_rel, d_status, d_outer, d_inner);
}

extern "C" int es_cylt_complex_eval_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                                           const double* d_w_im, int n, double* d_D_re, double* d_D_im, double* d_rel,
                                           uint8_t* d_status, double* d_outer, double* d_inner) {
  return eval_points<FAM_CYLT>(ctx, prob, d_k, d_w_re, d_w_im, n, d_D_re, d_D_im, d_rel, d_status, d_outer, d_inner);
}

extern "C" int es_cyl_complex_find_roots(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                         const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                                         const double* d_D_re, const double* d_D_im, const uint8_t* d_status, int n_iter,
                                         double tol_percent, es_complex_root_table* table, int* out_count) {
  return find_roots<FAM_CYL0>(ctx, prob, d_k, nk, d_w_re, n_re, d_w_im, n_im, w_mode, d_D_re, d_D_im, d_status, n_iter,
                              tol_percent, table, out_count);
}

extern "C" int es_cylt_complex_find_roots(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                          const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                                          const double* d_D_re, const double* d_D_im, const uint8_t* d_status, int n_iter,
                                          double tol_percent, es_complex_root_table* table, int* out_count) {
  return find_roots<FAM_CYLT>(ctx, prob, d_k, nk, d_w_re, n_re, d_w_im, n_im, w_mode, d_D_re, d_D_im, d_status, n_iter,
                              tol_percent, table, out_count);
}
