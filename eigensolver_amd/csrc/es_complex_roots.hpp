// The root search of the complex-frequency determinants, written once for both geometries (include/eigensolver_amd.h sections
// 6, 14 and 17): the candidate cells (winding-number flags, ordered compaction, cell centres: the kernels live in es_complex.hip),
// the complex secant refinement over an evaluator, and the host side of a find_roots call.  The flow slab (es_complex.hip)
// and the cylinder (es_cyl_complex.hip, both families) differ in the evaluator of the refinement kernel and in their argument
// check only.  Beside it the Newton rule of sections 12, 15 and 18 (cx_newton_lane), over an evaluator in the same way:
// es_complex_slopes.hip and es_cyl_complex_slopes.hip.
#pragma once
#include "es_complex_shared.hpp"

namespace es_complex_shared {

__device__ __forceinline__ cz cx_pick_w(int w_mode, double k, double wre, double wim) {
  return (w_mode == ES_W_PHASE_SPEED) ? cz(k * wre, k * wim) : cz(wre, wim);
}

// Flags the cells around which D_c winds, scans, and writes k, row and the cell centre of the first min(total, capacity)
// flagged cells into the table, their half diagonals into ctx->d_scratch ([n] real parts, then [n] imaginary parts).
// *total: all flagged cells (read back: synchronises).  Defined in es_complex.hip.
int cx_candidates(es_context* ctx, const double* d_k, const double* d_w_re, int n_re, const double* d_w_im, int n_im,
                  int w_mode, long cells, const double* d_D_re, const double* d_D_im, const uint8_t* d_status,
                  const es_complex_root_table& table, int* total);

// Complex secant iteration for candidate i of n; uniform trip count (all lanes evaluate together): eval(k, w, f, rel, st) is
// the determinant at one point, f = NaN unless st == ES_PT_OK, and has barriers, so every lane of the workgroup makes every
// call (lanes past n iterate on dummy inputs and store nothing).
template <class Eval>
__device__ __forceinline__ void cx_refine_candidate(Eval eval, es_complex_root_table tab, const double* __restrict__ half_re,
                                                    const double* __restrict__ half_im, int i, int n, int n_iter,
                                                    double tol_percent) {
  const bool in = i < n;
  const double k = in ? tab.d_k[i] : 1.0;
  const cz centre = in ? cz(tab.d_w_re[i], tab.d_w_im[i]) : cz(1.0, 0.1);
  const cz half = in ? cz(half_re[i], half_im[i]) : cz(0.1, 0.1);
  cz w0 = centre, w1 = centre + 0.5 * half;
  cz f0, f1; double rel0, rel1; uint8_t s0, s1;
  eval(k, w0, f0, rel0, s0);
  eval(k, w1, f1, rel1, s1);
  for (int it = 0; it < n_iter; ++it) {
    const cz df = f1 - f0;
    cz w2 = w1 - f1 * ((w1 - w0) / df);
    if (!cz_finite(w2) || cz_abs2(df) == 0.0) w2 = w1;    // converged (f1 == f0) or broken: stay
    w0 = w1; f0 = f1;
    w1 = w2;
    eval(k, w1, f1, rel1, s1);
    if (!cz_finite(f1)) { w1 = w0; f1 = f0; }              // stepped onto a leaky / singular point: back off
  }
  // rel of the final iterate
  eval(k, w1, f1, rel1, s1);
  if (in) {
    const double dist2 = cz_abs2(w1 - centre), diag2 = 4.0 * cz_abs2(half);
    tab.d_w_re[i] = w1.re;
    tab.d_w_im[i] = w1.im;
    tab.d_resid[i] = rel1;
    tab.d_flag[i] = (s1 == ES_PT_OK && rel1 < tol_percent && dist2 <= 4.0 * diag2) ? 1 : 0;
  }
}

// What one evaluation hands the Newton rule: D_c with its derivatives in omega and k (Dk: the final evaluation only), rel in
// percent and the status.
struct CxNewtonPoint {
  cz D, Dw, Dk;
  double rel;
  uint8_t st;
};

// Newton in omega at fixed k for guess i of the workgroup's cnt (es_complex_newton, es_cyl_complex_newton,
// es_cylt_complex_newton).  step(k, w) is the evaluation with d/d omega, last(k, w) the one with d/dk as well; both have
// barriers, so every lane of the workgroup makes this call.  A lane that has stopped keeps evaluating at its frozen omega;
// the workgroup leaves the loop together once no lane is active.  Lanes past cnt iterate on dummy inputs and store nothing.
template <class Step, class Final>
__device__ __forceinline__ void cx_newton_lane(Step step, Final last, const double* __restrict__ kv,
                                               const double* __restrict__ gre, const double* __restrict__ gim, int i, int cnt,
                                               int max_iter, double step_cap, double max_shift, double tol_percent,
                                               double* __restrict__ wre, double* __restrict__ wim, double* __restrict__ resid,
                                               double* __restrict__ dwdk, int32_t* __restrict__ iters_out,
                                               int32_t* __restrict__ flag_out) {
  const bool in = i < cnt;
  const double k = in ? kv[i] : 1.0;
  const cz guess = in ? cz(gre[i], gim[i]) : cz(1.0, 0.1);
  cz w = guess;
  int iters = 0;
  bool ok = true, active = in;
  for (int it = 0; it < max_iter; ++it) {                      // max_iter is uniform: every lane reaches the vote
    const CxNewtonPoint E = step(k, w);
    if (active) {
      const cz D = E.D, Dw = E.Dw;
      if (E.st != ES_PT_OK || !cz_finite(D) || !cz_finite(Dw) || (Dw.re == 0.0 && Dw.im == 0.0)) {
        ok = false;
        active = false;
      } else {
        cz s = -(D / Dw);
        const double a = cz_abs(s);
        if (a > step_cap) s = (step_cap / a) * s;
        w = w + s;
        ++iters;
        if (cz_abs(s) <= 1e-14 * fmax(1.0, cz_abs(w))) active = false;
      }
    }
    if (!__syncthreads_or(active ? 1 : 0)) break;
  }
  const CxNewtonPoint E = last(k, w);
  if (!in) return;
  const bool good = E.st == ES_PT_OK;
  const cz slope = good ? -(E.Dk / E.Dw) : cz(NAN, NAN);
  wre[i] = w.re;
  wim[i] = w.im;
  resid[i] = E.rel;
  if (dwdk) {
    dwdk[2 * (size_t)i] = slope.re;
    dwdk[2 * (size_t)i + 1] = slope.im;
  }
  iters_out[i] = iters;
  flag_out[i] = (ok && good && E.rel < tol_percent && cz_abs(w - guess) <= max_shift) ? 1 : 0;
}

// Host side of a find_roots call after the problem was accepted.  launch_refine(table, half_re, half_im, n) enqueues the
// geometry's refinement kernel for the n candidates on ctx->stream.
template <class Launch>
int cx_find_roots_host(es_context* ctx, const double* d_k, int nk, const double* d_w_re, int n_re, const double* d_w_im,
                       int n_im, int w_mode, const double* d_D_re, const double* d_D_im, const uint8_t* d_status, int n_iter,
                       es_complex_root_table* table, int* out_count, Launch launch_refine) {
  ES_REQUIRE(ctx, table && out_count, "null pointer");
  ES_REQUIRE(ctx, nk >= 0 && n_re >= 0 && n_im >= 0 && n_iter >= 0 && n_iter <= 1000 && table->capacity >= 0, "size");
  ES_REQUIRE(ctx, w_mode == ES_W_ABSOLUTE || w_mode == ES_W_PHASE_SPEED, "w_mode");
  *out_count = 0;
  const long cells = (long)nk * n_re * n_im;
  if (cells == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im && d_D_re && d_D_im && d_status, "null pointer");
  ES_REQUIRE(ctx, table->capacity == 0 || (table->d_k && table->d_w_re && table->d_w_im && table->d_resid &&
                                           table->d_row && table->d_flag), "null root table arrays");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int total = 0;
  int rc = cx_candidates(ctx, d_k, d_w_re, n_re, d_w_im, n_im, w_mode, cells, d_D_re, d_D_im, d_status, *table, &total);
  if (rc) return rc;
  *out_count = total;
  const int n = total < table->capacity ? total : table->capacity;
  if (n > 0) {
    const double* half = (const double*)ctx->d_scratch;
    launch_refine(*table, half, half + n, n);
    ES_HIP_CHECK(ctx, hipGetLastError());
    ES_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return (total > table->capacity) ? ES_ERR_CAPACITY : ES_SUCCESS;
}

}  // namespace es_complex_shared
