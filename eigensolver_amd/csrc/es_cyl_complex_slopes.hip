// Slopes and Newton tracing of complex roots of the cylinder, untwisted (FAM_CYL0: include/eigensolver_amd.h section 15,
// es_cyl_complex_*) and twisted (FAM_CYLT: section 18, es_cylt_complex_*): the two sides of the matching condition of
// es_cyl(t)_complex_eval_points, outer and inner, with their exact derivatives in omega (holomorphic) and k.  Tangent-linear
// (forward-mode) evaluation: the text of es_cyl_complex_shared.hpp, with the family as the kernels' template parameter, at the
// scalar esb::CJet<2> (value, d/d omega, d/dk) for the slopes and esb::CJet<1> (value, d/d omega; k a constant) for the Newton
// steps.  es_cyl_complex.hip runs the same text at esb::cz, so row 0 is the value of sections 14 and 17.  c1_power of the
// twisted family is read from the problem at run time.  The Newton rule is cx_newton_lane of es_complex_roots.hpp, the one
// of the flow slab.
//
// One (k, omega) pair per lane, 64-thread workgroups, the base table (seven fields, 20 for FAM_CYLT) staged chunk by chunk in
// LDS (cyl_stage_chunk): every lane of a workgroup makes every barrier call.  Lanes past the count march on the dummy pair and
// store nothing; a workgroup that lies wholly past the count returns at once, a decision that is uniform across it.  Not on
// the benchmark path: a latency chain, written for clarity.
#include "es_cyl_complex_shared.hpp"

namespace {
using namespace es_cyl_complex_shared;
using esb::CJet;

// the evaluation at (value, d/d omega, d/dk)
template <int F>
__device__ __forceinline__ CylcMatch<CJet<2>> cyljet_eval2(const ShootDev& P, double k, cz w, double* __restrict__ sb) {
  return cyl_shoot_point<CJet<2>, CJet<2>, F>(P, esb::cjet_variable<2>(cz(k), 1), esb::cjet_variable<2>(w, 0), sb);
}

template <int F>
__global__ __launch_bounds__(64) void cyljet_slopes_kernel(ShootDev P, const double* __restrict__ kv,
                                                           const double* __restrict__ wre, const double* __restrict__ wim,
                                                           int n, const int32_t* __restrict__ d_count,
                                                           double* __restrict__ outer, double* __restrict__ inner,
                                                           uint8_t* __restrict__ status) {
  __shared__ double sb[cyl_lds_doubles<F>()];                  // 7 (2 CH + 1) doubles: 14 392 B; FAM_CYLT 20 (2 CH + 1): 41 120 B
  const int cnt = es_count_clamped(d_count, n);                // n stays the row length of the [3][n][2] outputs
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole workgroup lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < cnt;
  const double k = in ? kv[i] : 1.0;
  const cz w = in ? cz(wre[i], wim[i]) : cz(1.0, 0.1);
  const CylcMatch<CJet<2>> E = cyljet_eval2<F>(P, k, w, sb);
  if (!in) return;
  const bool good = E.st == ES_PT_OK;                          // covers a non-finite component of outer or inner
  const cz eo[3] = {E.outer.v, E.outer.d[0], E.outer.d[1]}, ei[3] = {E.inner.v, E.inner.d[0], E.inner.d[1]};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t o = 2 * ((size_t)c * n + i);
    if (outer) {
      outer[o] = good ? eo[c].re : NAN;
      outer[o + 1] = good ? eo[c].im : NAN;
    }
    if (inner) {
      inner[o] = good ? ei[c].re : NAN;
      inner[o + 1] = good ? ei[c].im : NAN;
    }
  }
  if (status) status[i] = E.st;
}

// Newton in omega at fixed k, one guess per lane: cx_newton_lane over the cylinder's evaluation at CJet<1> (the steps) and
// CJet<2> (the final point).
// cyljet_newton_kernel<FAM_CYLT> holds two inlined copies of the evaluation (CJet<1> in the loop, CJet<2> after it) under the
// loop and vote of cx_newton_lane, and as first written spilled 53 scalar registers to vector lanes.  The remedies are those of
// cylc_refine_kernel<FAM_CYLT> (es_cyl_complex.hip), under the same switch: the wave-uniform arguments that count no
// barrier-carrying loop live in vector registers (one wave per SIMD: there is room), each copy derives its chunk and step
// counts from a scalar n_nodes of its own, and lanes past the count are handed the fixed dummy pair inside the evaluator -- the
// value cx_newton_lane already gave them -- which keeps the mask of `i < cnt` in use in every copy.  Same operations on the
// same values.  n_nodes, max_iter and cnt stay scalar.  Six spilled scalar registers are left (a hoisted literal and the offset
// of the workgroup size among the implicit arguments, both held across the loop by the shared text);
// tests/test_cyl_complex_slopes_codeobj.py holds the kernel to that.  How the counts moved: DESIGN.md section 8m.
template <int F>
__global__ __launch_bounds__(64) void cyljet_newton_kernel(ShootDev P, const double* __restrict__ kv,
                                                           const double* __restrict__ gre, const double* __restrict__ gim,
                                                           int n, const int32_t* __restrict__ d_count, int max_iter,
                                                           double step_cap, double max_shift, double tol_percent,
                                                           double* __restrict__ wre, double* __restrict__ wim,
                                                           double* __restrict__ resid, double* __restrict__ dwdk,
                                                           int32_t* __restrict__ iters_out, int32_t* __restrict__ flag_out) {
  __shared__ double sb[cyl_lds_doubles<F>()];
  const int cnt = es_count_clamped(d_count, n);
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole workgroup lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (cyl_uniforms_in_vgprs<F>) {
    vector_resident(P);
    ES_V(kv); ES_V(gre); ES_V(gim); ES_V(step_cap); ES_V(max_shift); ES_V(tol_percent);
    ES_V(wre); ES_V(wim); ES_V(resid); ES_V(dwdk); ES_V(iters_out); ES_V(flag_out);
  }
  cx_newton_lane(
      [&](double k, cz w) {
        decltype(auto) Q = cyl_own_counts<F>(P);
        if constexpr (cyl_uniforms_in_vgprs<F>)
          if (!(i < cnt)) w = cz(1.0, 0.1);                    // past the count: the dummy pair
        const CylcMatch<CJet<1>> E = cyl_shoot_point<CJet<1>, double, F>(Q, k, esb::cjet_variable<1>(w, 0), sb);
        return CxNewtonPoint{E.outer.v - E.inner.v, E.outer.d[0] - E.inner.d[0], cz(0.0, 0.0), E.rel, E.st};
      },
      [&](double k, cz w) {
        decltype(auto) Q = cyl_own_counts<F>(P);
        if constexpr (cyl_uniforms_in_vgprs<F>)
          if (!(i < cnt)) w = cz(1.0, 0.1);
        const CylcMatch<CJet<2>> E = cyljet_eval2<F>(Q, k, w, sb);
        return CxNewtonPoint{E.outer.v - E.inner.v, E.outer.d[0] - E.inner.d[0], E.outer.d[1] - E.inner.d[1], E.rel, E.st};
      },
      kv, gre, gim, i, cnt, max_iter, step_cap, max_shift, tol_percent, wre, wim, resid, dwdk, iters_out, flag_out);
}

template <int F>
int root_slopes(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                const int32_t* d_count, double* d_outer, double* d_inner, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx<F>(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cyljet_slopes_kernel<F>, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, cyl_cx_dev(prob), d_k, d_w_re,
                     d_w_im, n, d_count, d_outer, d_inner, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

template <int F>
int newton(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_guess_re, const double* d_guess_im, int n,
           const int32_t* d_count, int max_iter, double step_cap, double max_shift, double tol_percent, double* d_w_re,
           double* d_w_im, double* d_resid, double* d_dwdk, int32_t* d_iters, int32_t* d_flag) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cyl_cx<F>(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  ES_REQUIRE(ctx, max_iter >= 0, "max_iter");
  ES_REQUIRE(ctx, step_cap > 0.0 && max_shift > 0.0 && tol_percent > 0.0, "step_cap, max_shift and tol_percent must be positive");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_guess_re && d_guess_im && d_w_re && d_w_im && d_resid && d_iters && d_flag, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cyljet_newton_kernel<F>, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, cyl_cx_dev(prob), d_k, d_guess_re,
                     d_guess_im, n, d_count, max_iter, step_cap, max_shift, tol_percent, d_w_re, d_w_im, d_resid, d_dwdk,
                     d_iters, d_flag);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace

extern "C" int es_cyl_complex_root_slopes(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                                          const double* d_w_im, int n, const int32_t* d_count, double* d_outer,
                                          double* d_inner, uint8_t* d_status) {
  return root_slopes<FAM_CYL0>(ctx, prob, d_k, d_w_re, d_w_im, n, d_count, d_outer, d_inner, d_status);
}

extern "C" int es_cylt_complex_root_slopes(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                                           const double* d_w_im, int n, const int32_t* d_count, double* d_outer,
                                           double* d_inner, uint8_t* d_status) {
  return root_slopes<FAM_CYLT>(ctx, prob, d_k, d_w_re, d_w_im, n, d_count, d_outer, d_inner, d_status);
}

extern "C" int es_cyl_complex_newton(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_guess_re,
                                     const double* d_guess_im, int n, const int32_t* d_count, int max_iter, double step_cap,
                                     double max_shift, double tol_percent, double* d_w_re, double* d_w_im, double* d_resid,
                                     double* d_dwdk, int32_t* d_iters, int32_t* d_flag) {
  return newton<FAM_CYL0>(ctx, prob, d_k, d_guess_re, d_guess_im, n, d_count, max_iter, step_cap, max_shift, tol_percent, d_w_re,
                          d_w_im, d_resid, d_dwdk, d_iters, d_flag);
}

extern "C" int es_cylt_complex_newton(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_guess_re,
                                      const double* d_guess_im, int n, const int32_t* d_count, int max_iter, double step_cap,
                                      double max_shift, double tol_percent, double* d_w_re, double* d_w_im, double* d_resid,
                                      double* d_dwdk, int32_t* d_iters, int32_t* d_flag) {
  return newton<FAM_CYLT>(ctx, prob, d_k, d_guess_re, d_guess_im, n, d_count, max_iter, step_cap, max_shift, tol_percent, d_w_re,
                          d_w_im, d_resid, d_dwdk, d_iters, d_flag);
}
