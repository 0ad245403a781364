// Slopes and Newton tracing of complex roots of the flow slab (include/eigensolver_amd.h section 12): the two sides of the
// matching condition of es_complex_eval_points, outer and inner, with their exact derivatives in omega (holomorphic) and k.
// Tangent-linear (forward-mode) evaluation: the formulas of es_complex_shared.hpp at the scalar esb::CJet<2> (value,
// d/d omega, d/dk; the wavenumber the real pair esb::RealK (k, 1)) for the slopes and esb::CJet<1> (value, d/d omega; k a
// constant) for the Newton steps.  es_complex.hip runs the same text at esb::cz, so row 0 of outer - inner is the D_c of
// es_complex_eval_points bit for bit.
//
// One (k, omega) pair per lane, 64-thread workgroups, the profile table staged chunk by chunk in LDS (cx_stage_chunk):
// every lane of a workgroup reaches every barrier.  Lanes past the count march on dummy inputs and store nothing.
#include "es_complex_roots.hpp"

namespace {
using namespace es_complex_shared;
using esb::CJet;

// the evaluation at (value, d/d omega, d/dk)
__device__ __forceinline__ CxMatch<CJet<2>> cx_eval2(const ShootDev& P, int variant, double k, cz w, double* __restrict__ sb) {
  return cx_eval(P, variant, esb::RealK{k, 1.0}, esb::cjet_variable<2>(w, 0), sb);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cx_slopes_kernel(ShootDev P, int variant, const double* __restrict__ kv,
                                                       const double* __restrict__ wre, const double* __restrict__ wim, int n,
                                                       const int32_t* __restrict__ d_count, double* __restrict__ outer,
                                                       double* __restrict__ inner, uint8_t* __restrict__ status) {
  __shared__ double sb[CX_LDS_DOUBLES];
  const int cnt = es_count_clamped(d_count, n);                // n stays the row length of the [3][n][2] outputs
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole workgroup lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < cnt;
  const double k = in ? kv[i] : 1.0;
  const cz w = in ? cz(wre[i], wim[i]) : cz(1.0, 0.1);
  const CxMatch<CJet<2>> E = cx_eval2(P, variant, k, w, sb);
  if (!in) return;
  const bool good = E.st == ES_PT_OK && all_finite(E.outer) && all_finite(E.inner);
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

// Newton in omega at fixed k, one guess per lane: the rule of cx_newton_lane (es_complex_roots.hpp) over the slab's evaluation
// at CJet<1> (the steps) and CJet<2> (the final point).
__global__ __launch_bounds__(64) void cx_newton_kernel(ShootDev P, int variant, const double* __restrict__ kv,
                                                       const double* __restrict__ gre, const double* __restrict__ gim, int n,
                                                       const int32_t* __restrict__ d_count, int max_iter, double step_cap,
                                                       double max_shift, double tol_percent, double* __restrict__ wre,
                                                       double* __restrict__ wim, double* __restrict__ resid,
                                                       double* __restrict__ dwdk, int32_t* __restrict__ iters_out,
                                                       int32_t* __restrict__ flag_out) {
  __shared__ double sb[CX_LDS_DOUBLES];
  const int cnt = es_count_clamped(d_count, n);
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole workgroup lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  cx_newton_lane(
      [&](double k, cz w) {
        const CxMatch<CJet<1>> E = cx_eval(P, variant, k, esb::cjet_variable<1>(w, 0), sb);
        return CxNewtonPoint{E.outer.v - E.inner.v, E.outer.d[0] - E.inner.d[0], cz(0.0, 0.0), E.rel, E.st};
      },
      [&](double k, cz w) {
        const CxMatch<CJet<2>> E = cx_eval2(P, variant, k, w, sb);
        return CxNewtonPoint{E.outer.v - E.inner.v, E.outer.d[0] - E.inner.d[0], E.outer.d[1] - E.inner.d[1], E.rel, E.st};
      },
      kv, gre, gim, i, cnt, max_iter, step_cap, max_shift, tol_percent, wre, wim, resid, dwdk, iters_out, flag_out);
}

}  // namespace

extern "C" int es_complex_root_slopes(es_context* ctx, const es_problem* prob, int variant, const double* d_k,
                                      const double* d_w_re, const double* d_w_im, int n, const int32_t* d_count,
                                      double* d_outer, double* d_inner, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cx(ctx, prob, variant);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_w_im, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cx_slopes_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, variant, d_k, d_w_re,
                     d_w_im, n, d_count, d_outer, d_inner, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_complex_newton(es_context* ctx, const es_problem* prob, int variant, const double* d_k,
                                 const double* d_guess_re, const double* d_guess_im, int n, const int32_t* d_count,
                                 int max_iter, double step_cap, double max_shift, double tol_percent, double* d_w_re,
                                 double* d_w_im, double* d_resid, double* d_dwdk, int32_t* d_iters, int32_t* d_flag) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_cx(ctx, prob, variant);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  ES_REQUIRE(ctx, max_iter >= 0, "max_iter");
  ES_REQUIRE(ctx, step_cap > 0.0 && max_shift > 0.0 && tol_percent > 0.0, "step_cap, max_shift and tol_percent must be positive");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_guess_re && d_guess_im && d_w_re && d_w_im && d_resid && d_iters && d_flag, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cx_newton_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, variant, d_k, d_guess_re,
                     d_guess_im, n, d_count, max_iter, step_cap, max_shift, tol_percent, d_w_re, d_w_im, d_resid, d_dwdk,
                     d_iters, d_flag);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
