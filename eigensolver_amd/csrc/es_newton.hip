// Newton tracing of real dispersion roots (include/eigensolver_amd.h section 13): from one guess per lane, Newton's iteration in
// omega at fixed k on the determinant D = outer - inner of es_shoot_eval_points, with the exact D_w of the jet march of
// es_jet.hpp -- the rule of es_complex_newton (section 12) in real arithmetic.  The steps run at jet width ND = 1 (value,
// d/d omega; k is a constant), the final evaluation at ND = 2, which also gives d omega / dk = -D_k / D_w, and looks at the
// continuum the way shoot_point does: phase-speed bands where the problem has them, sign tracking through the march otherwise.
//
// One guess per lane, 64-lane workgroups.  The march reads the node base fields by scalar loads (wave-uniform addresses, also
// under divergence); nothing is staged in LDS and there is no barrier, so a lane that has stopped simply goes inactive and a
// wave ends with its slowest lane.  (Whether an LDS-staged march with a workgroup vote, as cx_newton_kernel, is faster at one
// wave per SIMD or fewer has not been measured: es_shoot_shared.hpp, shoot_point_impl.)
#include "es_jet.hpp"

namespace {
using namespace es_shoot_shared;

template <int FAM>
__global__ __launch_bounds__(64) void root_newton_kernel(ShootDev P, const double* __restrict__ kv,
                                                         const double* __restrict__ gv, int n,
                                                         const int32_t* __restrict__ d_count, int max_iter, double step_cap,
                                                         double max_shift, double tol_percent, double* __restrict__ w_out,
                                                         double* __restrict__ resid, double* __restrict__ dwdk,
                                                         int32_t* __restrict__ iters_out, int32_t* __restrict__ flag_out,
                                                         uint8_t* __restrict__ status) {
  const int cnt = es_count_clamped(d_count, n);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;                                        // no barrier below: lanes past the count leave at once
  const double k = kv[i], guess = gv[i];
  double w = guess;
  int iters = 0;
  bool ok = true;
  for (int it = 0; it < max_iter; ++it) {
    const JetMatch<1> E = jet_march<FAM, 1, false>(P, k, w);
    const double D = E.outer.v - E.inner.v, Dw = E.outer.d[0] - E.inner.d[0];
    if (E.status != ES_PT_OK || !isfinite(D) || !isfinite(Dw) || Dw == 0.0) {
      ok = false;
      break;
    }
    double s = -D / Dw;
    if (fabs(s) > step_cap) s = copysign(step_cap, s);
    w += s;
    ++iters;
    if (fabs(s) <= 1e-14 * fabs(w)) break;             // relative alone: an absolute floor would tie the rule to one unit system
  }
  // the final point: slopes in both variables, and the status es_shoot_eval_points gives the pair
  JetMatch<2> E;
  bool crossed;
  if (fam_has_bands<FAM>() && P.use_bands) {
    E = jet_march<FAM, 2, false>(P, k, w);
    crossed = band_crossed(P, k, w);
  } else {
    E = jet_march<FAM, 2, true>(P, k, w);
    crossed = E.crossed;
  }
  Mismatch M;
  M.outer = E.outer.v;
  M.inner = E.inner.v;
  M.d = E.outer.v - E.inner.v;
  ExteriorLite X;
  X.status = E.status;
  double D, rel;
  uint8_t st;
  finish_point(P, M, X, crossed, D, rel, st);
  const bool has_value = st == ES_PT_OK || st == ES_PT_CONTINUUM;
  w_out[i] = w;
  resid[i] = has_value ? rel : NAN;
  if (dwdk) dwdk[i] = has_value ? -(E.outer.d[1] - E.inner.d[1]) / (E.outer.d[0] - E.inner.d[0]) : NAN;
  iters_out[i] = iters;
  flag_out[i] = (ok && st == ES_PT_OK && rel < tol_percent && fabs(w - guess) <= max_shift) ? 1 : 0;
  if (status) status[i] = st;
}

template <int FAM>
int launch_newton(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_guess, int n,
                  const int32_t* d_count, int max_iter, double step_cap, double max_shift, double tol_percent, double* d_w,
                  double* d_resid, double* d_dwdk, int32_t* d_iters, int32_t* d_flag, uint8_t* d_status) {
  hipLaunchKernelGGL((root_newton_kernel<FAM>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, d_k, d_guess, n,
                     d_count, max_iter, step_cap, max_shift, tol_percent, d_w, d_resid, d_dwdk, d_iters, d_flag, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace

extern "C" int es_shoot_newton(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_guess, int n,
                               const int32_t* d_count, int max_iter, double step_cap, double max_shift, double tol_percent,
                               double* d_w, double* d_resid, double* d_dwdk, int32_t* d_iters, int32_t* d_flag,
                               uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, n >= 0, "negative size");
  ES_REQUIRE(ctx, max_iter >= 0, "max_iter");
  ES_REQUIRE(ctx, step_cap > 0.0 && max_shift > 0.0 && tol_percent > 0.0, "step_cap, max_shift and tol_percent must be positive");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_guess && d_w && d_resid && d_iters && d_flag, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define ES_NEWTON(F) launch_newton<F>(ctx, prob, d_k, d_guess, n, d_count, max_iter, step_cap, max_shift, tol_percent, d_w, \
                                      d_resid, d_dwdk, d_iters, d_flag, d_status)
  ES_DISPATCH_FAMILY(prob->dev.family, ES_NEWTON)
#undef ES_NEWTON
}
