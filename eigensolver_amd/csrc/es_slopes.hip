// Dispersion slopes of a (k, omega) pair: the boundary determinant D = outer - inner of es_shoot_eval_points together with its
// exact partial derivatives in omega and k (include/eigensolver_amd.h section 11).  Tangent-linear (forward-mode) evaluation:
// the node entries, coefficient sets, adjoint RK4 steps, closed-form exterior and boundary algebra of es_shoot_device.hpp,
// instantiated over 3-component jets (value, d/d omega, d/d k) -- the text the value kernels instantiate over double.  The
// jet type and the one-pair march are es_jet.hpp's (shared with the Newton kernel of es_newton.hip); this file holds the
// kernel, the launcher and the ABI entry.  One pair per lane; each lane stores once per output at the end.
#include "es_jet.hpp"

namespace {
using namespace es_shoot_shared;

template <int FAM>
__global__ __launch_bounds__(64) void root_slopes_kernel(ShootDev P, const double* __restrict__ kv,
                                                         const double* __restrict__ wv, int n,
                                                         const int32_t* __restrict__ d_count, double* __restrict__ outer,
                                                         double* __restrict__ inner, uint8_t* __restrict__ status) {
  const int cnt = es_count_clamped(d_count, n);                // n stays the row length of the [3][n] outputs
  if ((int)(blockIdx.x * blockDim.x) >= cnt) return;           // the whole wave lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < cnt;
  // not tracked: ES_PT_CONTINUUM is not looked at
  const JetMatch<2> M = jet_march<FAM, 2, false>(P, in ? kv[i] : 1.0, in ? wv[i] : 1.0);
  if (!in) return;
  const bool good = M.status == ES_PT_OK && jet_finite(M.outer) && jet_finite(M.inner);
  const Jet3 bad = jet_of<2>(NAN, [](int) { return NAN; });
  const Jet3 O = good ? M.outer : bad, J = good ? M.inner : bad;
  if (outer) {
    outer[i] = O.v;
    outer[(size_t)n + i] = O.d[0];
    outer[2 * (size_t)n + i] = O.d[1];
  }
  if (inner) {
    inner[i] = J.v;
    inner[(size_t)n + i] = J.d[0];
    inner[2 * (size_t)n + i] = J.d[1];
  }
  if (status) status[i] = (uint8_t)M.status;
}

template <int FAM>
int launch_slopes(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n, const int32_t* d_count,
                  double* d_outer, double* d_inner, uint8_t* d_status) {
  hipLaunchKernelGGL((root_slopes_kernel<FAM>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, d_k, d_w, n, d_count,
                     d_outer, d_inner, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace

extern "C" int es_shoot_root_slopes(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                                    const int32_t* d_count, double* d_outer, double* d_inner, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define ES_SLOPES(F) launch_slopes<F>(ctx, prob, d_k, d_w, n, d_count, d_outer, d_inner, d_status)
  ES_DISPATCH_FAMILY(prob->dev.family, ES_SLOPES)
#undef ES_SLOPES
}
