// Branch label of a (k, omega) pair: the number of sign changes of the interior eigenfunction rows, their maxima and where
// they sit (include/eigensolver_amd.h section 10).  What the reference's analysis scripts stand in for with hand-picked
// phase-speed cut-offs per data set (analysis_cylinder_flow_coronal.py:244-372: fast_sausage_branch1/2/3, slow_body_kink, ...).
// One (k, omega) pair per lane and the marches of interior_rows (es_interior_march.hpp), the function eigen_interior_kernel
// (es_eigenfunction.hip) calls too: the entries reduced here are the ones that kernel writes.  Nothing is written per node:
// four integers and two doubles per row pair live in registers and each lane stores once per output at the end.
#include "es_interior_march.hpp"

namespace {
using namespace es_shoot_shared;

// Running reduction of one row.  DOWN: the march visits the nodes N-1 ... 0 (cylinders: from the axis node out to the
// boundary), so a later entry has the smaller index and >= keeps the smallest index that attains the maximum; the count of
// sign changes does not depend on the direction.
struct RowTrack {
  double peak = -1.0;      // max |x| so far; no entry yet: below every |x|
  int node = -1;
  int last = 0;            // sign of the last entry kept, 0: none yet
  int changes = 0;
  template <bool DOWN>
  __device__ __forceinline__ void add(double x, int j) {
    const int s = (x > 0.0) - (x < 0.0);                       // 0 for +-0 and NaN: the entry is skipped
    changes += ((s * last) < 0) ? 1 : 0;
    last = s ? s : last;
    const double a = fabs(x);
    const bool up = DOWN ? (a >= peak) : (a > peak);           // a NaN compares false: skipped here too
    peak = up ? a : peak;
    node = up ? j : node;
  }
};

template <int FAM>
__global__ __launch_bounds__(64) void mode_signature_kernel(ShootDev P, const double* __restrict__ kv,
                                                            const double* __restrict__ wv, int n,
                                                            const int32_t* __restrict__ d_count,
                                                            int32_t* __restrict__ nodes_value, int32_t* __restrict__ nodes_flux,
                                                            int32_t* __restrict__ peak_node_value,
                                                            int32_t* __restrict__ peak_node_flux,
                                                            double* __restrict__ peak_value, double* __restrict__ peak_flux,
                                                            uint8_t* __restrict__ status) {
  constexpr bool CYL = (FAM == FAM_CYL0 || FAM == FAM_CYLT);
  n = es_count_clamped(d_count, n);
  if ((int)(blockIdx.x * blockDim.x) >= n) return;             // the whole wave lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const double k = in ? kv[i] : 1.0;
  const double w = in ? wv[i] : 1.0;
  const ExteriorLite X = exterior_lite(P, k, w, w);
  const bool ok = X.status == ES_PT_OK;
  RowTrack tv, tf;
  interior_rows<FAM>(P, k, w, X, [&](int node, double value, double f) {
    tv.add<CYL>(value, node);
    tf.add<CYL>(f, node);
  });
  if (!in) return;
  // one store per output and lane, lane i at entry i
  if (nodes_value) nodes_value[i] = ok ? tv.changes : -1;
  if (nodes_flux) nodes_flux[i] = ok ? tf.changes : -1;
  if (peak_node_value) peak_node_value[i] = ok ? tv.node : -1;
  if (peak_node_flux) peak_node_flux[i] = ok ? tf.node : -1;
  if (peak_value) peak_value[i] = (ok && tv.node >= 0) ? tv.peak : NAN;
  if (peak_flux) peak_flux[i] = (ok && tf.node >= 0) ? tf.peak : NAN;
  if (status) status[i] = (uint8_t)X.status;
}

template <int FAM>
int launch_signature(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                     const int32_t* d_count, int32_t* nv, int32_t* nf, int32_t* pnv, int32_t* pnf, double* pv, double* pf,
                     uint8_t* st) {
  hipLaunchKernelGGL((mode_signature_kernel<FAM>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, d_k, d_w, n,
                     d_count, nv, nf, pnv, pnf, pv, pf, st);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace

extern "C" int es_shoot_mode_signature(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                                       const int32_t* d_count, int32_t* d_nodes_value, int32_t* d_nodes_flux,
                                       int32_t* d_peak_node_value, int32_t* d_peak_node_flux, double* d_peak_value,
                                       double* d_peak_flux, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define ES_SIG(F) launch_signature<F>(ctx, prob, d_k, d_w, n, d_count, d_nodes_value, d_nodes_flux, d_peak_node_value, \
                                      d_peak_node_flux, d_peak_value, d_peak_flux, d_status)
  ES_DISPATCH_FAMILY(prob->dev.family, ES_SIG)
#undef ES_SIG
}
