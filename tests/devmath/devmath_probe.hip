// Test-only device build of the math header (eigensolver_amd/csrc/es_bessel.hpp): one (order, argument) per thread, so that
// the paths the header takes only inside __HIP_DEVICE_COMPILE__ -- qdiv on v_rcp_f64, the __constant__ reciprocal and
// Chebyshev tables, the device log / exp / sqrt -- can be measured against correctly rounded values
// (tests/test_devmath_gpu.py, tests/golden/bessel_truth.npz).  Compiled by eigensolver_amd/build.py with the library's flags
// into eigensolver_amd/lib/libes_devmath_probe.so; never loaded by the package.
//
// Every launcher takes device pointers and a stream, returns the hipError_t of the launch and does not synchronise.
// d_n == nullptr: every thread evaluates order n_all, a kernel argument -- wave-uniform, as in the product, where the
// order is a field of the problem; otherwise thread i evaluates order d_n[i] (loops of different lengths in one wave).
#include <hip/hip_runtime.h>

#include "../../eigensolver_amd/csrc/es_bessel.hpp"

namespace {
constexpr int kThreads = 256;

template <bool UNIFORM>
__global__ __launch_bounds__(kThreads) void ke_pair_kernel(const int* __restrict__ nv, int n_all, const double* __restrict__ x,
                                                           int count, double* __restrict__ o0, double* __restrict__ o1) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  double a, b;
  esb::ke_pair(UNIFORM ? n_all : nv[i], x[i], a, b);
  o0[i] = a; o1[i] = b;
}

template <bool UNIFORM>
__global__ __launch_bounds__(kThreads) void ie_pair_kernel(const int* __restrict__ nv, int n_all, const double* __restrict__ x,
                                                           int count, double* __restrict__ o0, double* __restrict__ o1) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  double a, b;
  esb::ie_pair(UNIFORM ? n_all : nv[i], x[i], a, b);
  o0[i] = a; o1[i] = b;
}

// fed by ke_pair at the same argument, as the exterior solution does
template <bool UNIFORM>
__global__ __launch_bounds__(kThreads) void ie_pair_from_k_kernel(const int* __restrict__ nv, int n_all,
                                                                  const double* __restrict__ x, int count,
                                                                  double* __restrict__ o0, double* __restrict__ o1) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const int n = UNIFORM ? n_all : nv[i];
  double kn, kn1, a, b;
  esb::ke_pair(n, x[i], kn, kn1);
  esb::ie_pair_from_k(n, x[i], kn, kn1, a, b);
  o0[i] = a; o1[i] = b;
}

template <bool UNIFORM>
__global__ __launch_bounds__(kThreads) void jy_pair_kernel(const int* __restrict__ nv, int n_all, const double* __restrict__ x,
                                                           int count, double* __restrict__ o0, double* __restrict__ o1,
                                                           double* __restrict__ o2, double* __restrict__ o3) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  double j0, j1, y0, y1;
  esb::jy_pair(UNIFORM ? n_all : nv[i], x[i], j0, j1, y0, y1);
  o0[i] = j0; o1[i] = j1; o2[i] = y0; o3[i] = y1;
}

__global__ __launch_bounds__(kThreads) void qdiv_kernel(const double* __restrict__ a, const double* __restrict__ b, int count,
                                                        double* __restrict__ o) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  o[i] = esb::qdiv(a[i], b[i]);
}

inline dim3 blocks(int count) { return dim3((unsigned)((count + kThreads - 1) / kThreads)); }
}  // namespace

#define DM_LAUNCH2(KERNEL)                                                                                            \
  if (count <= 0) return 0;                                                                                           \
  if (d_n) hipLaunchKernelGGL((KERNEL<false>), blocks(count), dim3(kThreads), 0, stream, d_n, 0, d_x, count, d_o0, d_o1); \
  else hipLaunchKernelGGL((KERNEL<true>), blocks(count), dim3(kThreads), 0, stream, d_n, n_all, d_x, count, d_o0, d_o1);  \
  return (int)hipGetLastError();

extern "C" {
int dm_ke_pair(const int* d_n, int n_all, const double* d_x, int count, double* d_o0, double* d_o1, hipStream_t stream) {
  DM_LAUNCH2(ke_pair_kernel)
}
int dm_ie_pair(const int* d_n, int n_all, const double* d_x, int count, double* d_o0, double* d_o1, hipStream_t stream) {
  DM_LAUNCH2(ie_pair_kernel)
}
int dm_ie_pair_from_k(const int* d_n, int n_all, const double* d_x, int count, double* d_o0, double* d_o1, hipStream_t stream) {
  DM_LAUNCH2(ie_pair_from_k_kernel)
}
int dm_jy_pair(const int* d_n, int n_all, const double* d_x, int count, double* d_o0, double* d_o1, double* d_o2,
               double* d_o3, hipStream_t stream) {
  if (count <= 0) return 0;
  if (d_n) hipLaunchKernelGGL((jy_pair_kernel<false>), blocks(count), dim3(kThreads), 0, stream, d_n, 0, d_x, count, d_o0, d_o1, d_o2, d_o3);
  else hipLaunchKernelGGL((jy_pair_kernel<true>), blocks(count), dim3(kThreads), 0, stream, d_n, n_all, d_x, count, d_o0, d_o1, d_o2, d_o3);
  return (int)hipGetLastError();
}
int dm_qdiv(const double* d_a, const double* d_b, int count, double* d_o, hipStream_t stream) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(qdiv_kernel, blocks(count), dim3(kThreads), 0, stream, d_a, d_b, count, d_o);
  return (int)hipGetLastError();
}
}
