// Test-only device build of the math headers (eigensolver_amd/csrc/es_bessel.hpp, es_bessel_complex.hpp, es_cjet.hpp): one
// (order, argument) per thread, so that the paths the headers take only inside __HIP_DEVICE_COMPILE__ -- qdiv on v_rcp_f64,
// the __constant__ reciprocal and Chebyshev tables, the device log / exp / sqrt / hypot / atan2 / sin / cos -- can be measured
// against correctly rounded values (tests/test_devmath_gpu.py, tests/golden/bessel_truth.npz, bessel_complex_truth.npz).
// Compiled by eigensolver_amd/build.py with the library's flags into eigensolver_amd/lib/libes_devmath_probe.so; never loaded
// by the package.
//
// Every launcher takes device pointers and a stream, returns the hipError_t of the launch and does not synchronise.
// d_n == nullptr: every thread evaluates order n_all, a kernel argument -- wave-uniform, as in the product, where the
// order is a field of the problem; otherwise thread i evaluates order d_n[i] (loops of different lengths in one wave).
// Complex arrays are interleaved (re, im) pairs of doubles.
#include <hip/hip_runtime.h>

#include "../../eigensolver_amd/csrc/es_bessel.hpp"
#include "../../eigensolver_amd/csrc/es_cjet.hpp"

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

// ---- complex argument: es_bessel_complex.hpp, es_cjet.hpp ------------------------------------------------------------------------
__device__ __forceinline__ esb::cz cz_at(const double* __restrict__ z, int i) { return esb::cz(z[2 * i], z[2 * i + 1]); }
__device__ __forceinline__ void cz_put(double* __restrict__ o, int i, esb::cz a) { o[2 * i] = a.re; o[2 * i + 1] = a.im; }

template <bool UNIFORM>
__global__ __launch_bounds__(kThreads) void cke_pair_kernel(const int* __restrict__ nv, int n_all, const double* __restrict__ z,
                                                            int count, double* __restrict__ o0, double* __restrict__ o1) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  esb::cz a, b;
  esb::cke_pair(UNIFORM ? n_all : nv[i], cz_at(z, i), a, b);
  cz_put(o0, i, a); cz_put(o1, i, b);
}

// fed by cke_pair at the same argument, as the exterior solution does
template <bool UNIFORM>
__global__ __launch_bounds__(kThreads) void cie_pair_from_k_kernel(const int* __restrict__ nv, int n_all,
                                                                   const double* __restrict__ z, int count,
                                                                   double* __restrict__ o0, double* __restrict__ o1) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const int n = UNIFORM ? n_all : nv[i];
  esb::cz kn, kn1, a, b;
  esb::cke_pair(n, cz_at(z, i), kn, kn1);
  esb::cie_pair_from_k(n, cz_at(z, i), kn, kn1, a, b);
  cz_put(o0, i, a); cz_put(o1, i, b);
}

// the CJet<1> forms with z the variable: o0, o1 the value components, d0, d1 the derivatives in z
template <bool UNIFORM>
__global__ __launch_bounds__(kThreads) void cke_pair_jet_kernel(const int* __restrict__ nv, int n_all, const double* __restrict__ z,
                                                                int count, double* __restrict__ o0, double* __restrict__ o1,
                                                                double* __restrict__ d0, double* __restrict__ d1) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  esb::CJet<1> K, K1;
  esb::cke_pair(UNIFORM ? n_all : nv[i], esb::cjet_variable<1>(cz_at(z, i), 0), K, K1);
  cz_put(o0, i, K.v); cz_put(o1, i, K1.v); cz_put(d0, i, K.d[0]); cz_put(d1, i, K1.d[0]);
}

template <bool UNIFORM>
__global__ __launch_bounds__(kThreads) void cie_pair_from_k_jet_kernel(const int* __restrict__ nv, int n_all,
                                                                       const double* __restrict__ z, int count,
                                                                       double* __restrict__ o0, double* __restrict__ o1,
                                                                       double* __restrict__ d0, double* __restrict__ d1) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const int n = UNIFORM ? n_all : nv[i];
  const esb::CJet<1> Z = esb::cjet_variable<1>(cz_at(z, i), 0);
  esb::CJet<1> K, K1, I, I1;
  esb::cke_pair(n, Z, K, K1);
  esb::cie_pair_from_k(n, Z, K, K1, I, I1);
  cz_put(o0, i, I.v); cz_put(o1, i, I1.v); cz_put(d0, i, I.d[0]); cz_put(d1, i, I1.d[0]);
}

// the primitives of the complex scalar; OP: 0 cz_sqrt(b), 1 cz_log(b), 2 cz_exp(b), 3 a / b, 4 Re a / b (a: a real array)
template <int OP>
__global__ __launch_bounds__(kThreads) void cz_primitive_kernel(const double* __restrict__ a, const double* __restrict__ b, int count,
                                                                double* __restrict__ o) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const esb::cz zb = cz_at(b, i);
  esb::cz r;
  if (OP == 0) r = esb::cz_sqrt(zb);
  else if (OP == 1) r = esb::cz_log(zb);
  else if (OP == 2) r = esb::cz_exp(zb);
  else if (OP == 3) r = cz_at(a, i) / zb;
  else r = a[i] / zb;
  cz_put(o, i, r);
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

// ---- complex argument; d_z, d_o*, d_d*: complex arrays of `count` (2 count doubles) -----------------------------------------------
int dm_cke_pair(const int* d_n, int n_all, const double* d_x, int count, double* d_o0, double* d_o1, hipStream_t stream) {
  DM_LAUNCH2(cke_pair_kernel)
}
int dm_cie_pair_from_k(const int* d_n, int n_all, const double* d_x, int count, double* d_o0, double* d_o1, hipStream_t stream) {
  DM_LAUNCH2(cie_pair_from_k_kernel)
}
#define DM_LAUNCH4(KERNEL)                                                                                                      \
  if (count <= 0) return 0;                                                                                                     \
  if (d_n) hipLaunchKernelGGL((KERNEL<false>), blocks(count), dim3(kThreads), 0, stream, d_n, 0, d_x, count, d_o0, d_o1, d_d0, d_d1); \
  else hipLaunchKernelGGL((KERNEL<true>), blocks(count), dim3(kThreads), 0, stream, d_n, n_all, d_x, count, d_o0, d_o1, d_d0, d_d1);  \
  return (int)hipGetLastError();
int dm_cke_pair_jet(const int* d_n, int n_all, const double* d_x, int count, double* d_o0, double* d_o1, double* d_d0, double* d_d1,
                    hipStream_t stream) {
  DM_LAUNCH4(cke_pair_jet_kernel)
}
int dm_cie_pair_from_k_jet(const int* d_n, int n_all, const double* d_x, int count, double* d_o0, double* d_o1, double* d_d0,
                           double* d_d1, hipStream_t stream) {
  DM_LAUNCH4(cie_pair_from_k_jet_kernel)
}
// op: 0 cz_sqrt(b), 1 cz_log(b), 2 cz_exp(b) (d_a unused), 3 a / b (d_a complex), 4 a / b (d_a real)
int dm_cz_primitive(int op, const double* d_a, const double* d_b, int count, double* d_o, hipStream_t stream) {
  if (count <= 0) return 0;
  if (op < 0 || op > 4) return (int)hipErrorInvalidValue;
  if (op >= 3 && !d_a) return (int)hipErrorInvalidValue;
  switch (op) {
    case 0: hipLaunchKernelGGL((cz_primitive_kernel<0>), blocks(count), dim3(kThreads), 0, stream, d_a, d_b, count, d_o); break;
    case 1: hipLaunchKernelGGL((cz_primitive_kernel<1>), blocks(count), dim3(kThreads), 0, stream, d_a, d_b, count, d_o); break;
    case 2: hipLaunchKernelGGL((cz_primitive_kernel<2>), blocks(count), dim3(kThreads), 0, stream, d_a, d_b, count, d_o); break;
    case 3: hipLaunchKernelGGL((cz_primitive_kernel<3>), blocks(count), dim3(kThreads), 0, stream, d_a, d_b, count, d_o); break;
    default: hipLaunchKernelGGL((cz_primitive_kernel<4>), blocks(count), dim3(kThreads), 0, stream, d_a, d_b, count, d_o); break;
  }
  return (int)hipGetLastError();
}
}
