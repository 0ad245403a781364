// Test-only device build of the math headers (eigensolver_amd/csrc/es_bessel.hpp, es_bessel_complex.hpp, es_cjet.hpp, and the
// real jets es_jet.hpp, es_jet2.hpp operator by operator): one (order, argument) resp. one operand row per thread, so that
// the paths the headers take only inside __HIP_DEVICE_COMPILE__ -- qdiv on v_rcp_f64,
// the __constant__ reciprocal and Chebyshev tables, the device log / exp / sqrt / hypot / atan2 / sin / cos -- can be measured
// against correctly rounded values (tests/test_devmath_gpu.py, tests/golden/bessel_truth.npz, bessel_complex_truth.npz,
// jet_truth.npz).
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
#include "../../eigensolver_amd/csrc/es_jet2.hpp"

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

// ---- the real jets: es_jet.hpp, es_jet2.hpp ----------------------------------------------------------------------------------------
// The Bessel lifts with x the variable, in Jet<1> and in Jet2<1>.  Ten doubles per row: Jet<1> (A.v, A.d, B.v, B.d), then
// Jet2<1> (A.v, A.d, A.h, B.v, B.d, B.h); (A, B) = (e^x K_n, e^x K_{n+1}) resp. e^-x (I_n, I_{n+1}) fed by ke_pair at the
// same argument.
template <bool UNIFORM, bool IE>
__global__ __launch_bounds__(kThreads) void bessel_jets_kernel(const int* __restrict__ nv, int n_all, const double* __restrict__ x,
                                                               int count, double* __restrict__ o) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const int n = UNIFORM ? n_all : nv[i];
  const Jet<1> X1 = jet_variable<1>(x[i], 0);
  const Jet2<1> X2 = JetVariable<Jet2<1>>::make(x[i], 0);
  Jet<1> A1, B1;
  Jet2<1> A2, B2;
  ke_pair(n, X1, A1, B1);
  ke_pair(n, X2, A2, B2);
  if (IE) {
    Jet<1> I1, J1;
    Jet2<1> I2, J2;
    ie_pair_from_k(n, X1, A1, B1, I1, J1);
    ie_pair_from_k(n, X2, A2, B2, I2, J2);
    A1 = I1; B1 = J1; A2 = I2; B2 = J2;
  }
  double* r = o + 10 * (size_t)i;
  r[0] = A1.v; r[1] = A1.d[0]; r[2] = B1.v; r[3] = B1.d[0];
  r[4] = A2.j.v; r[5] = A2.j.d[0]; r[6] = A2.h[0]; r[7] = B2.j.v; r[8] = B2.j.d[0]; r[9] = B2.h[0];
}

// A row of six doubles (v, d[0], d[1], h[0], h[1], h[2]) as a Jet2<2>; as a Jet2<1> it is (v, d[0], h[0]), the components in
// the first variable alone.  A Jet<NV> result goes to a row of three doubles (v, d[0], d[1]).
template <int NV> __device__ __forceinline__ Jet2<NV> jet2_at(const double* __restrict__ p, int i) {
  const double* r = p + 6 * (size_t)i;
  Jet2<NV> x;
  x.j.v = r[0];
  x.j.d[0] = r[1];
  x.h[0] = r[3];
  if constexpr (NV == 2) { x.j.d[1] = r[2]; x.h[1] = r[4]; x.h[2] = r[5]; }
  return x;
}
template <int NV> __device__ __forceinline__ void jet_put(double* __restrict__ p, int i, const Jet<NV>& x) {
  double* r = p + 3 * (size_t)i;
  r[0] = x.v;
  r[1] = x.d[0];
  if constexpr (NV == 2) r[2] = x.d[1];
}
template <int NV> __device__ __forceinline__ void jet2_put(double* __restrict__ p, int i, const Jet2<NV>& x) {
  double* r = p + 6 * (size_t)i;
  r[0] = x.j.v;
  r[1] = x.j.d[0];
  r[3] = x.h[0];
  if constexpr (NV == 2) { r[2] = x.j.d[1]; r[4] = x.h[1]; r[5] = x.h[2]; }
}

// One operator or overload of the two headers per OP (the list at dm_jet_op), on Jet2<NV> operands x, y, z, doubles a, b, c
// and an int e: r2 the Jet2<NV> result, r1 the same operator on the operands' Jet<NV> parts, r0 the plain double operation
// on the values.
constexpr int kJetOps = 33;
template <int OP, int NV>
__global__ __launch_bounds__(kThreads) void jet_op_kernel(const double* __restrict__ px, const double* __restrict__ py,
                                                          const double* __restrict__ pz, const double* __restrict__ pa,
                                                          const double* __restrict__ pb, const double* __restrict__ pc,
                                                          const int* __restrict__ pe, int count, double* __restrict__ o2,
                                                          double* __restrict__ o1, double* __restrict__ o0) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const Jet2<NV> x = jet2_at<NV>(px, i), y = jet2_at<NV>(py, i), z = jet2_at<NV>(pz, i);
  const double a = pa[i], b = pb[i], c = pc[i];
  const int e = pe[i];
  Jet2<NV> r2;
  Jet<NV> r1;
  double r0;
  if constexpr (OP == 0) { r2 = -x; r1 = -x.j; r0 = -x.j.v; }
  else if constexpr (OP == 1) { r2 = x + y; r1 = x.j + y.j; r0 = x.j.v + y.j.v; }
  else if constexpr (OP == 2) { r2 = x - y; r1 = x.j - y.j; r0 = x.j.v - y.j.v; }
  else if constexpr (OP == 3) { r2 = x + a; r1 = x.j + a; r0 = x.j.v + a; }
  else if constexpr (OP == 4) { r2 = a + x; r1 = a + x.j; r0 = a + x.j.v; }
  else if constexpr (OP == 5) { r2 = x - a; r1 = x.j - a; r0 = x.j.v - a; }
  else if constexpr (OP == 6) { r2 = a - x; r1 = a - x.j; r0 = a - x.j.v; }
  else if constexpr (OP == 7) { r2 = x * a; r1 = x.j * a; r0 = x.j.v * a; }
  else if constexpr (OP == 8) { r2 = a * x; r1 = a * x.j; r0 = a * x.j.v; }
  else if constexpr (OP == 9) { r2 = x; r2 *= a; r1 = x.j; r1 *= a; r0 = x.j.v; r0 *= a; }
  else if constexpr (OP == 10) { r2 = x * y; r1 = x.j * y.j; r0 = x.j.v * y.j.v; }
  else if constexpr (OP == 11) { r2 = fma(x, y, z); r1 = fma(x.j, y.j, z.j); r0 = fma(x.j.v, y.j.v, z.j.v); }
  else if constexpr (OP == 12) { r2 = fma(a, x, y); r1 = fma(a, x.j, y.j); r0 = fma(a, x.j.v, y.j.v); }
  else if constexpr (OP == 13) { r2 = fma(x, y, a); r1 = fma(x.j, y.j, a); r0 = fma(x.j.v, y.j.v, a); }
  else if constexpr (OP == 14) { r2 = fma(a, x, b); r1 = fma(a, x.j, b); r0 = fma(a, x.j.v, b); }
  else if constexpr (OP == 15) { r2 = fma(x, a, y); r1 = fma(x.j, a, y.j); r0 = fma(x.j.v, a, y.j.v); }
  else if constexpr (OP == 16) { r2 = fma(x, a, b); r1 = fma(x.j, a, b); r0 = fma(x.j.v, a, b); }
  else if constexpr (OP == 17) { r2 = rcp_from(x, a); r1 = rcp_from(x.j, a); r0 = a; }
  else if constexpr (OP == 18) { r2 = rcp(x); r1 = rcp(x.j); r0 = 1.0 / x.j.v; }
  else if constexpr (OP == 19) { r2 = fast_rcp(x); r1 = fast_rcp(x.j); r0 = fast_rcp(x.j.v); }
  else if constexpr (OP == 20) { r2 = x / y; r1 = x.j / y.j; r0 = x.j.v / y.j.v; }
  else if constexpr (OP == 21) { r2 = a / x; r1 = a / x.j; r0 = a / x.j.v; }
  else if constexpr (OP == 22) { r2 = x / a; r1 = x.j / a; r0 = x.j.v / a; }
  else if constexpr (OP == 23) { r2 = sqrt(x); r1 = sqrt(x.j); r0 = sqrt(x.j.v); }
  else if constexpr (OP == 24) { r2 = exp(x); r1 = exp(x.j); r0 = exp(x.j.v); }
  else if constexpr (OP == 25) { r2 = ldexp(x, e); r1 = ldexp(x.j, e); r0 = ldexp(x.j.v, e); }
  else if constexpr (OP == 26) { r2 = lift_onto(y.j, a, b, x); r1 = y.j; r0 = y.j.v; }
  else if constexpr (OP == 27) { r2 = lift(a, b, c, x); r1 = lift(a, b, x.j); r0 = a; }
  else if constexpr (OP == 28) { r2 = fabs(x); r1 = fabs(x.j); r0 = fabs(x.j.v); }
  else if constexpr (OP == 29) {                               // jet_finite: 1.0 or 0.0 in the value, zeros elsewhere
    r2 = Jet2<NV>(jet_finite(x) ? 1.0 : 0.0); r1 = Jet<NV>(jet_finite(x.j) ? 1.0 : 0.0); r0 = isfinite(x.j.v) ? 1.0 : 0.0;
  }
  else if constexpr (OP == 30) { r2 = Jet2<NV>(val(x)); r1 = Jet<NV>(val(x.j)); r0 = x.j.v; }      // val and the constant
  else if constexpr (OP == 31) { r2 = Jet2<NV>(a); r1 = Jet<NV>(a); r0 = a; }
  else { r2 = JetVariable<Jet2<NV>>::make(a, e); r1 = JetVariable<Jet<NV>>::make(a, e); r0 = a; }  // variable number e
  jet2_put<NV>(o2, i, r2);
  jet_put<NV>(o1, i, r1);
  o0[i] = r0;
}

template <int OP>
void jet_op_launch(int nv, const double* x, const double* y, const double* z, const double* a, const double* b, const double* c,
                   const int* e, int count, double* o2, double* o1, double* o0, hipStream_t stream) {
  if (nv == 1) hipLaunchKernelGGL((jet_op_kernel<OP, 1>), blocks(count), dim3(kThreads), 0, stream, x, y, z, a, b, c, e, count, o2, o1, o0);
  else hipLaunchKernelGGL((jet_op_kernel<OP, 2>), blocks(count), dim3(kThreads), 0, stream, x, y, z, a, b, c, e, count, o2, o1, o0);
}
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

// ---- the real jets ------------------------------------------------------------------------------------------------------------------
// d_o: 10 count doubles, per row Jet<1> (A.v, A.d, B.v, B.d) and Jet2<1> (A.v, A.d, A.h, B.v, B.d, B.h) with x the variable
int dm_ke_pair_jets(const int* d_n, int n_all, const double* d_x, int count, double* d_o, hipStream_t stream) {
  if (count <= 0) return 0;
  if (d_n) hipLaunchKernelGGL((bessel_jets_kernel<false, false>), blocks(count), dim3(kThreads), 0, stream, d_n, 0, d_x, count, d_o);
  else hipLaunchKernelGGL((bessel_jets_kernel<true, false>), blocks(count), dim3(kThreads), 0, stream, d_n, n_all, d_x, count, d_o);
  return (int)hipGetLastError();
}
int dm_ie_pair_from_k_jets(const int* d_n, int n_all, const double* d_x, int count, double* d_o, hipStream_t stream) {
  if (count <= 0) return 0;
  if (d_n) hipLaunchKernelGGL((bessel_jets_kernel<false, true>), blocks(count), dim3(kThreads), 0, stream, d_n, 0, d_x, count, d_o);
  else hipLaunchKernelGGL((bessel_jets_kernel<true, true>), blocks(count), dim3(kThreads), 0, stream, d_n, n_all, d_x, count, d_o);
  return (int)hipGetLastError();
}
// One operator or overload per row, in Jet2<nv>, Jet<nv> and double (nv: 1 or 2).  d_x, d_y, d_z: 6 count doubles, a row
// (v, d[0], d[1], h[0], h[1], h[2]); nv = 1 reads (v, d[0], h[0]) of it.  d_a, d_b, d_c: count doubles; d_e: count ints.
// d_o2: 6 count doubles, the Jet2 result in the layout of the operands; d_o1: 3 count doubles, the Jet result (v, d[0], d[1]);
// d_o0: count doubles.  nv = 1 leaves the components of the second variable untouched.  Every pointer must be given.
// op:  0 -x          1 x + y        2 x - y        3 x + a         4 a + x         5 x - a          6 a - x
//      7 x * a       8 a * x        9 x *= a      10 x * y        11 fma(x, y, z) 12 fma(a, x, y)  13 fma(x, y, a)
//     14 fma(a, x, b)              15 fma(x, a, y)                16 fma(x, a, b) 17 rcp_from(x, a)                18 rcp(x)
//     19 fast_rcp(x)               20 x / y       21 a / x        22 x / a        23 sqrt(x)       24 exp(x)
//     25 ldexp(x, e)               26 lift_onto(y.j, a, b, x) (Jet: y.j itself)   27 lift(a, b, c, x) (Jet: lift(a, b, x.j))
//     28 fabs(x)    29 jet_finite(x) as the constant 1.0 / 0.0    30 the constant val(x)           31 the constant a
//     32 the variable number e at the value a (JetVariable, jet_variable)
#define DM_JET_OP(OP) case OP: jet_op_launch<OP>(nv, d_x, d_y, d_z, d_a, d_b, d_c, d_e, count, d_o2, d_o1, d_o0, stream); break;
int dm_jet_op(int op, int nv, const double* d_x, const double* d_y, const double* d_z, const double* d_a, const double* d_b,
              const double* d_c, const int* d_e, int count, double* d_o2, double* d_o1, double* d_o0, hipStream_t stream) {
  if (count <= 0) return 0;
  if (op < 0 || op >= kJetOps || (nv != 1 && nv != 2)) return (int)hipErrorInvalidValue;
  if (!d_x || !d_y || !d_z || !d_a || !d_b || !d_c || !d_e || !d_o2 || !d_o1 || !d_o0) return (int)hipErrorInvalidValue;
  switch (op) {
    DM_JET_OP(0) DM_JET_OP(1) DM_JET_OP(2) DM_JET_OP(3) DM_JET_OP(4) DM_JET_OP(5) DM_JET_OP(6) DM_JET_OP(7) DM_JET_OP(8)
    DM_JET_OP(9) DM_JET_OP(10) DM_JET_OP(11) DM_JET_OP(12) DM_JET_OP(13) DM_JET_OP(14) DM_JET_OP(15) DM_JET_OP(16)
    DM_JET_OP(17) DM_JET_OP(18) DM_JET_OP(19) DM_JET_OP(20) DM_JET_OP(21) DM_JET_OP(22) DM_JET_OP(23) DM_JET_OP(24)
    DM_JET_OP(25) DM_JET_OP(26) DM_JET_OP(27) DM_JET_OP(28) DM_JET_OP(29) DM_JET_OP(30) DM_JET_OP(31) DM_JET_OP(32)
  }
  return (int)hipGetLastError();
}
}
