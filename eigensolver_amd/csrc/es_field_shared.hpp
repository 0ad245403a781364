// What the field-synthesis translation units (es_fields.hip, es_cartesian.hip, es_slab_fields.hip) have in common: the
// three-point gradient stencil, the one rounding to fp32, the bracket search over a piecewise table with the
// interpolation that follows it, the store tail of a lane's four points, the <SWAP, WIDE> dispatch and the (z, t) phase
// table.  Everything on the device is force-inlined, so a kernel compiles as if the text stood in its own file.
#pragma once
#include "es_common.hpp"

namespace {

// ---- three-point gradient -------------------------------------------------------------------------------------------
// np.gradient(a, x, edge_order=2) at node q of a region of len >= 3 nodes with abscissae x, coefficient form and order of
// operations included: nodes p, p+1, p+2 with spacings d1, d2; the node differentiated is the middle one, or the first /
// last at a region end.  The caller applies (c0 a[p] + c1 a[p+1]) + c2 a[p+2].
struct Stencil3 { int p; double c0, c1, c2; };

__device__ __forceinline__ Stencil3 gradient_stencil(const double* x, int q, int len) {
  Stencil3 s;
  s.p = q - 1;
  if (s.p < 0) s.p = 0;
  if (s.p > len - 3) s.p = len - 3;
  const double d1 = x[s.p + 1] - x[s.p], d2 = x[s.p + 2] - x[s.p + 1];
  if (q == 0) {
    s.c0 = -(2.0 * d1 + d2) / (d1 * (d1 + d2));
    s.c1 = (d1 + d2) / (d1 * d2);
    s.c2 = -d1 / (d2 * (d1 + d2));
  } else if (q == len - 1) {
    s.c0 = d2 / (d1 * (d1 + d2));
    s.c1 = -(d2 + d1) / (d1 * d2);
    s.c2 = (2.0 * d2 + d1) / (d2 * (d1 + d2));
  } else {
    s.c0 = -d2 / (d1 * (d1 + d2));
    s.c1 = (d2 - d1) / (d1 * d2);
    s.c2 = d1 / (d2 * (d1 + d2));
  }
  return s;
}

// ---- fp32 as it is stored -------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t stored_bits(uint32_t u, bool swap) { return swap ? __builtin_bswap32(u) : u; }

__device__ __forceinline__ uint32_t f32_bits(double v, bool swap) {
  return stored_bits(__float_as_uint((float)v), swap);   // the one rounding to fp32
}

// the fill value as it is stored: as bits, so that a NaN keeps its payload
inline uint32_t fill_bits_of(float fill, bool swap) {
  uint32_t u;
  memcpy(&u, &fill, sizeof(fill));
  return stored_bits(u, swap);
}

// ---- bracket search and interpolation -------------------------------------------------------------------------------
// bisection steps that bring a region of `longest` nodes down to one interval
inline int bisection_iters(int longest) {
  int iters = 0;
  while ((1ll << iters) < (long long)longest - 1) ++iters;
  return iters;
}

// For each of a lane's four abscissae x[e], searched side by side: the largest j in [lo[e], hi[e]] with tab[j] <= x[e], at
// most the last but one, left in lo[e].
__device__ __forceinline__ void bracket4(const double* __restrict__ tab, const double (&x)[4], int (&lo)[4], int (&hi)[4],
                                         int iters) {
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (hi[e] - lo[e] > 1) {
        const int mid = (lo[e] + hi[e]) >> 1;
        if (tab[mid] <= x[e]) lo[e] = mid; else hi[e] = mid;
      }
    }
  }
}

// Linear interpolation inside the bracket [x0, x1]; at_end holds only on the last node of a region and selects that
// node's value as tabulated.
struct Lerp {
  double tt; bool at_end;
  __device__ __forceinline__ Lerp(double x, double x0, double x1) : tt((x - x0) / (x1 - x0)), at_end(x >= x1) {}
  __device__ __forceinline__ double operator()(double A0, double A1) const {
    const double v = A0 + (A1 - A0) * tt;
    return at_end ? A1 : v;
  }
};

// ---- store tail -----------------------------------------------------------------------------------------------------
// points outside the table (bit e of `valid` clear) carry the fill
__device__ __forceinline__ void fill_invalid(uint32_t (&b)[4], unsigned valid, uint32_t fill_bits) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (!((valid >> e) & 1u)) b[e] = fill_bits;
}

// The four values of a lane into the row dst.  WIDE: idx[0..3] are consecutive, idx[0] a multiple of 4 and the row
// 16-byte aligned with a length that is a multiple of 4, so a lane has all four points or none: one 16-byte store.
// Otherwise four 4-byte stores, those of the points inside the mesh (bits of `live`).
template <bool WIDE>
__device__ __forceinline__ void store4(uint32_t* dst, const size_t (&idx)[4], const uint32_t (&b)[4], unsigned live) {
  if (WIDE) {
    *reinterpret_cast<uint4*>(dst + idx[0]) = make_uint4(b[0], b[1], b[2], b[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if ((live >> e) & 1u) dst[idx[e]] = b[e];
  }
}

// the <SWAP, WIDE> instantiation of a kernel template for two host flags
#define ES_SWAP_WIDE_KERNEL(kernel, swap, wide)                                \
  ((swap) ? ((wide) ? kernel<true, true> : kernel<true, false>)                \
          : ((wide) ? kernel<false, true> : kernel<false, false>))

// ---- (z, t) phase table ---------------------------------------------------------------------------------------------
// [e^{w_im t_tau}] cos(k z_l - w_re t_tau) at [tau * n_z + l], the same with sin behind it at [n_z n_t + tau * n_z + l];
// the growth factor only with GROWTH (a real mode multiplies by nothing)
template <bool GROWTH>
__global__ __launch_bounds__(256) void zt_tables_kernel(const double* __restrict__ z, int n_z,
                                                       const double* __restrict__ tt, int n_t, double k, double w_re,
                                                       double w_im, double* __restrict__ tab) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n_zt = (size_t)n_z * n_t;
  if (i >= n_zt) return;
  const size_t tau = i / n_z, l = i - tau * n_z;
  const double ph = k * z[l] - w_re * tt[tau];
  if (GROWTH) {
    const double E = exp(w_im * tt[tau]);
    tab[i] = E * cos(ph);
    tab[n_zt + i] = E * sin(ph);
  } else {
    tab[i] = cos(ph);
    tab[n_zt + i] = sin(ph);
  }
}

// the table of one call in the context's scratch, enqueued on its stream
template <bool GROWTH>
inline int zt_tables(es_context* ctx, const double* d_z, int n_z, const double* d_t, int n_t, double k, double w_re,
                     double w_im, double** tab) {
  const size_t n_zt = (size_t)n_z * n_t;
  const int rc = es_ensure_scratch(ctx, 2 * n_zt * sizeof(double));
  if (rc) return rc;
  *tab = static_cast<double*>(ctx->d_scratch);
  hipLaunchKernelGGL(zt_tables_kernel<GROWTH>, dim3((unsigned)((n_zt + 255) / 256)), dim3(256), 0, ctx->stream, d_z, n_z,
                     d_t, n_t, k, w_re, w_im, *tab);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace
