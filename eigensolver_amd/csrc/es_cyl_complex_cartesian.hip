// K20: Cartesian sampling of an unstable cylinder mode, with its vorticity (include/eigensolver_amd.h section 20): section 8
// at complex frequency, on the complex amplitude tables of es_cyl_complex_polarisation.  No problem handle: one text for
// the untwisted and the rotating cylinder.  The CPU restatement is tests/cyl_complex_cartesian_model.py.
//   es_cyl_complex_vorticity_amplitudes   complex v_r, v_phi, v_z amplitudes -> the three complex radial amplitudes of
//                                         curl v; one lane per (mode, radial point); derivatives by gradient_stencil per
//                                         region, of the real and the imaginary part separately
//   es_cyl_complex_cartesian_synthesis    complex amplitudes of one mode -> float32 frames [t][variable][z][y][x] of
//                                         Re[c e^{i (k z - w t)}] = c_re EC - c_im ES, the growth factor included; the
//                                         (x, y) stage once per point, then bound by store bandwidth.  Launch shape, region
//                                         and tie rules, item walk and host checks are section 8's own text
//                                         (es_cartesian_shared.hpp); the (z, t) table is zt_tables<true> of
//                                         es_field_shared.hpp.
#include "es_cartesian_shared.hpp"

namespace {

// ---- complex v amplitudes -> complex amplitudes of curl v -----------------------------------------------------------
// With d/dz -> i k:  W_r = -m a_z / r + i k a_phi,  W_phi = -a_z' + i k a_r,  W_z = (m a_r - a_phi - r a_phi') / r.
// Each part keeps section 8's grouping (Wr_C, Wr_S, ... of vorticity_amplitudes_kernel), so that on a table with zero
// imaginary parts Re W = (Wr_C, Wphi_C, Wz_C) and Im W = (-Wr_S, -Wphi_S, 0) in value.
__global__ __launch_bounds__(256) void cylcart_vorticity_amplitudes_kernel(const double* __restrict__ radius,
                                                                          const double* __restrict__ amp,
                                                                          const double* __restrict__ kk, int n, int N,
                                                                          int n_ext, double dm, double* __restrict__ vort) {
  const size_t n_r = (size_t)N + (size_t)n_ext;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * n_r) return;
  const size_t i = t / n_r;
  const int j = (int)(t - i * n_r);
  const int base = (j < N) ? 0 : N;
  const int len = (j < N) ? N : n_ext;                 // >= 3 (checked by the host)
  const int q = j - base;
  const double* r = radius + i * n_r + base;
  const double* A = amp + 2 * (i * (size_t)ES_AMP_COUNT * n_r + base);   // (re, im) pairs
  const Stencil3 g = gradient_stencil(r, q, len);
  const int p = g.p;
  const double* ar = A + 2 * (size_t)ES_AMP_V_R * n_r;
  const double* ap = A + 2 * (size_t)ES_AMP_V_PHI * n_r;
  const double* az = A + 2 * (size_t)ES_AMP_V_Z * n_r;
  const double rq = r[q], k = kk[i];
  double a_r[2], a_p[2], a_z[2], d_az[2], d_ap[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    d_az[h] = (g.c0 * az[2 * p + h] + g.c1 * az[2 * (p + 1) + h]) + g.c2 * az[2 * (p + 2) + h];
    d_ap[h] = (g.c0 * ap[2 * p + h] + g.c1 * ap[2 * (p + 1) + h]) + g.c2 * ap[2 * (p + 2) + h];
    a_r[h] = ar[2 * q + h]; a_p[h] = ap[2 * q + h]; a_z[h] = az[2 * q + h];
  }
  double* V = vort + 2 * (i * (size_t)ES_CVORT_COUNT * n_r + j);
  V[2 * ES_CVORT_R * n_r] = -(dm * a_z[0]) / rq + -(k * a_p[1]);
  V[2 * ES_CVORT_R * n_r + 1] = -(dm * a_z[1]) / rq + k * a_p[0];
  V[2 * ES_CVORT_PHI * n_r] = -d_az[0] + -(k * a_r[1]);
  V[2 * ES_CVORT_PHI * n_r + 1] = -d_az[1] + k * a_r[0];
#pragma unroll
  for (int h = 0; h < 2; ++h) V[2 * ES_CVORT_Z * n_r + h] = ((dm * a_r[h] - a_p[h]) - rq * d_ap[h]) / rq;
}

// ---- complex amplitudes -> frames on the (x, y, z, t) mesh ----------------------------------------------------------
// The shape of cartesian_synthesis_kernel, from the same text (es_cartesian_shared.hpp, which says why).  What differs is
// what a lane keeps: per selected variable and point a COMPLEX coefficient c, formed part by part exactly as section 8
// forms its real one, and the value is c_re EC - c_im ES, with EC and ES by scalar loads from the __restrict__ table.  All
// 2 x 10 coefficient sets of the four points stay in registers (160 VGPRs); the second launch bound holds the kernel to the
// 256 registers of two waves per SIMD (DESIGN 8o has the count and what the alternatives cost).
template <bool SWAP, bool WIDE>
__global__ __launch_bounds__(64, 2) void cylcart_synthesis_kernel(CartArgs a, const double* __restrict__ tab,
                                                                 uint32_t* __restrict__ out) {
  const size_t n_zt = (size_t)a.n_z * a.n_t;
  CartLane s;
  if (!cart_stage<WIDE>(a, s)) return;
  double c[2][ES_CVAR_COUNT][4];                       // [re, im][variable][point]
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < ES_CVAR_COUNT; ++v) c[h][v][e] = 0.0;
    if (!((s.valid >> e) & 1u)) continue;
    const CartPoint p = cart_point(a, s, e);
    const double vs = a.v_scale, ct = p.ct, st = p.st, cm = p.cm, sm = p.sm;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      cart_amp_coefficients<2>(a, p, h, e, c[h]);
      if (a.mask & (bit(ES_CVAR_VORT_X) | bit(ES_CVAR_VORT_Y))) {
        const double wr = (p.L<2>(a.vort, ES_CVORT_R, h) * vs) * sm, wp = (p.L<2>(a.vort, ES_CVORT_PHI, h) * vs) * cm;
        c[h][ES_CVAR_VORT_X][e] = wr * ct - wp * st;
        c[h][ES_CVAR_VORT_Y][e] = wr * st + wp * ct;
      }
      if (a.mask & bit(ES_CVAR_VORT_Z)) c[h][ES_CVAR_VORT_Z][e] = (p.L<2>(a.vort, ES_CVORT_Z, h) * vs) * sm;
    }
  }
  cart_walk<WIDE>(a, out, s, [&](int v, size_t zt, uint32_t (&b)[4]) {
    const double EC = tab[zt], ES = tab[n_zt + zt];
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = f32_bits(c[0][v][e] * EC - c[1][v][e] * ES, SWAP);
  });
}

}  // namespace

extern "C" int es_cyl_complex_vorticity_amplitudes(es_context* ctx, const double* d_radius, const double* d_amp, int n,
                                                   int n_nodes, int n_ext, int m, const double* d_k, double* d_vort) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  unsigned blocks;
  const int rc = vorticity_args(ctx, d_radius, d_amp, n, n_nodes, n_ext, m, d_k, d_vort, blocks);
  if (rc || !blocks) return rc;
  hipLaunchKernelGGL(cylcart_vorticity_amplitudes_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_radius, d_amp, d_k, n,
                     n_nodes, n_ext, (double)m, d_vort);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

// The launch split is section 8's (es_cyl_cartesian_split): the points per lane are the same.
extern "C" int es_cyl_complex_cartesian_synthesis(es_context* ctx, const double* d_radius, const double* d_amp,
                                                  const double* d_vort, int n_nodes, int n_ext, int m, double k,
                                                  double w_re, double w_im, const double* d_x, int n_x, const double* d_y,
                                                  int n_y, const double* d_z, int n_z, const double* d_t, int n_t,
                                                  uint32_t var_mask, double v_scale, float fill, int flags,
                                                  float* d_out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  CartLaunch L;
  bool none;
  const int rc = cartesian_args<true>(ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w_re, w_im, d_x, n_x, d_y, n_y, d_z,
                                      n_z, d_t, n_t, var_mask, v_scale, fill, flags, d_out, L, none);
  if (rc || none) return rc;
  hipLaunchKernelGGL(ES_SWAP_WIDE_KERNEL(cylcart_synthesis_kernel, L.swap, L.wide), L.grid, dim3(64), 0, ctx->stream, L.a,
                     L.tab, L.out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
