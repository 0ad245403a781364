// K20: Cartesian sampling of an unstable cylinder mode, with its vorticity (include/eigensolver_amd.h section 20): section 8
// at complex frequency, on the complex amplitude tables of es_cyl_complex_polarisation.  No problem handle: one text for
// the untwisted and the rotating cylinder.  The CPU restatement is tests/cyl_complex_cartesian_model.py.
//   es_cyl_complex_vorticity_amplitudes   complex v_r, v_phi, v_z amplitudes -> the three complex radial amplitudes of
//                                         curl v; one lane per (mode, radial point); derivatives by gradient_stencil per
//                                         region, of the real and the imaginary part separately
//   es_cyl_complex_cartesian_synthesis    complex amplitudes of one mode -> float32 frames [t][variable][z][y][x] of
//                                         Re[c e^{i (k z - w t)}] = c_re EC - c_im ES, the growth factor included; the
//                                         (x, y) stage once per point, then bound by store bandwidth.  Launch shape, region
//                                         and tie rules, stores: those of cartesian_synthesis_kernel (es_cartesian.hip);
//                                         the (z, t) table is zt_tables<true> of es_field_shared.hpp.
#include "es_field_shared.hpp"

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
struct CCartArgs {
  const double* radius; const double* amp; const double* vort;   // [n_r], [7 x n_r x 2], [3 x n_r x 2] (NULL without vorticity)
  const double* x; const double* y;
  int N, n_ext, m, n_x, n_z, n_t, n_sel;
  size_t n_pts;                                        // n_x n_y: the points of one z plane, contiguous in d_out
  int iters;                                           // bisection steps that bring any region down to one interval
  int z_parts, z_chunk;                                // a frame's z planes are cut into z_parts pieces of z_chunk planes
  int items_per_block;                                 // (frame, piece) items a workgroup walks
  uint32_t mask, fill_bits;                            // fill as it is stored (already byte-swapped if requested)
  double v_scale;
};

constexpr uint32_t bit(int v) { return 1u << v; }

// The shape of cartesian_synthesis_kernel (es_cartesian.hip), which says why: one wave per workgroup, a z plane walked as one
// array of n_x n_y points in pieces of 256, four points per lane (WIDE: consecutive, one 16-byte store; else lane + 64 e,
// four 4-byte stores), the (x, y) stage once, then (frame, z piece) items with variable outer and z planes inner, EC and ES
// by scalar loads.  What differs is what a lane keeps: per selected variable and point a COMPLEX coefficient c, formed
// part by part exactly as section 8 forms its real one, and the value is c_re EC - c_im ES.  All 2 x 10 coefficient sets of
// the four points stay in registers (160 VGPRs); the second launch bound holds the kernel to the 256 registers of two waves
// per SIMD (DESIGN 8o has the count and what the alternatives cost).
template <bool SWAP, bool WIDE>
__global__ __launch_bounds__(64, 2) void cylcart_synthesis_kernel(CCartArgs a, const double* __restrict__ tab,
                                                                 uint32_t* __restrict__ out) {
  const size_t p0 = (size_t)blockIdx.x * 256;
  const int N = a.N, n_r = a.N + a.n_ext;
  const double* __restrict__ rad = a.radius;
  const double r_first = rad[0], r_last = rad[n_r - 1];
  const double r_b = (N > 0) ? rad[N - 1] : 0.0;       // boundary radius: r == r_b takes the interior values
  const uint32_t mask = a.mask;
  const double vs = a.v_scale;
  const size_t n_zt = (size_t)a.n_z * a.n_t;
  const int n_items = a.n_t * a.z_parts;

  size_t pt[4];
  double xv[4], yv[4], rr[4];
  int lo[4], hi[4];
  unsigned live = 0, valid = 0;
  // region: interior [r_first, r_b], exterior (r_b, r_last]; r = 0, the hole, the far field and NaN are outside
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    pt[e] = p0 + (WIDE ? (size_t)threadIdx.x * 4 + e : (size_t)threadIdx.x + 64 * e);
    const bool in_mesh = pt[e] < a.n_pts;
    const size_t iy = in_mesh ? pt[e] / (size_t)a.n_x : 0;
    const size_t ix = in_mesh ? pt[e] - iy * (size_t)a.n_x : 0;
    xv[e] = a.x[ix];
    yv[e] = a.y[iy];
    const double r = hypot(xv[e], yv[e]);
    const bool in = N > 0 && r >= r_first && r <= r_b;
    const bool ex = a.n_ext > 0 && r <= r_last && (N > 0 ? r > r_b : r >= r_first);
    const bool ok = in_mesh && (in || ex) && r > 0.0;
    const int base = in ? 0 : N;
    rr[e] = r;
    lo[e] = base;
    hi[e] = ok ? base + (in ? N : a.n_ext) - 1 : base;
    live |= (in_mesh ? 1u : 0u) << e;
    valid |= (ok ? 1u : 0u) << e;
  }
  if (!live) return;
  bracket4(rad, rr, lo, hi, a.iters);                  // largest j of the region with rad[j] <= r, at most the last but one
  double c[2][ES_CVAR_COUNT][4];                       // [re, im][variable][point]
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < ES_CVAR_COUNT; ++v) c[h][v][e] = 0.0;
    if (!((valid >> e) & 1u)) continue;
    const int j = lo[e];
    const double r = rr[e];
    const Lerp lerp(r, rad[j], rad[j + 1]);
    auto L = [&](const double* __restrict__ tabv, int ch, int h) {     // part h of channel ch, interpolated
      return lerp(tabv[2 * ((size_t)ch * n_r + j) + h], tabv[2 * ((size_t)ch * n_r + j + 1) + h]);
    };
    const double ct = xv[e] / r, st = yv[e] / r;
    double cm = 1.0, sm = 0.0;                         // cos(m theta), sin(m theta) by angle addition
    for (int s = 0; s < a.m; ++s) {
      const double c2 = cm * ct - sm * st, s2 = sm * ct + cm * st;
      cm = c2; sm = s2;
    }
    const double fs = -sm;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (mask & bit(ES_CVAR_P_T)) c[h][ES_CVAR_P_T][e] = L(a.amp, ES_AMP_P_T, h) * cm;
      if (mask & (bit(ES_CVAR_XI_X) | bit(ES_CVAR_XI_Y))) {
        const double pr = L(a.amp, ES_AMP_XI_R, h) * cm, pp = L(a.amp, ES_AMP_XI_PHI, h) * fs;
        c[h][ES_CVAR_XI_X][e] = pr * ct - pp * st;
        c[h][ES_CVAR_XI_Y][e] = pr * st + pp * ct;
      }
      if (mask & bit(ES_CVAR_XI_Z)) c[h][ES_CVAR_XI_Z][e] = L(a.amp, ES_AMP_XI_Z, h) * cm;
      if (mask & (bit(ES_CVAR_V_X) | bit(ES_CVAR_V_Y))) {
        const double pr = (L(a.amp, ES_AMP_V_R, h) * vs) * cm, pp = (L(a.amp, ES_AMP_V_PHI, h) * vs) * fs;
        c[h][ES_CVAR_V_X][e] = pr * ct - pp * st;
        c[h][ES_CVAR_V_Y][e] = pr * st + pp * ct;
      }
      if (mask & bit(ES_CVAR_V_Z)) c[h][ES_CVAR_V_Z][e] = (L(a.amp, ES_AMP_V_Z, h) * vs) * cm;
      if (mask & (bit(ES_CVAR_VORT_X) | bit(ES_CVAR_VORT_Y))) {
        const double wr = (L(a.vort, ES_CVORT_R, h) * vs) * sm, wp = (L(a.vort, ES_CVORT_PHI, h) * vs) * cm;
        c[h][ES_CVAR_VORT_X][e] = wr * ct - wp * st;
        c[h][ES_CVAR_VORT_Y][e] = wr * st + wp * ct;
      }
      if (mask & bit(ES_CVAR_VORT_Z)) c[h][ES_CVAR_VORT_Z][e] = (L(a.vort, ES_CVORT_Z, h) * vs) * sm;
    }
  }

  const int item0 = (int)blockIdx.y * a.items_per_block;
  const int item1 = (item0 + a.items_per_block < n_items) ? item0 + a.items_per_block : n_items;
  for (int item = item0; item < item1; ++item) {
    const int tau = item / a.z_parts;
    const int l0 = (item - tau * a.z_parts) * a.z_chunk;
    const int l1 = (l0 + a.z_chunk < a.n_z) ? l0 + a.z_chunk : a.n_z;
    int slot = 0;
#pragma unroll
    for (int v = 0; v < ES_CVAR_COUNT; ++v) {
      if (!((mask >> v) & 1u)) continue;
      const size_t plane = ((size_t)tau * a.n_sel + slot) * (size_t)a.n_z;
      ++slot;
      for (int l = l0; l < l1; ++l) {
        const size_t zt = (size_t)tau * a.n_z + l;
        const double EC = tab[zt], ES = tab[n_zt + zt];
        uint32_t b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = f32_bits(c[0][v][e] * EC - c[1][v][e] * ES, SWAP);
        fill_invalid(b, valid, a.fill_bits);
        store4<WIDE>(out + (plane + l) * a.n_pts, pt, b, live);
      }
    }
  }
}

}  // namespace

extern "C" int es_cyl_complex_vorticity_amplitudes(es_context* ctx, const double* d_radius, const double* d_amp, int n,
                                                   int n_nodes, int n_ext, int m, const double* d_k, double* d_vort) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, n >= 0 && n_nodes >= 0 && n_ext >= 0, "negative size");
  ES_REQUIRE(ctx, m >= 0, "m");
  ES_REQUIRE(ctx, n_nodes == 0 || n_nodes >= 3, "the interior needs at least 3 points for its radial derivative");
  ES_REQUIRE(ctx, n_ext == 0 || n_ext >= 3, "the exterior needs at least 3 points for its radial derivative");
  const size_t n_r = (size_t)n_nodes + (size_t)n_ext;
  ES_REQUIRE(ctx, n_r < 0x7fffffffull, "too many radial points");
  if (n == 0 || n_r == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_radius && d_amp && d_k && d_vort, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t tot = (size_t)n * n_r;
  ES_REQUIRE(ctx, (tot + 255) / 256 <= 0x7fffffffull, "too many points");
  hipLaunchKernelGGL(cylcart_vorticity_amplitudes_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream,
                     d_radius, d_amp, d_k, n, n_nodes, n_ext, (double)m, d_vort);
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
  ES_REQUIRE(ctx, n_nodes >= 0 && n_ext >= 0 && n_x >= 0 && n_y >= 0 && n_z >= 0 && n_t >= 0, "negative size");
  ES_REQUIRE(ctx, m >= 0, "m");
  ES_REQUIRE(ctx, var_mask != 0, "empty variable mask");
  ES_REQUIRE(ctx, (var_mask >> ES_CVAR_COUNT) == 0, "unknown variable bit");
  ES_REQUIRE(ctx, (flags & ES_FIELD_Z_REFERENCE_ANGLE) == 0,
             "ES_FIELD_Z_REFERENCE_ANGLE is not offered on the Cartesian mesh (its curl is another one)");
  ES_REQUIRE(ctx, (flags & ~ES_FIELD_BIG_ENDIAN) == 0, "flags");
  ES_REQUIRE(ctx, n_nodes == 0 || n_nodes >= 3, "the interior needs at least 3 points");
  ES_REQUIRE(ctx, n_ext == 0 || n_ext >= 3, "the exterior needs at least 3 points");
  const size_t n_r = (size_t)n_nodes + (size_t)n_ext;
  ES_REQUIRE(ctx, n_r > 0 && n_r < 0x7fffffffull, "radial table size");
  const uint32_t vort_bits = bit(ES_CVAR_VORT_X) | bit(ES_CVAR_VORT_Y) | bit(ES_CVAR_VORT_Z);
  ES_REQUIRE(ctx, !(var_mask & vort_bits) || d_vort, "a vorticity variable needs d_vort");
  ES_REQUIRE(ctx, (size_t)n_z * (size_t)n_t < 0x7fffffffull, "mesh too large");
  ES_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_out) & 3u) == 0, "float32 output needs 4-byte alignment");
  if (n_x == 0 || n_y == 0 || n_z == 0 || n_t == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_radius && d_amp && d_x && d_y && d_z && d_t && d_out, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double* tab;
  int rc = zt_tables<true>(ctx, d_z, n_z, d_t, n_t, k, w_re, w_im, &tab);
  if (rc) return rc;
  const bool swap = (flags & ES_FIELD_BIG_ENDIAN) != 0;
  CCartArgs a;
  a.radius = d_radius; a.amp = d_amp; a.vort = d_vort; a.x = d_x; a.y = d_y;
  a.N = n_nodes; a.n_ext = n_ext; a.m = m; a.n_x = n_x; a.n_z = n_z; a.n_t = n_t;
  a.n_sel = __builtin_popcount(var_mask);
  a.iters = bisection_iters(n_nodes > n_ext ? n_nodes : n_ext);
  a.fill_bits = fill_bits_of(fill, swap);
  a.mask = var_mask; a.v_scale = v_scale;
  a.n_pts = (size_t)n_x * (size_t)n_y;
  int pieces, groups;
  rc = es_cyl_cartesian_split(n_x, n_y, n_z, n_t, &pieces, &a.z_chunk, &a.z_parts, &a.items_per_block, &groups);
  ES_REQUIRE(ctx, rc == ES_SUCCESS, "mesh too large");
  const bool wide = (a.n_pts % 4 == 0) && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
  const dim3 grid((unsigned)pieces, (unsigned)groups), block(64);
  uint32_t* out = reinterpret_cast<uint32_t*>(d_out);
  auto kernel = ES_SWAP_WIDE_KERNEL(cylcart_synthesis_kernel, swap, wide);
  hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, a, tab, out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
