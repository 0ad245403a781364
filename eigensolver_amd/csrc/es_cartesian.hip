// Cartesian sampling of a cylinder mode, with its vorticity (include/eigensolver_amd.h section 8): the fourth stage of the
// reference, which flattens the polar mesh, hands it to scipy.interpolate.griddata and differences the result with
// np.gradient along the index axes (Cylinder/Non-uniform flow/Coronal/Movies/Vorticity_gaussian_flow.py:1190-1262).
// A mode is A(r) trig(m theta) trig(k z - w t): at a Cartesian point r and the angle factors are computed directly, only
// the radial amplitudes are interpolated (linearly, separately on each side of the interface), and the curl of the
// product form is a closed expression in the amplitudes and their radial derivatives.
//   es_cyl_vorticity_amplitudes   v_r, v_phi, v_z amplitudes -> the five radial amplitudes of curl v; one lane per
//                                 (mode, radial point); derivatives by three-point formulas per region
//   es_cyl_cartesian_synthesis    amplitudes of one mode -> float32 frames [t][variable][z][y][x]; the (x, y) stage
//                                 (hypot, search, interpolation) once per point, then bound by store bandwidth
#include "es_cartesian_shared.hpp"

namespace {

// ---- v amplitudes -> amplitudes of curl v ---------------------------------------------------------------------------
// d/dr is np.gradient(a, r, edge_order=2) of each region on its own (gradient_stencil).
__global__ __launch_bounds__(256) void vorticity_amplitudes_kernel(const double* __restrict__ radius,
                                                                  const double* __restrict__ amp,
                                                                  const double* __restrict__ kk, int n, int N, int n_ext,
                                                                  double dm, double* __restrict__ vort) {
  const size_t n_r = (size_t)N + (size_t)n_ext;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * n_r) return;
  const size_t i = t / n_r;
  const int j = (int)(t - i * n_r);
  const int base = (j < N) ? 0 : N;
  const int len = (j < N) ? N : n_ext;                 // >= 3 (checked by the host)
  const int q = j - base;
  const double* r = radius + i * n_r + base;
  const double* A = amp + i * (size_t)ES_AMP_COUNT * n_r + base;
  const Stencil3 g = gradient_stencil(r, q, len);
  const int p = g.p;
  const double* az = A + (size_t)ES_AMP_V_Z * n_r;
  const double* ap = A + (size_t)ES_AMP_V_PHI * n_r;
  const double d_az = (g.c0 * az[p] + g.c1 * az[p + 1]) + g.c2 * az[p + 2];
  const double d_ap = (g.c0 * ap[p] + g.c1 * ap[p + 1]) + g.c2 * ap[p + 2];
  const double rq = r[q], a_r = A[(size_t)ES_AMP_V_R * n_r + q], a_p = ap[q], a_z = az[q], k = kk[i];
  double* V = vort + i * (size_t)ES_VORT_COUNT * n_r + j;
  V[ES_VORT_R_C * n_r] = -(dm * a_z) / rq;
  V[ES_VORT_R_S * n_r] = -(k * a_p);
  V[ES_VORT_PHI_C * n_r] = -d_az;
  V[ES_VORT_PHI_S * n_r] = -(k * a_r);
  V[ES_VORT_Z_C * n_r] = ((dm * a_r - a_p) - rq * d_ap) / rq;
}

// ---- amplitudes -> frames on the (x, y, z, t) mesh ------------------------------------------------------------------
// Launch shape, (x, y) stage and item walk: es_cartesian_shared.hpp.  A lane keeps per selected variable the coefficient
// of cos(k z - w t) (and of sin(k z - w t) for vort_x, vort_y) of its four points in registers.  The (z, t) table and the
// output stay __restrict__ kernel arguments, so that the phase factors arrive by scalar loads (cart_walk says why).
template <bool SWAP, bool WIDE>
__global__ __launch_bounds__(64) void cartesian_synthesis_kernel(CartArgs a, const double* __restrict__ tab,
                                                                uint32_t* __restrict__ out) {
  const size_t n_zt = (size_t)a.n_z * a.n_t;
  CartLane s;
  if (!cart_stage<WIDE>(a, s)) return;
  double cC[ES_CVAR_COUNT][4], cS[2][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int v = 0; v < ES_CVAR_COUNT; ++v) cC[v][e] = 0.0;
    cS[0][e] = 0.0; cS[1][e] = 0.0;
    if (!((s.valid >> e) & 1u)) continue;
    const CartPoint p = cart_point(a, s, e);
    cart_amp_coefficients<1>(a, p, 0, e, cC);
    const double vs = a.v_scale, ct = p.ct, st = p.st, cm = p.cm, sm = p.sm;
    if (a.mask & (bit(ES_CVAR_VORT_X) | bit(ES_CVAR_VORT_Y))) {
      const double wrc = (p.L<1>(a.vort, ES_VORT_R_C, 0) * vs) * sm, wrs = (p.L<1>(a.vort, ES_VORT_R_S, 0) * vs) * sm;
      const double wpc = (p.L<1>(a.vort, ES_VORT_PHI_C, 0) * vs) * cm, wps = (p.L<1>(a.vort, ES_VORT_PHI_S, 0) * vs) * cm;
      cC[ES_CVAR_VORT_X][e] = wrc * ct - wpc * st;
      cS[0][e] = wrs * ct - wps * st;
      cC[ES_CVAR_VORT_Y][e] = wrc * st + wpc * ct;
      cS[1][e] = wrs * st + wps * ct;
    }
    if (a.mask & bit(ES_CVAR_VORT_Z)) cC[ES_CVAR_VORT_Z][e] = (p.L<1>(a.vort, ES_VORT_Z_C, 0) * vs) * sm;
  }
  cart_walk<WIDE>(a, out, s, [&](int v, size_t zt, uint32_t (&b)[4]) {
    const double C = tab[zt];
    if (v == ES_CVAR_VORT_X || v == ES_CVAR_VORT_Y) {
      const double S = tab[n_zt + zt];
      const int sv = (v == ES_CVAR_VORT_X) ? 0 : 1;
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = f32_bits(cC[v][e] * C + cS[sv][e] * S, SWAP);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = f32_bits(cC[v][e] * C, SWAP);
    }
  });
}

}  // namespace

extern "C" int es_cyl_vorticity_amplitudes(es_context* ctx, const double* d_radius, const double* d_amp, int n,
                                           int n_nodes, int n_ext, int m, const double* d_k, double* d_vort) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  unsigned blocks;
  const int rc = vorticity_args(ctx, d_radius, d_amp, n, n_nodes, n_ext, m, d_k, d_vort, blocks);
  if (rc || !blocks) return rc;
  hipLaunchKernelGGL(vorticity_amplitudes_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_radius, d_amp, d_k, n, n_nodes,
                     n_ext, (double)m, d_vort);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

// Workgroups over (piece of 256 points, group of (frame, z piece) items): about 16 waves per CU, so that every CU streams,
// and no more, because each workgroup repeats the (x, y) stage of its points.
extern "C" int es_cyl_cartesian_split(int n_x, int n_y, int n_z, int n_t, int* pieces, int* z_chunk, int* z_parts,
                                      int* items_per_group, int* groups) {
  if (n_x <= 0 || n_y <= 0 || n_z <= 0 || n_t <= 0 || !pieces || !z_chunk || !z_parts || !items_per_group || !groups)
    return ES_ERR_INVALID_ARG;
  const size_t gx = ((size_t)n_x * (size_t)n_y + 255) / 256;
  if (gx > 0x7fffffffull) return ES_ERR_INVALID_ARG;
  const size_t want = 4096;
  size_t wy = (want + gx - 1) / gx;                      // item groups wanted
  size_t parts = (wy + (size_t)n_t - 1) / (size_t)n_t;   // pieces per frame (1 when the frames alone give enough items)
  if (parts > (size_t)n_z) parts = (size_t)n_z;
  const int chunk = (int)(((size_t)n_z + parts - 1) / parts);
  const int zp = (n_z + chunk - 1) / chunk;
  const size_t items = (size_t)n_t * zp;
  if (items >= 0x7fffffffull) return ES_ERR_INVALID_ARG;
  if (wy > items) wy = items;
  if (wy > 65535) wy = 65535;
  const int ipg = (int)((items + wy - 1) / wy);          // the same number of items for every workgroup but the last
  *pieces = (int)gx; *z_chunk = chunk; *z_parts = zp; *items_per_group = ipg;
  *groups = (int)((items + ipg - 1) / ipg);
  return ES_SUCCESS;
}

extern "C" int es_cyl_cartesian_synthesis(es_context* ctx, const double* d_radius, const double* d_amp,
                                          const double* d_vort, int n_nodes, int n_ext, int m, double k, double w,
                                          const double* d_x, int n_x, const double* d_y, int n_y, const double* d_z,
                                          int n_z, const double* d_t, int n_t, uint32_t var_mask, double v_scale,
                                          float fill, int flags, float* d_out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  CartLaunch L;
  bool none;
  const int rc = cartesian_args<false>(ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, 0.0, d_x, n_x, d_y, n_y, d_z, n_z,
                                       d_t, n_t, var_mask, v_scale, fill, flags, d_out, L, none);
  if (rc || none) return rc;
  hipLaunchKernelGGL(ES_SWAP_WIDE_KERNEL(cartesian_synthesis_kernel, L.swap, L.wide), L.grid, dim3(64), 0, ctx->stream, L.a,
                     L.tab, L.out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
