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
#include "es_field_shared.hpp"

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
struct CartArgs {
  const double* radius; const double* amp; const double* vort;   // [n_r], [7 x n_r], [5 x n_r] (NULL without vorticity)
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

// One wave per workgroup.  The (y, x) points of a z plane are contiguous in d_out (x fastest), so the plane is walked as
// one array of n_x n_y points in pieces of 256: no tail per row.  A lane owns four points of its piece and finds, once,
// their r, angle factors and interpolated amplitudes; it keeps per selected variable the coefficient of cos(k z - w t)
// (and of sin(k z - w t) for vort_x, vort_y) in registers and then walks its (frame, z piece) items, variable outer and z
// planes inner, so that a wave's consecutive stores stay in one variable's block.  Nothing is read back.  The (z, t) table
// and the output are __restrict__ kernel arguments so that cos / sin(k z - w t) arrive by scalar loads and the loop waits on
// them alone, not on the vector-memory counter its own stores share.
//   WIDE  (every plane starts on a 16-byte boundary: n_x n_y a multiple of 4 and d_out aligned) the lane owns four
//         consecutive points: one 16-byte store per lane, 1 KiB per wave-instruction;
//   else  the lane owns the points lane, lane + 64, lane + 128, lane + 192 of the piece: four 4-byte stores, each
//         wave-instruction 256 contiguous bytes whatever the alignment -- not the 16-byte-strided dwords that four
//         consecutive points per lane would give (slower on the 267 x 267 mesh in its one run).
// The tables (13 n_r doubles at most) are read from global memory: a lane reads 8 x 13 entries at most, far fewer than
// staging the tables in LDS would move per one-wave workgroup.  That is an argument from counts; an LDS-staged variant
// has not been built or measured.
template <bool SWAP, bool WIDE>
__global__ __launch_bounds__(64) void cartesian_synthesis_kernel(CartArgs a, const double* __restrict__ tab,
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
  double cC[ES_CVAR_COUNT][4], cS[2][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int v = 0; v < ES_CVAR_COUNT; ++v) cC[v][e] = 0.0;
    cS[0][e] = 0.0; cS[1][e] = 0.0;
    if (!((valid >> e) & 1u)) continue;
    const int j = lo[e];
    const double r = rr[e];
    const Lerp lerp(r, rad[j], rad[j + 1]);
    auto L = [&](const double* __restrict__ tabv, int c) {
      return lerp(tabv[(size_t)c * n_r + j], tabv[(size_t)c * n_r + j + 1]);
    };
    const double ct = xv[e] / r, st = yv[e] / r;
    double cm = 1.0, sm = 0.0;                         // cos(m theta), sin(m theta) by angle addition
    for (int s = 0; s < a.m; ++s) {
      const double c2 = cm * ct - sm * st, s2 = sm * ct + cm * st;
      cm = c2; sm = s2;
    }
    const double fs = -sm;
    if (mask & bit(ES_CVAR_P_T)) cC[ES_CVAR_P_T][e] = L(a.amp, ES_AMP_P_T) * cm;
    if (mask & (bit(ES_CVAR_XI_X) | bit(ES_CVAR_XI_Y))) {
      const double pr = L(a.amp, ES_AMP_XI_R) * cm, pp = L(a.amp, ES_AMP_XI_PHI) * fs;
      cC[ES_CVAR_XI_X][e] = pr * ct - pp * st;
      cC[ES_CVAR_XI_Y][e] = pr * st + pp * ct;
    }
    if (mask & bit(ES_CVAR_XI_Z)) cC[ES_CVAR_XI_Z][e] = L(a.amp, ES_AMP_XI_Z) * cm;
    if (mask & (bit(ES_CVAR_V_X) | bit(ES_CVAR_V_Y))) {
      const double pr = (L(a.amp, ES_AMP_V_R) * vs) * cm, pp = (L(a.amp, ES_AMP_V_PHI) * vs) * fs;
      cC[ES_CVAR_V_X][e] = pr * ct - pp * st;
      cC[ES_CVAR_V_Y][e] = pr * st + pp * ct;
    }
    if (mask & bit(ES_CVAR_V_Z)) cC[ES_CVAR_V_Z][e] = (L(a.amp, ES_AMP_V_Z) * vs) * cm;
    if (mask & (bit(ES_CVAR_VORT_X) | bit(ES_CVAR_VORT_Y))) {
      const double wrc = (L(a.vort, ES_VORT_R_C) * vs) * sm, wrs = (L(a.vort, ES_VORT_R_S) * vs) * sm;
      const double wpc = (L(a.vort, ES_VORT_PHI_C) * vs) * cm, wps = (L(a.vort, ES_VORT_PHI_S) * vs) * cm;
      cC[ES_CVAR_VORT_X][e] = wrc * ct - wpc * st;
      cS[0][e] = wrs * ct - wps * st;
      cC[ES_CVAR_VORT_Y][e] = wrc * st + wpc * ct;
      cS[1][e] = wrs * st + wps * ct;
    }
    if (mask & bit(ES_CVAR_VORT_Z)) cC[ES_CVAR_VORT_Z][e] = (L(a.vort, ES_VORT_Z_C) * vs) * sm;
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
        const double C = tab[zt];
        uint32_t b[4];
        if (v == ES_CVAR_VORT_X || v == ES_CVAR_VORT_Y) {
          const double S = tab[n_zt + zt];
          const int sv = (v == ES_CVAR_VORT_X) ? 0 : 1;
#pragma unroll
          for (int e = 0; e < 4; ++e) b[e] = f32_bits(cC[v][e] * C + cS[sv][e] * S, SWAP);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) b[e] = f32_bits(cC[v][e] * C, SWAP);
        }
        fill_invalid(b, valid, a.fill_bits);
        store4<WIDE>(out + (plane + l) * a.n_pts, pt, b, live);
      }
    }
  }
}

}  // namespace

extern "C" int es_cyl_vorticity_amplitudes(es_context* ctx, const double* d_radius, const double* d_amp, int n,
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
  hipLaunchKernelGGL(vorticity_amplitudes_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream,
                     d_radius, d_amp, d_k, n, n_nodes, n_ext, (double)m, d_vort);
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
  int rc = zt_tables<false>(ctx, d_z, n_z, d_t, n_t, k, w, 0.0, &tab);
  if (rc) return rc;
  const bool swap = (flags & ES_FIELD_BIG_ENDIAN) != 0;
  CartArgs a;
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
  const size_t gx = (size_t)pieces;
  const unsigned gy = (unsigned)groups;
  const bool wide = (a.n_pts % 4 == 0) && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
  const dim3 grid((unsigned)gx, gy), block(64);
  uint32_t* out = reinterpret_cast<uint32_t*>(d_out);
  auto kernel = ES_SWAP_WIDE_KERNEL(cartesian_synthesis_kernel, swap, wide);
  hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, a, tab, out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
