// What the two Cartesian sampling translation units share (es_cartesian.hip: section 8, a real mode;
// es_cyl_complex_cartesian.hip: section 20, an unstable mode at complex frequency): the argument block, the
// once-per-workgroup (x, y) stage with the region and tie rules, the coefficient text of the seven non-vorticity variables,
// the (frame, z piece) item walk and the host-side checks.  ONE text, so that a point cannot fall into another region in one
// family only.  Everything is in the unnamed namespace and force-inlined, so each unit compiles as if the text stood in its
// own file.
#pragma once
#include "es_field_shared.hpp"

namespace {

struct CartArgs {
  const double* radius; const double* amp; const double* vort;   // [n_r], [7 x n_r], [5 x n_r] (NULL without vorticity);
                                                       // complex: [7 x n_r x 2], [3 x n_r x 2], (re, im) pairs
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

// ---- the (x, y) stage -----------------------------------------------------------------------------------------------
// a lane's four points: index in the z plane, coordinates, r, the bracket (lo: its lower node after cart_stage); bit e of
// `live`: the point is in the mesh; of `valid`: it is inside the radial table as well
struct CartLane {
  size_t pt[4];
  double xv[4], yv[4], rr[4];
  int lo[4], hi[4];
  unsigned live, valid;
};

// One wave per workgroup.  The (y, x) points of a z plane are contiguous in d_out (x fastest), so the plane is walked as
// one array of n_x n_y points in pieces of 256: no tail per row.  A lane owns four points of its piece and finds, once,
// their r and bracket:
//   WIDE  (every plane starts on a 16-byte boundary: n_x n_y a multiple of 4 and d_out aligned) the lane owns four
//         consecutive points: one 16-byte store per lane, 1 KiB per wave-instruction;
//   else  the lane owns the points lane, lane + 64, lane + 128, lane + 192 of the piece: four 4-byte stores, each
//         wave-instruction 256 contiguous bytes whatever the alignment -- not the 16-byte-strided dwords that four
//         consecutive points per lane would give (slower on the 267 x 267 mesh in its one run).
// The tables (13 n_r doubles at most) are read from global memory: a lane reads 8 x 13 entries at most, far fewer than
// staging the tables in LDS would move per one-wave workgroup.  That is an argument from counts; an LDS-staged variant
// has not been built or measured.
// Returns false when the lane has no point in the mesh.
template <bool WIDE>
__device__ __forceinline__ bool cart_stage(const CartArgs& a, CartLane& s) {
  const size_t p0 = (size_t)blockIdx.x * 256;
  const int N = a.N, n_r = a.N + a.n_ext;
  const double* __restrict__ rad = a.radius;
  const double r_first = rad[0], r_last = rad[n_r - 1];
  const double r_b = (N > 0) ? rad[N - 1] : 0.0;       // boundary radius: r == r_b takes the interior values
  s.live = 0; s.valid = 0;
  // region: interior [r_first, r_b], exterior (r_b, r_last]; r = 0, the hole, the far field and NaN are outside
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s.pt[e] = p0 + (WIDE ? (size_t)threadIdx.x * 4 + e : (size_t)threadIdx.x + 64 * e);
    const bool in_mesh = s.pt[e] < a.n_pts;
    const size_t iy = in_mesh ? s.pt[e] / (size_t)a.n_x : 0;
    const size_t ix = in_mesh ? s.pt[e] - iy * (size_t)a.n_x : 0;
    s.xv[e] = a.x[ix];
    s.yv[e] = a.y[iy];
    const double r = hypot(s.xv[e], s.yv[e]);
    const bool in = N > 0 && r >= r_first && r <= r_b;
    const bool ex = a.n_ext > 0 && r <= r_last && (N > 0 ? r > r_b : r >= r_first);
    const bool ok = in_mesh && (in || ex) && r > 0.0;
    const int base = in ? 0 : N;
    s.rr[e] = r;
    s.lo[e] = base;
    s.hi[e] = ok ? base + (in ? N : a.n_ext) - 1 : base;
    s.live |= (in_mesh ? 1u : 0u) << e;
    s.valid |= (ok ? 1u : 0u) << e;
  }
  if (!s.live) return false;
  bracket4(rad, s.rr, s.lo, s.hi, a.iters);            // largest j of the region with rad[j] <= r, at most the last but one
  return true;
}

// ---- coefficients of a valid point ----------------------------------------------------------------------------------
// what the coefficient formulas of point e need: the interpolation in its bracket and the angle factors
struct CartPoint {
  Lerp lerp;
  size_t n_r; int j;
  double ct, st, cm, sm;                               // cos, sin of theta and of m theta
  // part h of channel ch of a table whose entries are PARTS interleaved doubles, interpolated
  template <int PARTS>
  __device__ __forceinline__ double L(const double* __restrict__ tabv, int ch, int h) const {
    return lerp(tabv[PARTS * ((size_t)ch * n_r + j) + h], tabv[PARTS * ((size_t)ch * n_r + j + 1) + h]);
  }
};

__device__ __forceinline__ CartPoint cart_point(const CartArgs& a, const CartLane& s, int e) {
  const double* __restrict__ rad = a.radius;
  const int j = s.lo[e];
  const double r = s.rr[e];
  const double ct = s.xv[e] / r, st = s.yv[e] / r;
  double cm = 1.0, sm = 0.0;                           // cos(m theta), sin(m theta) by angle addition
  for (int i = 0; i < a.m; ++i) {
    const double c2 = cm * ct - sm * st, s2 = sm * ct + cm * st;
    cm = c2; sm = s2;
  }
  return CartPoint{Lerp(r, rad[j], rad[j + 1]), (size_t)(a.N + a.n_ext), j, ct, st, cm, sm};
}

// P_T ... v_z of point e, part h of PARTS (1: a real table; 2: (re, im) pairs, each part formed as the real one is):
// the coefficient of cos(k z - w t), into c[variable][e]
template <int PARTS>
__device__ __forceinline__ void cart_amp_coefficients(const CartArgs& a, const CartPoint& p, int h, int e,
                                                      double (&c)[ES_CVAR_COUNT][4]) {
  const uint32_t mask = a.mask;
  const double vs = a.v_scale, ct = p.ct, st = p.st, cm = p.cm, fs = -p.sm;
  if (mask & bit(ES_CVAR_P_T)) c[ES_CVAR_P_T][e] = p.L<PARTS>(a.amp, ES_AMP_P_T, h) * cm;
  if (mask & (bit(ES_CVAR_XI_X) | bit(ES_CVAR_XI_Y))) {
    const double pr = p.L<PARTS>(a.amp, ES_AMP_XI_R, h) * cm, pp = p.L<PARTS>(a.amp, ES_AMP_XI_PHI, h) * fs;
    c[ES_CVAR_XI_X][e] = pr * ct - pp * st;
    c[ES_CVAR_XI_Y][e] = pr * st + pp * ct;
  }
  if (mask & bit(ES_CVAR_XI_Z)) c[ES_CVAR_XI_Z][e] = p.L<PARTS>(a.amp, ES_AMP_XI_Z, h) * cm;
  if (mask & (bit(ES_CVAR_V_X) | bit(ES_CVAR_V_Y))) {
    const double pr = (p.L<PARTS>(a.amp, ES_AMP_V_R, h) * vs) * cm, pp = (p.L<PARTS>(a.amp, ES_AMP_V_PHI, h) * vs) * fs;
    c[ES_CVAR_V_X][e] = pr * ct - pp * st;
    c[ES_CVAR_V_Y][e] = pr * st + pp * ct;
  }
  if (mask & bit(ES_CVAR_V_Z)) c[ES_CVAR_V_Z][e] = (p.L<PARTS>(a.amp, ES_AMP_V_Z, h) * vs) * cm;
}

// ---- the item walk --------------------------------------------------------------------------------------------------
// The lane's coefficients are in registers; it walks its (frame, z piece) items, variable outer and z planes inner, so
// that a wave's consecutive stores stay in one variable's block.  Nothing is read back.  values(v, zt, b) fills the four
// stored words of variable v at row zt of the (z, t) table.  That table and `out` are __restrict__ kernel arguments so
// that cos / sin(k z - w t) arrive by scalar loads and the loop waits on them alone, not on the vector-memory counter its
// own stores share.
template <bool WIDE, class Values>
__device__ __forceinline__ void cart_walk(const CartArgs& a, uint32_t* __restrict__ out, const CartLane& s, Values values) {
  const int n_items = a.n_t * a.z_parts;
  const int item0 = (int)blockIdx.y * a.items_per_block;
  const int item1 = (item0 + a.items_per_block < n_items) ? item0 + a.items_per_block : n_items;
  for (int item = item0; item < item1; ++item) {
    const int tau = item / a.z_parts;
    const int l0 = (item - tau * a.z_parts) * a.z_chunk;
    const int l1 = (l0 + a.z_chunk < a.n_z) ? l0 + a.z_chunk : a.n_z;
    int slot = 0;
#pragma unroll
    for (int v = 0; v < ES_CVAR_COUNT; ++v) {
      if (!((a.mask >> v) & 1u)) continue;
      const size_t plane = ((size_t)tau * a.n_sel + slot) * (size_t)a.n_z;
      ++slot;
      for (int l = l0; l < l1; ++l) {
        uint32_t b[4];
        values(v, (size_t)tau * a.n_z + l, b);
        fill_invalid(b, s.valid, a.fill_bits);
        store4<WIDE>(out + (plane + l) * a.n_pts, s.pt, b, s.live);
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// argument checks of the two vorticity-amplitude calls and their launch size, one lane per (mode, radial point);
// blocks == 0: nothing to do
inline int vorticity_args(es_context* ctx, const double* d_radius, const double* d_amp, int n, int n_nodes, int n_ext, int m,
                          const double* d_k, const double* d_vort, unsigned& blocks) {
  blocks = 0;
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
  blocks = (unsigned)((tot + 255) / 256);
  return ES_SUCCESS;
}

// What a synthesis call launches: workgroups of one wave over (piece of 256 points, group of (frame, z piece) items), the
// split of es_cyl_cartesian_split.
struct CartLaunch {
  CartArgs a;
  double* tab;                                         // the (z, t) table, in the context's scratch
  uint32_t* out;
  dim3 grid;
  bool swap, wide;
};

// argument checks of the two synthesis calls, the (z, t) table (GROWTH: with e^{w_im t}) enqueued on the context's stream
// and the launch; *none: nothing to write
template <bool GROWTH>
inline int cartesian_args(es_context* ctx, const double* d_radius, const double* d_amp, const double* d_vort, int n_nodes,
                          int n_ext, int m, double k, double w_re, double w_im, const double* d_x, int n_x,
                          const double* d_y, int n_y, const double* d_z, int n_z, const double* d_t, int n_t,
                          uint32_t var_mask, double v_scale, float fill, int flags, float* d_out, CartLaunch& L, bool& none) {
  none = true;
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
  int rc = zt_tables<GROWTH>(ctx, d_z, n_z, d_t, n_t, k, w_re, w_im, &L.tab);
  if (rc) return rc;
  L.swap = (flags & ES_FIELD_BIG_ENDIAN) != 0;
  CartArgs& a = L.a;
  a.radius = d_radius; a.amp = d_amp; a.vort = d_vort; a.x = d_x; a.y = d_y;
  a.N = n_nodes; a.n_ext = n_ext; a.m = m; a.n_x = n_x; a.n_z = n_z; a.n_t = n_t;
  a.n_sel = __builtin_popcount(var_mask);
  a.iters = bisection_iters(n_nodes > n_ext ? n_nodes : n_ext);
  a.fill_bits = fill_bits_of(fill, L.swap);
  a.mask = var_mask; a.v_scale = v_scale;
  a.n_pts = (size_t)n_x * (size_t)n_y;
  int pieces, groups;
  rc = es_cyl_cartesian_split(n_x, n_y, n_z, n_t, &pieces, &a.z_chunk, &a.z_parts, &a.items_per_block, &groups);
  ES_REQUIRE(ctx, rc == ES_SUCCESS, "mesh too large");
  L.wide = (a.n_pts % 4 == 0) && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
  L.grid = dim3((unsigned)pieces, (unsigned)groups);
  L.out = reinterpret_cast<uint32_t*>(d_out);
  none = false;
  return ES_SUCCESS;
}

}  // namespace
