// K2: uniform cylinder in closed form -- the determinant D(k, omega; m) from Bessel functions, one grid point per lane.
//
// Restates, for the uniform limit the reference uses as its benchmark case (profile width 1e5, CF:126, CD-C:125 with
// dr = 1e5), what the workers compute numerically (CF:694-804):
//   interior  P'' + P'/r - (m_i + m^2/r^2) P = 0 ,  m_i = (k^2 vA^2 - Om^2)(k^2 c^2 - Om^2)/((c^2+vA^2)(k^2 cT^2 - Om^2)),
//             Om = omega - k U_i        (the general coefficient set of CF:577-626 reduces to this)
//             -> P = f1(kappa |r|) + beta f2(kappa |r|),  (f1, f2) = (I_m, K_m) for m_i > 0, (J_m, Y_m) for m_i < 0,
//             beta from the axis condition at r_axis: P = 0 (kink, CF:795 with B_phi = 0) or P' = 0 (sausage, CF:1092)
//   xi_i = P' / (rho_i (Om^2 - k^2 vA^2))   (xi = (C1 P + D P')/C3 with C1 = 0, C3 = D rho (Om^2 - wA^2), CF:798)
//   exterior and mismatch exactly as in the shooting path (exterior_cylinder).
#include "es_common.hpp"
#include "es_shoot_device.hpp"
#include "es_refine_rule.hpp"

namespace {

struct UniDev {
  double c2, vA2, rho_i, U_i, S, cT2;
  double r_sign, r_axis;
  int axis_bc;
};

__device__ __forceinline__ double pick_w_u(const double* __restrict__ wv, int w_mode, double k, int row, int nw, int iw) {
  if (w_mode == ES_W_PHASE_SPEED) return k * wv[iw];
  if (w_mode == ES_W_PER_ROW) return wv[(size_t)row * nw + iw];
  return wv[iw];
}

// d ln P / d|r| at |r| = 1 of the interior solution that satisfies the axis condition at r_axis.
__device__ __forceinline__ double interior_logder(const UniDev& U, int m, double m_i, bool& singular) {
  const double dm = (double)m;
  singular = false;
  if (m_i > 0.0) {
    const double kap = sqrt(m_i), xa = kap * U.r_axis, xb = kap;
    double Ib, Ib1, Kb, Kb1, Ia, Ia1, Ka, Ka1;
    esb::ke_pair(m, xb, Kb, Kb1);  esb::ie_pair_from_k(m, xb, Kb, Kb1, Ib, Ib1);
    esb::ke_pair(m, xa, Ka, Ka1);  esb::ie_pair_from_k(m, xa, Ka, Ka1, Ia, Ia1);
    const double dIb = Ib1 + (dm / xb) * Ib, dKb = -Kb1 + (dm / xb) * Kb;      // scaled derivatives
    const double dIa = Ia1 + (dm / xa) * Ia, dKa = -Ka1 + (dm / xa) * Ka;
    // P = I + beta K ; in scaled form beta K(xb)/I(xb) carries exp(-2 (xb - xa))
    const double E2 = exp(-2.0 * (xb - xa));
    const double g = (U.axis_bc == ES_AXIS_SAUSAGE) ? -(dIa / dKa) : -(Ia / Ka);
    const double num = dIb + E2 * g * dKb;
    const double den = Ib + E2 * g * Kb;
    return kap * num / den;
  } else if (m_i < 0.0) {
    const double kap = sqrt(-m_i), xa = kap * U.r_axis, xb = kap;
    double Jb, Jb1, Yb, Yb1, Ja, Ja1, Ya, Ya1;
    esb::jy_pair(m, xb, Jb, Jb1, Yb, Yb1);
    esb::jy_pair(m, xa, Ja, Ja1, Ya, Ya1);
    const double dJb = -Jb1 + (dm / xb) * Jb, dYb = -Yb1 + (dm / xb) * Yb;
    const double dJa = -Ja1 + (dm / xa) * Ja, dYa = -Ya1 + (dm / xa) * Ya;
    const double g = (U.axis_bc == ES_AXIS_SAUSAGE) ? -(dJa / dYa) : -(Ja / Ya);
    return kap * (dJb + g * dYb) / (Jb + g * Yb);
  }
  singular = true;
  return NAN;
}

// D, rel and status of ONE point for the interior order m and the exterior order m_ext (every other field of P and U as
// given).  The only evaluation site of the closed form: the grid kernel, the fused evaluate-and-flag kernel of the root
// search, its bracket-end kernel and its refinement all call it, so a value that two of them compute is the same bits
// (the build has -ffp-contract=off: the arithmetic does not depend on what the function is inlined into).
__device__ __forceinline__ void uni_point(const ShootDev& P0, const UniDev& U, int m, int m_ext, double k, double w,
                                          double& D, double& rel, uint8_t& st) {
  ShootDev P = P0;
  P.m = m; P.m_ext = m_ext;
  const Exterior X = exterior_cylinder(P, k, w, w);
  const double k2 = k * k;
  const double Om = w - k * U.U_i;
  const double Om2 = Om * Om;
  const double m_i = ((k2 * U.vA2 - Om2) * (k2 * U.c2 - Om2)) / (U.S * (k2 * U.cT2 - Om2));
  st = (uint8_t)X.status;
  D = NAN; rel = NAN;
  if (X.status == ES_PT_OK) {
    bool sing;
    const double ld = interior_logder(U, m, m_i, sing);              // d ln P / d|r|
    const double Pb = X.yb;
    const double dPdr = U.r_sign * ld * Pb;                          // dP/dr in the signed coordinate
    const double xi_i = dPdr / (U.rho_i * (Om2 - k2 * U.vA2));
    const double xi_e = X.cst * X.dyb;
    D = xi_e - xi_i;
    rel = fabs(D) * 100.0 / fmax(fabs(xi_e), fabs(xi_i));
    if (sing || !isfinite(D)) { st = ES_PT_NONFINITE; }
  }
}

__global__ __launch_bounds__(256) void cyl_uniform_kernel(ShootDev P, UniDev U, const double* __restrict__ kv, int nk,
                                                          const double* __restrict__ wv, int nw, int w_mode,
                                                          double* __restrict__ Dout, double* __restrict__ relout,
                                                          uint8_t* __restrict__ stout) {
  const int iw = blockIdx.x * 256 + threadIdx.x;
  for (int row = blockIdx.y; row < nk; row += gridDim.y) {
    if (iw >= nw) continue;
    const double k = kv[row];
    const double w = pick_w_u(wv, w_mode, k, row, nw, iw);
    double D, rel; uint8_t st;
    uni_point(P, U, P.m, P.m_ext, k, w, D, rel, st);
    const size_t o = (size_t)row * nw + iw;
    Dout[o] = D;
    stout[o] = st;
    if (relout) relout[o] = rel;
  }
}

// ---- root search over (m, k, omega): es_cyl_uniform_find_roots ------------------------------------------------------------
// Rows of the search are (order, k-row) pairs, row = io * nk + ik, order outer.  A wave owns a TILE of one row: 63 cells
// (omega_j, omega_j+1) plus the halo point of the last cell, j = 63 t + lane.  Every lane evaluates its own point once, the
// upper end of a cell comes from lane + 1 by shuffle, and lane 63 -- whose point is lane 0 of the next tile -- never owns a
// cell: no lane evaluates a second point, no D array is read back, and a wave costs 64 evaluations for 63 cells.  Rows have
// T = ceil((nw - 1) / 63) tiles (at least one), so a tile never spans two rows or two orders.  Cells are numbered by their
// SLOT, 64 (row * T + t) + lane: slots increase with (order, row, omega), which is all the ordered compaction of
// es_cell_rank needs, and a workgroup of four tiles is one block of 256 slots.
constexpr int UNI_TILE = 63;
inline int uni_tiles_per_row(int nw) { return nw > 1 ? (int)(((long)nw - 2) / UNI_TILE) + 1 : 1; }

struct UniGrid {
  const double* kv; const double* wv;
  int nk, nw, w_mode, m_first;
  long rows;          // n_orders * nk
  int tiles_per_row;  // T
};

__global__ __launch_bounds__(256) void cyl_uniform_flag_kernel(ShootDev P, UniDev U, UniGrid G, double* __restrict__ Dout,
                                                               uint8_t* __restrict__ stout, uint64_t* __restrict__ masks,
                                                               int* __restrict__ block_counts) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long tile = (long)blockIdx.x * 4 + wave;                       // wave-uniform
  const long row = tile / G.tiles_per_row;
  bool flag = false;
  if (row < G.rows) {
    const int t = (int)(tile - row * G.tiles_per_row);
    const int io = (int)(row / G.nk), ik = (int)(row - (long)io * G.nk);
    const int j = t * UNI_TILE + lane;
    const bool in = j < G.nw;
    const double k = G.kv[ik];
    const double w = in ? pick_w_u(G.wv, G.w_mode, k, ik, G.nw, j) : 1.0;
    const int m = G.m_first + io;
    double D, rel; uint8_t st;
    uni_point(P, U, m, m, k, w, D, rel, st);
    const int ok0 = in && st == ES_PT_OK;
    const double d1 = __shfl_down(D, 1);
    const int ok1 = __shfl_down(ok0, 1);
    // lane 63 owns no cell; the last point of a row has no upper neighbour (ok1 = 0 there: j + 1 >= nw)
    flag = lane < UNI_TILE && ok0 && ok1 && (D * d1 < 0.0);
    // lane 63's point is stored by the next tile, which has it as lane 0 -- unless this is the last tile of the row
    if (in && (lane < UNI_TILE || t == G.tiles_per_row - 1)) {
      const size_t o = (size_t)row * G.nw + j;
      if (Dout) Dout[o] = D;
      if (stout) stout[o] = st;
    }
  }
  es_flag_block(flag, 64 * tile + lane, masks, block_counts);         // slot of this lane: masks[tile]
}

// record `pos` of the table = the pos-th flagged slot: k, row, order and the two grid frequencies of the cell
__global__ __launch_bounds__(256) void cyl_uniform_emit_kernel(UniGrid G, const uint64_t* __restrict__ masks,
                                                               const int* __restrict__ block_off, es_root_table tab,
                                                               int32_t* __restrict__ d_order) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const long tile = s >> 6;
  const int lane = (int)(s & 63);
  const int pos = es_flagged_pos(masks, block_off, s, 64 * G.rows * G.tiles_per_row, tab.capacity);
  if (pos < 0) return;
  const long row = tile / G.tiles_per_row;
  const int t = (int)(tile - row * G.tiles_per_row);
  const int io = (int)(row / G.nk), ik = (int)(row - (long)io * G.nk);
  const int j = t * UNI_TILE + lane;
  const double k = G.kv[ik];
  tab.d_k[pos] = k;
  tab.d_row[pos] = (int32_t)ik;
  if (d_order) d_order[pos] = (int32_t)(G.m_first + io);
  tab.d_w_lo[pos] = pick_w_u(G.wv, G.w_mode, k, ik, G.nw, j);
  tab.d_w_hi[pos] = pick_w_u(G.wv, G.w_mode, k, ik, G.nw, j + 1);
}

// D at the two ends of every bracket, recomputed by uni_point from the k and omega the emit kernel wrote (the doubles the
// flag kernel evaluated: the same bits, whether or not the caller keeps the grid), one lane per end, into the d_w (lower
// end) and d_resid (upper end) columns, which hold them until the refinement overwrites both.
__global__ __launch_bounds__(256) void cyl_uniform_ends_kernel(ShootDev P, UniDev U, es_root_table tab,
                                                               const int32_t* __restrict__ d_order, int m_first,
                                                               const int* __restrict__ d_n, int n_max) {
  const int n = *d_n < n_max ? *d_n : n_max;
  if ((int)(blockIdx.x * 128) >= n) return;                                               // workgroup-uniform
  const int i = blockIdx.x * 128 + ((int)threadIdx.x >> 1), e = threadIdx.x & 1;
  const bool in = i < n;
  const double k = in ? tab.d_k[i] : 1.0;
  const double w = in ? (e ? tab.d_w_hi[i] : tab.d_w_lo[i]) : 1.0;
  const int m = (in && d_order) ? d_order[i] : m_first;
  double D, rel; uint8_t st;
  uni_point(P, U, m, m, k, w, D, rel, st);
  if (in) (e ? tab.d_resid : tab.d_w)[i] = D;
}

// The ES_REFINE_SECTION rule (es_refine_rule.hpp, the text refine_kernel + refine_polish_kernel of es_refine.hip use) with the
// closed form as the evaluation: 16 lanes per bracket, n_rounds rounds of 17-section steered by a wave ballot, then
// UNI_POLISH regula-falsi steps in which the 16 lanes of a bracket evaluate the same secant point (an evaluation is a few
// Bessel calls: two rounds in twelve at a sixteenth of their use cost less than two more launches).  One evaluation site.
// Count from device memory, launch sized for the capacity; workgroups beyond the count return at once.
constexpr int UNI_LANES = 16;
constexpr int UNI_POLISH = 2;

__global__ __launch_bounds__(256) void cyl_uniform_refine_kernel(ShootDev P, UniDev U, es_root_table tab,
                                                                 const int32_t* __restrict__ d_order, int m_first,
                                                                 const int* __restrict__ d_n, int n_max, int n_rounds,
                                                                 double tol_percent) {
  constexpr int GROUPS = 64 / UNI_LANES;
  const int n = *d_n < n_max ? *d_n : n_max;
  if ((int)(blockIdx.x * 4 * GROUPS) >= n) return;                                        // workgroup-uniform
  const int lane = threadIdx.x & 63;
  const int g = lane / UNI_LANES, j = lane % UNI_LANES;
  const int i = (blockIdx.x * 4 + ((int)threadIdx.x >> 6)) * GROUPS + g;
  const bool in = i < n;
  const double k = in ? tab.d_k[i] : 1.0;
  const int m = (in && d_order) ? d_order[i] : m_first;
  es_bracket b = {in ? tab.d_w_lo[i] : 1.0, in ? tab.d_w_hi[i] : 2.0, in ? tab.d_w[i] : 1.0, in ? tab.d_resid[i] : -1.0};
  const double frac = es_section_frac<UNI_LANES>(j);
  double D = 0.0, rel = 0.0; uint8_t st = 0;
  double root = b.lo;
  for (int it = 0; it < n_rounds + UNI_POLISH; ++it) {
    const bool section = it < n_rounds;
    const double x = section ? es_section_point(b, frac) : es_secant_point(b);
    uni_point(P, U, m, m, k, x, D, rel, st);
    if (section) {
      b = es_section_update<UNI_LANES>(b, x, D, g);
    } else {
      root = x;
      b = es_secant_update(b, x, D);
    }
  }
  if (in && j == 0) {
    tab.d_w_lo[i] = b.lo;
    tab.d_w_hi[i] = b.hi;
    tab.d_w[i] = root;
    tab.d_resid[i] = rel;
    tab.d_flag[i] = es_accept_flag(st, rel, tol_percent);
  }
}


}  // namespace

namespace {
int check_uniform_params(es_context* ctx, const es_cyl_uniform_params* p, int nk, int nw, int w_mode) {
  ES_REQUIRE(ctx, p != nullptr, "null params");
  ES_REQUIRE(ctx, nk >= 0 && nw >= 0, "negative size");
  ES_REQUIRE(ctx, w_mode >= 0 && w_mode <= 2, "w_mode");
  ES_REQUIRE(ctx, p->r_boundary == -1.0 || p->r_boundary == 1.0, "r_boundary must be -1 or +1");
  ES_REQUIRE(ctx, p->r_axis > 0.0 && p->r_axis < 1.0, "r_axis");
  ES_REQUIRE(ctx, p->axis_bc == ES_AXIS_KINK || p->axis_bc == ES_AXIS_SAUSAGE, "axis_bc");
  return ES_SUCCESS;
}

void uniform_device_params(const es_cyl_uniform_params* p, ShootDev& S, UniDev& U) {
  memset(&S, 0, sizeof(S));
  S.family = FAM_CYL0;
  S.xb = p->r_boundary;
  S.rho_e = p->rho_e; S.vAe2 = p->vA_e * p->vA_e; S.ce2 = p->c_e * p->c_e; S.cTe2 = p->cT_e * p->cT_e;
  S.Se = S.vAe2 + S.ce2;
  S.R_factor = p->L_factor * 2.0 * 3.14159265358979323846;
  S.ic0 = p->ic_value; S.ic1 = p->ic_slope;
  S.m = p->m; S.m_ext = p->m_ext; S.axis_bc = p->axis_bc;
  U.c2 = p->c_i * p->c_i; U.vA2 = p->vA_i * p->vA_i; U.rho_i = p->rho_i; U.U_i = p->U_i;
  U.S = U.c2 + U.vA2; U.cT2 = U.c2 * U.vA2 / U.S;
  U.r_sign = p->r_boundary; U.r_axis = p->r_axis; U.axis_bc = p->axis_bc;
}

// Argument checks shared by the two searches; *empty: nothing to search (count 0).
int check_uniform_search(es_context* ctx, const es_cyl_uniform_params* p, int m_first, int n_orders, const double* d_k,
                         int nk, const double* d_w, int nw, int w_mode, int n_bisect, const es_root_table* table,
                         const int32_t* d_order, bool* empty) {
  int rc = check_uniform_params(ctx, p, nk, nw, w_mode);
  if (rc) return rc;
  ES_REQUIRE(ctx, n_orders >= 0 && n_bisect >= 0, "negative size");
  ES_REQUIRE(ctx, m_first >= 0 && (long)m_first + n_orders - 1 <= 64, "orders must lie in 0 .. 64");
  ES_REQUIRE(ctx, table, "null pointer");
  ES_REQUIRE(ctx, table->capacity >= 0, "negative size");
  ES_REQUIRE(ctx, table->capacity == 0 || (table->d_k && table->d_w && table->d_w_lo && table->d_w_hi &&
                                           table->d_resid && table->d_row && table->d_flag),
             "null root table arrays");
  ES_REQUIRE(ctx, d_order || n_orders <= 1, "d_order is required for more than one order");
  *empty = (long)n_orders * nk * nw == 0;
  if (!*empty) {
    ES_REQUIRE(ctx, d_k && d_w, "null pointer");
    const long rows = (long)n_orders * nk;
    const long tiles = rows * uni_tiles_per_row(nw);
    ES_REQUIRE(ctx, tiles <= (1L << 32), "grid too large for one call");
  }
  return ES_SUCCESS;
}

// fused evaluate-and-flag + scan + emit + bracket ends + refinement, everything enqueued: the bracket count is left in
// ctx->d_total, and d_n (ctx->d_total or the caller's copy of it) is where the kernels sized for the capacity read it
int uniform_search_enqueue(es_context* ctx, const es_cyl_uniform_params* p, int m_first, int n_orders, const double* d_k,
                           int nk, const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent, double* d_D,
                           uint8_t* d_status, const es_root_table* table, int32_t* d_order, int32_t* d_count) {
  ShootDev S; UniDev U;
  uniform_device_params(p, S, U);
  UniGrid G;
  G.kv = d_k; G.wv = d_w; G.nk = nk; G.nw = nw; G.w_mode = w_mode; G.m_first = m_first;
  G.rows = (long)n_orders * nk;
  G.tiles_per_row = uni_tiles_per_row(nw);
  const long tiles = G.rows * G.tiles_per_row;
  const int nblocks = (int)((tiles + 3) / 4);
  int rc = es_ensure_scan_scratch(ctx, (size_t)nblocks * 256);
  if (rc) return rc;
  hipLaunchKernelGGL(cyl_uniform_flag_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, S, U, G, d_D, d_status,
                     ctx->d_masks, ctx->d_block_counts);
  ES_HIP_CHECK(ctx, hipGetLastError());
  rc = es_scan_block_counts_async(ctx, nblocks);
  if (rc) return rc;
  const int* d_n = ctx->d_total;
  if (d_count) {
    ES_HIP_CHECK(ctx, hipMemcpyAsync(d_count, ctx->d_total, sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    d_n = d_count;                                     // ctx->d_total is reused by the next call on this context
  }
  const int cap = table->capacity;
  if (cap > 0) {
    hipLaunchKernelGGL(cyl_uniform_emit_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, G, ctx->d_masks,
                       ctx->d_block_counts, *table, d_order);
    hipLaunchKernelGGL(cyl_uniform_ends_kernel, dim3((cap + 127) / 128), dim3(256), 0, ctx->stream, S, U, *table, d_order,
                       m_first, d_n, cap);
    const int rounds = es_section_rounds(n_bisect, UNI_LANES + 1);      // the count of launch_refine (es_refine.hip)
    constexpr int PER_WG = 4 * (64 / UNI_LANES);
    hipLaunchKernelGGL(cyl_uniform_refine_kernel, dim3((cap + PER_WG - 1) / PER_WG), dim3(256), 0, ctx->stream, S, U,
                       *table, d_order, m_first, d_n, cap, rounds, tol_percent);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  return ES_SUCCESS;
}
}  // namespace

extern "C" int es_cyl_uniform_eval(es_context* ctx, const es_cyl_uniform_params* p, const double* d_k, int nk,
                                   const double* d_w, int nw, int w_mode, double* d_D, double* d_rel,
                                   uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_uniform_params(ctx, p, nk, nw, w_mode);
  if (rc) return rc;
  ES_REQUIRE(ctx, p->m >= 0 && p->m <= 64 && p->m_ext >= 0 && p->m_ext <= 64, "m");
  if (nk == 0 || nw == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w && d_D && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ShootDev S; UniDev U;
  uniform_device_params(p, S, U);
  dim3 grid((nw + 255) / 256, nk < 65535 ? nk : 65535), block(256);
  hipLaunchKernelGGL(cyl_uniform_kernel, grid, block, 0, ctx->stream, S, U, d_k, nk, d_w, nw, w_mode, d_D, d_rel, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_cyl_uniform_find_roots(es_context* ctx, const es_cyl_uniform_params* p, int m_first, int n_orders,
                                         const double* d_k, int nk, const double* d_w, int nw, int w_mode, int n_bisect,
                                         double tol_percent, double* d_D, uint8_t* d_status, es_root_table* table,
                                         int32_t* d_order, int* h_count) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, h_count, "null pointer");
  bool empty = false;
  int rc = check_uniform_search(ctx, p, m_first, n_orders, d_k, nk, d_w, nw, w_mode, n_bisect, table, d_order, &empty);
  if (rc) return rc;
  *h_count = 0;
  if (empty) return ES_SUCCESS;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  rc = uniform_search_enqueue(ctx, p, m_first, n_orders, d_k, nk, d_w, nw, w_mode, n_bisect, tol_percent, d_D, d_status,
                              table, d_order, nullptr);
  if (rc) return rc;
  // the one read-back of this entry point
  ES_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_total, ctx->d_total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ES_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  *h_count = *ctx->h_total;
  return *h_count > table->capacity ? ES_ERR_CAPACITY : ES_SUCCESS;
}

extern "C" int es_cyl_uniform_find_roots_async(es_context* ctx, const es_cyl_uniform_params* p, int m_first, int n_orders,
                                               const double* d_k, int nk, const double* d_w, int nw, int w_mode,
                                               int n_bisect, double tol_percent, double* d_D, uint8_t* d_status,
                                               es_root_table* table, int32_t* d_order, int32_t* d_count) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, d_count, "null pointer");
  bool empty = false;
  int rc = check_uniform_search(ctx, p, m_first, n_orders, d_k, nk, d_w, nw, w_mode, n_bisect, table, d_order, &empty);
  if (rc) return rc;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (empty) {
    ES_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), ctx->stream));
    return ES_SUCCESS;
  }
  return uniform_search_enqueue(ctx, p, m_first, n_orders, d_k, nk, d_w, nw, w_mode, n_bisect, tol_percent, d_D, d_status,
                                table, d_order, d_count);
}
