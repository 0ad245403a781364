// K3: shooting evaluation of D(k, omega) in fp64, on a (k, omega) grid and at a list of points (es_shoot_eval_grid*,
// es_shoot_eval_points).  See es_shoot_device.hpp for the arithmetic and include/eigensolver_amd.h for the reference lines
// each entry point replaces.  The rest of the shooting path: es_refine.hip (K5: 17-section + secant refinement),
// es_screen.hip (fp32 screening march), es_roots.hip (K4: bracket detection, ordered root compaction, the search
// pipelines, exchange packing), es_problem.hip (problem handle); what crosses these files: es_shoot_host.hpp.
//
// Kernel layout (DESIGN.md section "kernels"):
//  * shoot_grid_kernel<FAM, PTS, MAXT, TRACK, WPE>: one workgroup per tile = (k-row, omega-segment of T * PTS points), omega
//    along the lanes (PTS points per lane, strided by the workgroup size so the 8-byte D stores of a wave are one
//    contiguous 512 B segment).  k is workgroup uniform, so everything that depends on (node, k, m) but not on omega is
//    computed ONCE per tile into an LDS table, chunk by chunk (CH RK4 steps per chunk); every lane then reads the same
//    LDS address (broadcast).  Launch shapes per family: pick_shape(); the launch has exactly one workgroup per tile
//    (es_tile_grid).  Families with fam_rcp4() take two RK4 steps per division (coefficients4).
//  * shoot_points_kernel<FAM>: one (k, omega) pair per lane with unrelated k: the k-independent base table is
//    staged in LDS chunk by chunk (es_shoot_shared.hpp: shoot_point), node entries are formed per lane.
//  * Every kernel that works on a list (points, brackets) takes (d_n, n_max) and starts with n = es_count(d_n, n_max)
//    (es_common.hpp): the launch is sized for n_max, the count is n_max itself (d_n == nullptr: the host knows it) or is
//    read from device memory (the asynchronous searches: n_max is the grid size or the table capacity).
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <type_traits>

#include "es_shoot_host.hpp"

namespace {
using namespace es_shoot_shared;

// ------------------------------------------------------------------------------------------------------------
// Options of one grid launch: skip = ES_EVAL_SKIP_CONTINUUM; cols != nullptr: only the omega-columns cols[1 .. cols[0]]
// are evaluated (live-column list built on the device by column_classify_kernel), the others were filled beforehand.
// part (compacted launches only): 0 = every segment; 1 = the full segments of a row; 2 = the columns behind the last
// full segment of width main_span, in segments of this launch's own (narrower) workgroups.  A partly filled segment in
// a 4-wave workgroup costs as much as a full one: its live wave shares a SIMD with two waves of other workgroups, and
// those workgroups are tied by their barriers to the pace of that SIMD, so the idle wave slots buy nothing; given to
// one-wave workgroups of a second launch, the remainder costs what its waves cost.
struct GridOpts {
  int skip;
  const int* cols;
  int part;
  int main_span;
};

// ROWS = 2: a workgroup holds TWO k-rows, waves 0, 1 the first and waves 2, 3 the second (128 lanes x PTS points each; its
// own LDS table per row).  A workgroup should have four waves, one per SIMD of its CU: the waves of a workgroup are tied to
// each other by the barriers around every LDS chunk, so a CU filled with three-wave workgroups runs at the pace of the SIMD
// that got four waves while another got two -- measured on 4096 rows, N = 2001, ns per point-step relative to rows of 1024
// frequencies (4 points x 256 lanes): 768 (4 x 192 lanes) 1.17, 384 (2 x 192) 1.17, 512 (4 x 128) 1.39, 256 (4 x 64) 1.83
// (tools/probe/time_row_width.py).  Rows of at most 128 x PTS frequencies therefore go two to a workgroup.
template <int FAM, int PTS, int MAXT, bool TRACK, int WPE = 0>
__global__ __launch_bounds__(MAXT) __attribute__((amdgpu_waves_per_eu(WPE ? WPE : 1, WPE ? WPE : 8)))
void shoot_grid_kernel(ShootDev P, const double* __restrict__ kv, int nk,
                                                          const double* __restrict__ wv, int nw, int w_mode,
                                                          double* __restrict__ Dout, double* __restrict__ relout,
                                                          uint8_t* __restrict__ stout, GridOpts opts) {
  constexpr int ROWS = 1;
#include "es_shoot_grid_body.hpp"
}

// two k-rows per workgroup (ROWS = 2): 256 threads, never compacted launches
template <int FAM, int PTS, bool TRACK, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void shoot_grid_kernel_r2(ShootDev P, const double* __restrict__ kv, int nk,
                                                          const double* __restrict__ wv, int nw, int w_mode,
                                                          double* __restrict__ Dout, double* __restrict__ relout,
                                                          uint8_t* __restrict__ stout, GridOpts opts) {
  constexpr int ROWS = 2;
  constexpr int MAXT = 256;
#include "es_shoot_grid_body.hpp"
}

// ---- ES_EVAL_SKIP_CONTINUUM with ES_W_PHASE_SPEED: whole omega-columns inside a continuum band ----------------------
// band_crossed() tests W' = (k W)/k, which is W up to the two roundings of the product and the quotient (|W' - W| <= 2
// ulp).  A column is removed from the launch only if W is inside a band by more than that for every k:
//     W - m > min lo  and  W + m < max hi  and  (W + m <= max lo  or  W - m >= min hi),      m = 4 ulp(W);
// columns within the margin of a band edge stay in the launch and are flagged point by point as before.
__device__ __forceinline__ bool column_dead(const ShootDev& P, double W) {
  const double m = 4.0 * 2.220446049250313e-16 * fabs(W);
  bool c = false;
  for (int t = 0; t < P.n_bands; ++t) {
    const bool some = (W - m > P.band[t][0]) && (W + m < P.band[t][3]);
    const bool notall = (W + m <= P.band[t][1]) || (W - m >= P.band[t][2]);
    c = c || (some && notall);
  }
  return c;
}

// One workgroup: dead flag per column + ordered list of the live columns (cols[0] = count, cols[1..] = indices).
__global__ __launch_bounds__(1024) void column_classify_kernel(ShootDev P, const double* __restrict__ Wv, int nw,
                                                               int* __restrict__ cols, uint8_t* __restrict__ dead) {
  __shared__ int wave_cnt[16];
  __shared__ int base;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int j0 = 0; j0 < nw; j0 += 1024) {
    const int j = j0 + tid;
    const bool in = j < nw;
    const bool dd = in && column_dead(P, Wv[j]);
    if (in) dead[j] = dd ? 1 : 0;
    const bool live = in && !dd;
    const uint64_t m = __ballot(live);
    if (lane == 0) wave_cnt[wid] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int v = 0; v < wid; ++v) off += wave_cnt[v];
    const uint64_t lower = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    if (live) cols[1 + off + __popcll(m & lower)] = j;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int v = 0; v < 16; ++v) t += wave_cnt[v]; base += t; }
    __syncthreads();
  }
  if (tid == 0) cols[0] = base;
}

// D = rel = NaN, status = CONTINUUM at every point of a dead column (status of a leaky / singular exterior takes
// precedence, exactly as finish_point() orders them: the exterior is evaluated here, it is cheap next to a march).
__global__ __launch_bounds__(256) void fill_dead_columns_kernel(ShootDev P, const double* __restrict__ kv, int nk,
                                                                const double* __restrict__ wv, int nw,
                                                                const uint8_t* __restrict__ dead,
                                                                double* __restrict__ Dout, double* __restrict__ relout,
                                                                uint8_t* __restrict__ stout) {
  const long cells = (long)nk * nw;
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long)gridDim.x * blockDim.x) {
    const long row = c / nw;
    const int j = (int)(c - row * nw);
    if (!dead[j]) continue;
    const double k = kv[row];
    const double w = k * wv[j];
    // exterior status from m_e and the exterior constant alone (the Bessel evaluation is not needed for it)
    const double k2 = k * k;
    const double Oe = (P.family == FAM_CYL0 || P.family == FAM_CYLT) ? w : (w - k * P.U_e);
    const double Oe2 = Oe * Oe;
    const double m_e = ((k2 * P.vAe2 - Oe2) * (k2 * P.ce2 - Oe2)) / (P.Se * (k2 * P.cTe2 - Oe2));
    const double cst = (P.family == FAM_CYL0 || P.family == FAM_CYLT)
                           ? -1.0 / (P.rho_e * (k2 * P.vAe2 - w * w))
                           : P.rho_e * P.Se * (k2 * P.cTe2 - Oe2) / (Oe * (k2 * P.ce2 - Oe2));
    uint8_t st = ES_PT_CONTINUUM;
    if (m_e < 0.0) st = ES_PT_LEAKY;
    else if (!(m_e > 0.0) || !isfinite(m_e) || !isfinite(cst)) st = ES_PT_NONFINITE;
    Dout[c] = NAN;
    if (relout) relout[c] = NAN;
    stout[c] = st;
  }
}

// One workgroup per 256 points of the launch bound.  The early exit is workgroup-uniform and comes before shoot_point's
// LDS staging, whose barriers every lane of a live workgroup reaches.
template <int FAM>
__global__ __launch_bounds__(256) void shoot_points_kernel(ShootDev P, const double* __restrict__ kv,
                                                           const double* __restrict__ wv, const int* __restrict__ d_n,
                                                           int n_max, double* __restrict__ Dout,
                                                           double* __restrict__ relout, uint8_t* __restrict__ stout) {
  ES_POINT_LDS(FAM);
  const int n = es_count(d_n, n_max);
  if ((long)blockIdx.x * 256 >= (long)n) return;                                          // workgroup-uniform
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const double k = in ? kv[i] : 1.0;
  const double w = in ? wv[i] : 1.0;
  double D, rel; uint8_t st;
  shoot_point<FAM>(P, k, w, w, D, rel, st, es_point_lds);
  if (in) {
    Dout[i] = D;
    stout[i] = st;
    if (relout) relout[i] = rel;
  }
}

// Launch shape of the grid kernel = (PTS points per lane, WPE waves per SIMD the register cap allows).  Every shape runs
// workgroups of at most 256 threads (one wave per SIMD of a CU) over tiles (k-row, omega-segment of T * PTS points) and
// parks the exterior results in LDS during the march, so the register cap 512 / WPE is the march loop's alone:
//   WPE = 2 -> 256 VGPRs, 3 -> 168, 4 -> 128.
// Round 2 picked between 1024-, 512- and 256-thread shapes by row width only; the 1024-thread ones (128 VGPRs by launch
// bounds) spilled 12 - 89 VGPRs inside the march loop of every family but the untwisted cylinder with one point per lane --
// exactly the shapes BASELINE configs[1] and configs[4] (1024 columns) selected.  Now every family has its own table of
// spill-free shapes (tools/codeobj_table.py prints registers / spills / LDS of each built instantiation;
// tests/test_codeobj.py fails on a spill in a shape the table selects) and the cost of a point in each of them, measured
// on the GPU (tools/probe/time_grid_shapes.py -> profiles/r3_grid_shapes.json); pick_shape() minimises
// padded points x cost per point for the row width at hand.  ES_GRID_SHAPE="pts,wpe" in the environment overrides it
// (tuning aid).  D does not depend on the shape: a point's arithmetic is the same in all of them
// (tests/test_shoot_gpu.py::test_grid_shapes_bit_identical).
struct GridShape { int pts, wpe; };

// Per family, indexed by points per lane (1, 2, 4): the register cap paired with it and the relative cost of one point,
// measured on the grids of the BASELINE configs (profiles/r3_grid_shapes.json: min of three launches, MI355X; all nine
// (points, cap) combinations per family bit-identical).  Reading of that table: with the spills gone the shapes of one
// family lie within 15 % of each other -- every one of them runs at 0.85 - 1.0 of the issue bound of its own instruction
// stream (tools/isa_loop_count.py) -- so the choice is about padding (a row of 384 frequencies fills 2 points x 192 lanes
// exactly, 4 points x 128 lanes waste a quarter) and about not spilling; four points per lane share the LDS reads and
// the loop overhead best.  WPE = 4 is used where the kernel fits 128 registers without a spill.
template <int FAM> struct ShapeTable;
// (untwisted cylinder: three points per lane are built for rows of 513 - 768 frequencies = 3 x 256 lanes, a four-wave workgroup
// where 4 x 192 lanes make a three-wave one.  For a row of 384 frequencies, configs[2], 3 x 128 lanes was measured too: 1.28 ms per
// launch against 1.14 ms for 2 x 192: its two-wave workgroups hold 39 KB of LDS each, four fit a CU, two waves per SIMD;
// measured again at the end of round 3 with a 128-thread instantiation -- 27 KB of LDS, 145 registers, two steps per division --:
// 1.12 - 1.14 ms against 1.08 - 1.10 ms for 2 x 192, configs[2] 7.18 - 7.25 against 7.24 ms per step; what rows of 384 needed was a
// four-wave workgroup: two rows each, shoot_grid_kernel_r2, 0.99 ms.  The other families keep wpe[3] = 0.)
// (measured again after the kernels became one tile per workgroup -- es_tile_index -- which freed 40 - 90 registers per
// shape: profiles/r3e_grid_shapes.json, ms per launch, best register cap per point count)
//   untwisted cylinder 1024 x 4096: 4 pts 5.03 (wpe 3), 2 pts 5.14, 1 pt 5.46; 4096 x 384: 2 pts x 192 lanes 1.27 (wpe 4; 1.32
//   at wpe 3), 4 pts x 128 lanes 1.80
template <> struct ShapeTable<FAM_CYL0>  { static constexpr int wpe[5] = {0, 4, 3, 3, 3}; static constexpr double cost[5] = {0, 1.09, 1.025, 1.01, 1.0}; };
// twisted cylinder 1024 x 1024, N = 2000: 4 pts 6.60 (200 registers, two workgroups per CU), 2 pts 6.70, 1 pt 6.85 (7.8 - 8.2
// for every shape while the tile loop was there)
template <> struct ShapeTable<FAM_CYLT>  { static constexpr int wpe[5] = {0, 3, 2, 0, 2}; static constexpr double cost[5] = {0, 1.04, 1.015, 0, 1.0}; };
// density slab 1024 x 1024: 4 pts 1.45 (wpe 3), 2 pts 1.62 (wpe 4), 1 pt 1.75 (wpe 4)
template <> struct ShapeTable<FAM_SLABD> { static constexpr int wpe[5] = {0, 4, 4, 0, 3}; static constexpr double cost[5] = {0, 1.20, 1.12, 0, 1.0}; };
// flow slab 1024 x 1024: 4 pts 1.28 (wpe 3), 2 pts 1.25 (wpe 4), 1 pt 1.33 (wpe 2): within the noise of one another
template <> struct ShapeTable<FAM_SLABF> { static constexpr int wpe[5] = {0, 2, 4, 0, 3}; static constexpr double cost[5] = {0, 1.04, 1.0, 0, 1.0}; };

inline int shape_threads(int nw, int pts) {
  int T = ((nw + pts - 1) / pts + 63) / 64 * 64;
  if (T < 64) T = 64;
  if (T > 256) T = 256;
  return T;
}

template <int FAM>
GridShape pick_shape(int nw, bool track) {
  GridShape best{4, 2};
  double best_cost = 1e300;
  for (int pts : {4, 3, 2, 1}) {
    if (ShapeTable<FAM>::wpe[pts] == 0) continue;      // not a shape of this family
    const int T = shape_threads(nw, pts);
    const long span = (long)T * pts;
    const long padded = (nw + span - 1) / span * span;
    // workgroups of fewer than four waves do not load the four SIMDs of a CU evenly and their waves wait for each other at
    // the chunk barriers: ns per point-step against four-wave workgroups, measured (tools/probe/time_row_width.py)
    static const double wave_count_cost[5] = {0.0, 1.83, 1.39, 1.17, 1.0};
    const double c = (double)padded * ShapeTable<FAM>::cost[pts] * wave_count_cost[T / 64];
    if (c < best_cost) { best_cost = c; best = GridShape{pts, ShapeTable<FAM>::wpe[pts]}; }
  }
  // per-node sign tracking of a band family (profiles whose continuum intervals do not overlap): 6 - 12 more registers
  // per point; the 256-register shapes hold them without a spill
  if (track && fam_has_bands<FAM>()) best.wpe = 2;
  if (const char* ev = getenv("ES_GRID_SHAPE")) {
    int p = 0, w = 0;
    if (sscanf(ev, "%d,%d", &p, &w) == 2 && p >= 1 && p <= 4 && w >= 2 && w <= 4) best = GridShape{p, w};
  }
  return best;
}

// which (PTS, WPE, TRACK) instantiations are built: the shapes the tables select, the tracking fall-backs at WPE = 2, and
// (-DES_ALL_GRID_SHAPES, the measuring build of tools/probe/time_grid_shapes.py) everything ES_GRID_SHAPE can name
template <int FAM, int PTS, int WPE, bool TRACK>
constexpr bool shape_built() {
  if (PTS == 3 && ShapeTable<FAM>::wpe[3] == 0) return false;
#if defined(ES_ALL_GRID_SHAPES)
  return true;
#else
  if (TRACK && fam_has_bands<FAM>()) return WPE == 2;
  if (FAM == FAM_CYL0 && PTS == 4 && WPE == 2) return true;   // A/B aid for the headline shape (ES_GRID_SHAPE=4,2: 175 VGPRs, no spill)
  return ShapeTable<FAM>::wpe[PTS] == WPE;
#endif
}

// rows of at most 512 frequencies of the band families (untwisted cylinder, slabs) go two to a four-wave workgroup
// (shoot_grid_kernel_r2: 128 lanes x ceil(nw / 128) points per row) unless the problem needs per-node sign tracking; ES_GRID_ROWS2=0 and ES_GRID_SHAPE select
// the one-row shapes (A/B aids)
template <int FAM>
bool rows2_shape(int nw, bool track) {
  if (!fam_has_bands<FAM>() || track || nw > 512) return false;
  const char* r2 = getenv("ES_GRID_ROWS2");
  return !(r2 && r2[0] == '0') && !getenv("ES_GRID_SHAPE");
}

template <int FAM>
int launch_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk, const double* d_w, int nw,
                int w_mode, double* d_D, double* d_rel, uint8_t* d_status, int flags = 0) {
  GridOpts opts;
  opts.skip = (flags & ES_EVAL_SKIP_CONTINUUM) ? 1 : 0;
  opts.cols = nullptr;
  opts.part = 0;
  opts.main_span = 0;
  if (opts.skip && w_mode == ES_W_PHASE_SPEED && fam_has_bands<FAM>() && prob->dev.use_bands) {
    // live-column list on the device, dead columns filled at once; the grid launch below is sized for all nw
    // columns (the count stays on the device), workgroups beyond the live ones return immediately
    if ((size_t)nw + 1 > ctx->cols_cap) {
      ES_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
      if (ctx->d_cols) ES_HIP_CHECK(ctx, hipFree(ctx->d_cols));
      if (ctx->d_coldead) ES_HIP_CHECK(ctx, hipFree(ctx->d_coldead));
      ctx->d_cols = nullptr; ctx->d_coldead = nullptr; ctx->cols_cap = 0;
      ES_HIP_CHECK(ctx, hipMalloc(&ctx->d_cols, ((size_t)nw + 1) * sizeof(int)));
      ES_HIP_CHECK(ctx, hipMalloc(&ctx->d_coldead, (size_t)nw));
      ctx->cols_cap = (size_t)nw + 1;
    }
    hipLaunchKernelGGL(column_classify_kernel, dim3(1), dim3(1024), 0, ctx->stream, prob->dev, d_w, nw, ctx->d_cols,
                       ctx->d_coldead);
    ES_HIP_CHECK(ctx, hipGetLastError());
    const long cells = (long)nk * nw;
    const int fb = (int)((cells + 255) / 256 < 8192 ? (cells + 255) / 256 : 8192);
    hipLaunchKernelGGL(fill_dead_columns_kernel, dim3(fb), dim3(256), 0, ctx->stream, prob->dev, d_k, nk, d_w, nw,
                       ctx->d_coldead, d_D, d_rel, d_status);
    ES_HIP_CHECK(ctx, hipGetLastError());
    opts.cols = ctx->d_cols;
  }
  // families with connected continuum bands: no per-node sign tracking (band_crossed)
  const bool track = !(fam_has_bands<FAM>() && prob->dev.use_bands);
  GridShape shape = pick_shape<FAM>(nw, track);
  const int T = shape_threads(nw, shape.pts);
  const long tiles = (long)nk * ((nw + (long)T * shape.pts - 1) / ((long)T * shape.pts));
  const dim3 grid = es_tile_grid(tiles);
  bool launched = false;
  es_timer_begin(ctx);
  if constexpr (fam_has_bands<FAM>()) {
    if (rows2_shape<FAM>(nw, track) && !opts.cols && nk >= 2) {
      const int pts2 = (nw + 127) / 128;
      const dim3 grid2 = es_tile_grid(((long)nk + 1) / 2);
#define ES_R2(P_)                                                                                                   \
      if (pts2 == P_) hipLaunchKernelGGL((shoot_grid_kernel_r2<FAM, P_, false, 3>), grid2, dim3(256), 0, ctx->stream, \
                                         prob->dev, d_k, nk, d_w, nw, w_mode, d_D, d_rel, d_status, opts);
      ES_R2(1) ES_R2(2) ES_R2(3) ES_R2(4)
#undef ES_R2
      launched = true;
    }
  }
  auto one = [&](auto pts_c, auto wpe_c, auto track_c) {
    constexpr int PTS = decltype(pts_c)::value, WPE = decltype(wpe_c)::value;
    constexpr bool TRACK = decltype(track_c)::value;
    if constexpr (shape_built<FAM, PTS, WPE, TRACK>() && (TRACK || fam_has_bands<FAM>())) {
      if (launched || shape.pts != PTS || shape.wpe != WPE || track != TRACK) return;
      launched = true;
      if constexpr (FAM == FAM_CYL0 && PTS == 4 && !TRACK) {
        if (opts.cols && T > 64) {
          // compacted launch: full segments in 4-wave workgroups, the remainder of each row in one-wave workgroups
          opts.part = 1;
          hipLaunchKernelGGL((shoot_grid_kernel<FAM, PTS, 256, TRACK, WPE>), grid, dim3(T), 0, ctx->stream,
                             prob->dev, d_k, nk, d_w, nw, w_mode, d_D, d_rel, d_status, opts);
          opts.part = 2;
          opts.main_span = 4 * T;
          const long tiles2 = (long)nk * (T / 64);
          hipLaunchKernelGGL((shoot_grid_kernel<FAM, 4, 64, false, 2>), es_tile_grid(tiles2),
                             dim3(64), 0, ctx->stream, prob->dev, d_k, nk, d_w, nw, w_mode, d_D, d_rel, d_status, opts);
          return;
        }
      }
      hipLaunchKernelGGL((shoot_grid_kernel<FAM, PTS, 256, TRACK, WPE>), grid, dim3(T), 0, ctx->stream, prob->dev,
                         d_k, nk, d_w, nw, w_mode, d_D, d_rel, d_status, opts);
    }
  };
  using std::integral_constant;
#define ES_SHAPE(P_, W_)                                                                                            \
  one(integral_constant<int, P_>{}, integral_constant<int, W_>{}, integral_constant<bool, false>{});                \
  one(integral_constant<int, P_>{}, integral_constant<int, W_>{}, integral_constant<bool, true>{});
  ES_SHAPE(4, 2) ES_SHAPE(4, 3) ES_SHAPE(4, 4) ES_SHAPE(3, 2) ES_SHAPE(3, 3) ES_SHAPE(2, 2) ES_SHAPE(2, 3) ES_SHAPE(2, 4) ES_SHAPE(1, 2) ES_SHAPE(1, 3) ES_SHAPE(1, 4)
#undef ES_SHAPE
  es_timer_end(ctx);
  if (!launched) {
    ctx->last_error = "grid launch shape not built (ES_GRID_SHAPE names a shape outside this build)";
    return ES_ERR_UNSUPPORTED;
  }
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

// fp64 evaluation of es_count(d_n, n_max) points, the launch sized for n_max (d_rel is optional)
template <int FAM>
int launch_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, const int* d_n, long n_max,
                  double* d_D, double* d_rel, uint8_t* d_status) {
  hipLaunchKernelGGL((shoot_points_kernel<FAM>), es_blocks(n_max), dim3(256), 0, ctx->stream, prob->dev, d_k, d_w, d_n,
                     es_bound(n_max), d_D, d_rel, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace

int dispatch_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, const int* d_n, long n_max,
                    double* d_D, double* d_rel, uint8_t* d_status) {
#define CALL_PTS(F) launch_points<F>(ctx, prob, d_k, d_w, d_n, n_max, d_D, d_rel, d_status)
  ES_DISPATCH_FAMILY(prob->dev.family, CALL_PTS)
#undef CALL_PTS
}

extern "C" int es_shoot_eval_grid_ex(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                     const double* d_w, int nw, int w_mode, int flags, double* d_D, double* d_rel,
                                     uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_problem(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, nk >= 0 && nw >= 0, "negative size");
  ES_REQUIRE(ctx, w_mode >= 0 && w_mode <= 2, "w_mode");
  ES_REQUIRE(ctx, (flags & ~ES_EVAL_SKIP_CONTINUUM) == 0, "unknown flags");
  if (nk == 0 || nw == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w && d_D && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define CALL_GRID(F) launch_grid<F>(ctx, prob, d_k, nk, d_w, nw, w_mode, d_D, d_rel, d_status, flags)
  ES_DISPATCH_FAMILY(prob->dev.family, CALL_GRID)
#undef CALL_GRID
}

// what launch_grid<FAM> picks for a row of nw frequencies
template <int FAM>
static int grid_shape_of(const es_problem* prob, int nw, int* h_pts, int* h_wpe, int* h_track) {
  const bool track = !(fam_has_bands<FAM>() && prob->dev.use_bands);
  const GridShape g = pick_shape<FAM>(nw, track);
  *h_pts = g.pts; *h_wpe = g.wpe; *h_track = track ? 1 : 0;
  if (rows2_shape<FAM>(nw, track)) { *h_pts = -((nw + 127) / 128); *h_wpe = 3; }
  return ES_SUCCESS;
}

extern "C" int es_shoot_grid_shape(es_context* ctx, const es_problem* prob, int nw, int* h_pts, int* h_wpe, int* h_track) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_problem(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, h_pts && h_wpe && h_track && nw > 0, "shape query arguments");
#define CALL_SHAPE(F) grid_shape_of<F>(prob, nw, h_pts, h_wpe, h_track)
  ES_DISPATCH_FAMILY(prob->dev.family, CALL_SHAPE)
#undef CALL_SHAPE
}

extern "C" int es_shoot_eval_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                  const double* d_w, int nw, int w_mode, double* d_D, double* d_rel,
                                  uint8_t* d_status) {
  return es_shoot_eval_grid_ex(ctx, prob, d_k, nk, d_w, nw, w_mode, 0, d_D, d_rel, d_status);
}

extern "C" int es_shoot_eval_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w,
                                    int n, double* d_D, double* d_rel, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_problem(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w && d_D && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return dispatch_points(ctx, prob, d_k, d_w, nullptr, n, d_D, d_rel, d_status);
}
