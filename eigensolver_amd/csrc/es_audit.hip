// es_shoot_audit_screening (include/eigensolver_amd.h section 2): the fp32-screened grid against the fp64 grid, on the
// device.  A pure function of its arrays: nothing is marched, 26 bytes are read per cell (18 without rel64) and nothing
// of the size of the grid is written (DESIGN.md section 4a' has the measured rate).
//  * audit_cells_kernel: one cell per lane, 256-thread workgroups.  The omega-neighbour of the merged and of the fp64 point
//    comes through __shfl_down (lane 63 loads the halo element), as in bracket_flag_kernel; __ballot gives the mask of
//    flagged cells for the ordered table (the context's compaction scratch, es_cell_rank) and the eight counts; the two
//    extrema travel as (value, lane) through a wave reduction.  One 64-byte partial per workgroup.
//  * audit_reduce_kernel: one workgroup folds the partials into d_counts / d_worst.  Integer sums and (value, cell)
//    comparisons with ties to the smaller cell only, no floating-point atomics: the result does not depend on the order
//    in which workgroups ran.
//  * audit_emit_kernel: flagged cells -> (cell, kind) at their rank; the kind bits are recomputed from the arrays.
#include "es_common.hpp"

#include <cmath>
#include <limits>

namespace {

constexpr long NO_CELL = std::numeric_limits<long>::max();       // "no candidate yet" of an extremum; reported as -1

enum { N_FLAGGED = 0, N_MISSED, N_FALSE, N_STATUS, N_SIGN, N_VOUCHED_OK, N_UNSURE, N_BRACKETS64, N_COUNTS };

struct audit_partial {                                           // per workgroup, 64 bytes
  int32_t n[N_COUNTS];
  double margin, err;
  long margin_cell, err_cell;
};

// One grid point as the audit sees it: the merged grid is what the search brackets on.
struct audit_point {
  double d_scr, d64;
  uint8_t s_scr, s64;
  __device__ bool unsure() const { return (s_scr & ES_PT_SCREEN_UNSURE) != 0; }
  __device__ double d_merged() const { return unsure() ? d64 : d_scr; }
  __device__ uint8_t s_merged() const { return unsure() ? s64 : s_scr; }
  __device__ bool vouched_ok() const { return !unsure() && s_scr == ES_PT_OK && s64 == ES_PT_OK; }
};

__device__ __forceinline__ audit_point audit_load(const double* __restrict__ D_scr, const uint8_t* __restrict__ st_scr,
                                                  const double* __restrict__ D64, const uint8_t* __restrict__ st64,
                                                  long c) {
  return audit_point{D_scr[c], D64[c], st_scr[c], st64[c]};
}

// B(D, st) of the header: the predicate of bracket_flag_kernel (NaN products compare false).
__device__ __forceinline__ bool audit_bracket(bool inner, bool ok0, bool ok1, double d0, double d1) {
  return inner && ok0 && ok1 && (d0 * d1 < 0.0);
}

// Kind bits of the cell whose own point is p; (dm1, okm1) / (d641, ok641) are its omega-neighbour on the merged and on the
// fp64 grid, `inner` is j < nw - 1.  *b64 receives B(D64, st64).
__device__ __forceinline__ int audit_kind(const audit_point& p, bool inner, double dm1, bool okm1, double d641,
                                          bool ok641, bool* b64) {
  const bool bm = audit_bracket(inner, p.s_merged() == ES_PT_OK, okm1, p.d_merged(), dm1);
  *b64 = audit_bracket(inner, p.s64 == ES_PT_OK, ok641, p.d64, d641);
  int kind = 0;
  if (*b64 && !bm) kind |= ES_AUDIT_MISSED;
  if (bm && !*b64) kind |= ES_AUDIT_FALSE;
  if (!p.unsure() && p.s_scr != p.s64) kind |= ES_AUDIT_STATUS;
  if (p.vouched_ok() && (signbit(p.d_scr) != signbit(p.d64))) kind |= ES_AUDIT_SIGN;
  return kind;
}

// (value, index) candidates: `a` replaces `b` when it is the better extremum, ties to the smaller index; a NaN value is
// never a candidate (the callers do not offer one).
__device__ __forceinline__ bool better_min(double va, long ia, double vb, long ib) {
  return ia != NO_CELL && (ib == NO_CELL || va < vb || (va == vb && ia < ib));
}
__device__ __forceinline__ bool better_max(double va, long ia, double vb, long ib) {
  return ia != NO_CELL && (ib == NO_CELL || va > vb || (va == vb && ia < ib));
}

__global__ __launch_bounds__(256) void audit_cells_kernel(const double* __restrict__ D_scr,
                                                          const uint8_t* __restrict__ st_scr,
                                                          const double* __restrict__ D64,
                                                          const uint8_t* __restrict__ st64,
                                                          const double* __restrict__ rel64, int nw, long cells,
                                                          uint64_t* __restrict__ masks, int* __restrict__ block_counts,
                                                          audit_partial* __restrict__ partials) {
  __shared__ int wave_n[4][N_COUNTS];
  __shared__ double wave_margin[4], wave_err[4];
  __shared__ long wave_margin_cell[4], wave_err_cell[4];
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool in = c < cells;
  audit_point p{0.0, 0.0, ES_PT_NONFINITE, ES_PT_NONFINITE};     // a point past the end: not OK, vouched, no status kind
  if (in) p = audit_load(D_scr, st_scr, D64, st64, c);
  // neighbour in omega: lane + 1 of the same wave, or the halo element for lane 63
  const double dm0 = p.d_merged();
  const int ok0 = (p.s_merged() == ES_PT_OK ? 1 : 0) | (p.s64 == ES_PT_OK ? 2 : 0);
  double dm1 = __shfl_down(dm0, 1);
  double d641 = __shfl_down(p.d64, 1);
  int ok1 = __shfl_down(ok0, 1);
  if (lane == 63) {
    dm1 = 0.0; d641 = 0.0; ok1 = 0;
    if (c + 1 < cells) {
      const audit_point q = audit_load(D_scr, st_scr, D64, st64, c + 1);
      dm1 = q.d_merged(); d641 = q.d64;
      ok1 = (q.s_merged() == ES_PT_OK ? 1 : 0) | (q.s64 == ES_PT_OK ? 2 : 0);
    }
  }
  int kind = 0;
  bool b64 = false;
  if (in) {
    const long row = c / nw;
    const int j = (int)(c - row * nw);
    kind = audit_kind(p, j < nw - 1, dm1, (ok1 & 1) != 0, d641, (ok1 & 2) != 0, &b64);
  }
  const uint64_t m = __ballot(kind != 0);
  const uint64_t m_missed = __ballot((kind & ES_AUDIT_MISSED) != 0), m_false = __ballot((kind & ES_AUDIT_FALSE) != 0);
  const uint64_t m_status = __ballot((kind & ES_AUDIT_STATUS) != 0), m_sign = __ballot((kind & ES_AUDIT_SIGN) != 0);
  const uint64_t m_vok = __ballot(in && p.vouched_ok()), m_unsure = __ballot(in && p.unsure());
  const uint64_t m_b64 = __ballot(b64);

  // compared points: vouched, both statuses OK, the two values differ and neither is NaN
  const bool compared = in && p.vouched_ok() && p.d_scr != p.d64 && !isnan(p.d_scr) && !isnan(p.d64);
  const double diff = fabs(p.d_scr - p.d64);
  double margin = fabs(p.d64) / diff;
  int margin_lane = (compared && !isnan(margin)) ? lane : 64;
  double err = 0.0;
  int err_lane = 64;
  if (compared && rel64 != nullptr && p.d64 != 0.0) {
    const double rel = rel64[c];
    if (isfinite(rel) && rel > 0.0) {
      err = diff / (fabs(p.d64) * 100.0 / rel);
      if (!isnan(err)) err_lane = lane;
    }
  }
  // wave reduction to lane 0; after the first step a lane holds candidates from lanes above its partner's, so ties are
  // decided by the lane they came from
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double om = __shfl_down(margin, off), oe = __shfl_down(err, off);
    const int oml = __shfl_down(margin_lane, off), oel = __shfl_down(err_lane, off);
    if (oml < 64 && (margin_lane == 64 || om < margin || (om == margin && oml < margin_lane))) {
      margin = om; margin_lane = oml;
    }
    if (oel < 64 && (err_lane == 64 || oe > err || (oe == err && oel < err_lane))) { err = oe; err_lane = oel; }
  }
  if (lane == 0) {
    masks[c >> 6] = m;
    int* n = wave_n[wid];
    n[N_FLAGGED] = __popcll(m);
    n[N_MISSED] = __popcll(m_missed);  n[N_FALSE] = __popcll(m_false);
    n[N_STATUS] = __popcll(m_status);  n[N_SIGN] = __popcll(m_sign);
    n[N_VOUCHED_OK] = __popcll(m_vok); n[N_UNSURE] = __popcll(m_unsure);
    n[N_BRACKETS64] = __popcll(m_b64);
    wave_margin[wid] = margin; wave_margin_cell[wid] = margin_lane < 64 ? c + margin_lane : NO_CELL;
    wave_err[wid] = err;       wave_err_cell[wid] = err_lane < 64 ? c + err_lane : NO_CELL;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    audit_partial out;
    for (int q = 0; q < N_COUNTS; ++q) out.n[q] = wave_n[0][q] + wave_n[1][q] + wave_n[2][q] + wave_n[3][q];
    out.margin = wave_margin[0]; out.margin_cell = wave_margin_cell[0];
    out.err = wave_err[0];       out.err_cell = wave_err_cell[0];
    for (int w = 1; w < 4; ++w) {
      if (better_min(wave_margin[w], wave_margin_cell[w], out.margin, out.margin_cell)) {
        out.margin = wave_margin[w]; out.margin_cell = wave_margin_cell[w];
      }
      if (better_max(wave_err[w], wave_err_cell[w], out.err, out.err_cell)) {
        out.err = wave_err[w]; out.err_cell = wave_err_cell[w];
      }
    }
    block_counts[blockIdx.x] = out.n[N_FLAGGED];
    partials[blockIdx.x] = out;
  }
}

// One workgroup: partials -> d_counts[10], d_worst[2].  nblocks == 0 writes the result of the empty grid.
__global__ __launch_bounds__(1024) void audit_reduce_kernel(const audit_partial* __restrict__ partials, int nblocks,
                                                            int64_t* __restrict__ d_counts,
                                                            double* __restrict__ d_worst) {
  __shared__ long long wave_n[16][N_COUNTS];
  __shared__ double wave_margin[16], wave_err[16];
  __shared__ long wave_margin_cell[16], wave_err_cell[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  long long n[N_COUNTS];
  for (int q = 0; q < N_COUNTS; ++q) n[q] = 0;
  double margin = INFINITY, err = 0.0;
  long margin_cell = NO_CELL, err_cell = NO_CELL;
  for (int i = tid; i < nblocks; i += 1024) {
    const audit_partial p = partials[i];
    for (int q = 0; q < N_COUNTS; ++q) n[q] += p.n[q];
    if (better_min(p.margin, p.margin_cell, margin, margin_cell)) { margin = p.margin; margin_cell = p.margin_cell; }
    if (better_max(p.err, p.err_cell, err, err_cell)) { err = p.err; err_cell = p.err_cell; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    for (int q = 0; q < N_COUNTS; ++q) n[q] += __shfl_down(n[q], off);
    const double om = __shfl_down(margin, off), oe = __shfl_down(err, off);
    const long omc = __shfl_down(margin_cell, off), oec = __shfl_down(err_cell, off);
    if (better_min(om, omc, margin, margin_cell)) { margin = om; margin_cell = omc; }
    if (better_max(oe, oec, err, err_cell)) { err = oe; err_cell = oec; }
  }
  if (lane == 0) {
    for (int q = 0; q < N_COUNTS; ++q) wave_n[wid][q] = n[q];
    wave_margin[wid] = margin; wave_margin_cell[wid] = margin_cell;
    wave_err[wid] = err;       wave_err_cell[wid] = err_cell;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) {
      for (int q = 0; q < N_COUNTS; ++q) n[q] += wave_n[w][q];
      if (better_min(wave_margin[w], wave_margin_cell[w], margin, margin_cell)) {
        margin = wave_margin[w]; margin_cell = wave_margin_cell[w];
      }
      if (better_max(wave_err[w], wave_err_cell[w], err, err_cell)) { err = wave_err[w]; err_cell = wave_err_cell[w]; }
    }
    for (int q = 0; q < N_COUNTS; ++q) d_counts[q] = n[q];
    d_counts[8] = margin_cell == NO_CELL ? -1 : margin_cell;
    d_counts[9] = err_cell == NO_CELL ? -1 : err_cell;
    d_worst[0] = margin_cell == NO_CELL ? INFINITY : margin;
    d_worst[1] = err_cell == NO_CELL ? 0.0 : err;
  }
}

__global__ __launch_bounds__(256) void audit_emit_kernel(const double* __restrict__ D_scr,
                                                         const uint8_t* __restrict__ st_scr,
                                                         const double* __restrict__ D64,
                                                         const uint8_t* __restrict__ st64, int nw, long cells,
                                                         const uint64_t* __restrict__ masks,
                                                         const int* __restrict__ block_off, int capacity,
                                                         int64_t* __restrict__ d_cell, uint8_t* __restrict__ d_kind) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int pos = es_flagged_pos(masks, block_off, c, cells, capacity);
  if (pos < 0) return;
  const audit_point p = audit_load(D_scr, st_scr, D64, st64, c);
  const long row = c / nw;
  const bool inner = (int)(c - row * nw) < nw - 1;               // then c + 1 is a cell of the same row
  double dm1 = 0.0, d641 = 0.0;
  bool okm1 = false, ok641 = false, b64;
  if (inner) {
    const audit_point q = audit_load(D_scr, st_scr, D64, st64, c + 1);
    dm1 = q.d_merged(); d641 = q.d64;
    okm1 = q.s_merged() == ES_PT_OK; ok641 = q.s64 == ES_PT_OK;
  }
  d_cell[pos] = c;
  d_kind[pos] = (uint8_t)audit_kind(p, inner, dm1, okm1, d641, ok641, &b64);
}

}  // namespace

extern "C" int es_shoot_audit_screening(es_context* ctx, int nk, int nw, const double* d_D_scr,
                                        const uint8_t* d_status_scr, const double* d_D64, const uint8_t* d_status64,
                                        const double* d_rel64, int capacity, int64_t* d_cell, uint8_t* d_kind,
                                        int64_t* d_counts, double* d_worst) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, nk >= 0 && nw >= 0 && capacity >= 0, "negative size");
  const long cells = (long)nk * nw;
  ES_REQUIRE(ctx, cells <= 0x7fffffffL, "nk * nw must be below 2^31");
  ES_REQUIRE(ctx, d_counts && d_worst, "null pointer");
  ES_REQUIRE(ctx, cells == 0 || (d_D_scr && d_status_scr && d_D64 && d_status64), "null pointer");
  ES_REQUIRE(ctx, capacity == 0 || (d_cell && d_kind), "null table with capacity > 0");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int nblocks = (int)((cells + 255) / 256);
  audit_partial* partials = nullptr;
  if (cells > 0) {
    int rc = es_ensure_scan_scratch(ctx, (size_t)cells);
    if (rc != ES_SUCCESS) return rc;
    rc = es_ensure_scratch(ctx, (size_t)nblocks * sizeof(audit_partial));
    if (rc != ES_SUCCESS) return rc;
    partials = (audit_partial*)ctx->d_scratch;
    hipLaunchKernelGGL(audit_cells_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, d_D_scr, d_status_scr, d_D64,
                       d_status64, d_rel64, nw, cells, ctx->d_masks, ctx->d_block_counts, partials);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(audit_reduce_kernel, dim3(1), dim3(1024), 0, ctx->stream, partials, nblocks, d_counts, d_worst);
  ES_HIP_CHECK(ctx, hipGetLastError());
  if (cells > 0 && capacity > 0) {
    int rc = es_scan_block_counts_async(ctx, nblocks);
    if (rc != ES_SUCCESS) return rc;
    hipLaunchKernelGGL(audit_emit_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, d_D_scr, d_status_scr, d_D64,
                       d_status64, nw, cells, ctx->d_masks, ctx->d_block_counts, capacity, d_cell, d_kind);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  return ES_SUCCESS;
}
