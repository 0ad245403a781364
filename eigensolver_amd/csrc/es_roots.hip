// K4: the root searches on an evaluated (k, omega) grid -- es_shoot_find_roots*, the screened / mixed searches -- and the
// exchange packing of their root tables.  Evaluation and refinement are dispatch_points / dispatch_refine
// (es_shoot_host.hpp); the fp32 march of the mixed searches is the public es_shoot_screen_grid.
//  * bracket_flag_kernel: sign change against the omega-neighbour through __shfl_down (lane 63 reads the halo
//    element), ballot masks + per-block counts; bracket_emit_kernel writes the ordered bracket list.
#include "es_shoot_host.hpp"

namespace {
using namespace es_shoot_shared;

// ---- brackets ------------------------------------------------------------------------------------------------
// cell c = row*nw + j ; bracket if j < nw-1, both ends ES_PT_OK and D[c]*D[c+1] < 0 (sign product as in CF:806).
__global__ __launch_bounds__(256) void bracket_flag_kernel(const double* __restrict__ D,
                                                           const uint8_t* __restrict__ st, int nw, long cells,
                                                           uint64_t* __restrict__ masks,
                                                           int* __restrict__ block_counts) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  double d0 = 0.0; int ok0 = 0;
  if (c < cells) { d0 = D[c]; ok0 = (st[c] == ES_PT_OK); }
  // neighbour in omega: lane+1 of the same wave, or the halo element for lane 63
  double d1 = __shfl_down(d0, 1);
  int ok1 = __shfl_down(ok0, 1);
  if (lane == 63) {
    if (c + 1 < cells) { d1 = D[c + 1]; ok1 = (st[c + 1] == ES_PT_OK); } else { d1 = 0.0; ok1 = 0; }
  }
  bool flag = false;
  if (c < cells) {
    const long row = c / nw;
    const int j = (int)(c - row * nw);
    flag = (j < nw - 1) && ok0 && ok1 && (d0 * d1 < 0.0);
  }
  es_flag_block(flag, c, masks, block_counts);
}

__global__ __launch_bounds__(256) void bracket_emit_kernel(const double* __restrict__ kv,
                                                           const double* __restrict__ wv, int nw, int w_mode,
                                                           long cells, const double* __restrict__ D,
                                                           const uint64_t* __restrict__ masks,
                                                           const int* __restrict__ block_off, es_root_table tab,
                                                           double* __restrict__ d_lo_sign, double* __restrict__ d_hi_sign) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int pos = es_flagged_pos(masks, block_off, c, cells, tab.capacity);
  if (pos < 0) return;
  const long row = c / nw;
  const int j = (int)(c - row * nw);
  const double k = kv[row];
  tab.d_k[pos] = k;
  tab.d_row[pos] = (int32_t)row;
  tab.d_w_lo[pos] = pick_w(wv, w_mode, k, (int)row, nw, j);
  tab.d_w_hi[pos] = pick_w(wv, w_mode, k, (int)row, nw, j + 1);
  d_lo_sign[pos] = D[c];
  d_hi_sign[pos] = D[c + 1];
}

// cells with the UNSURE bit -> ballot masks + block counts (same layout as bracket_flag_kernel)
__global__ __launch_bounds__(256) void unsure_flag_kernel(const uint8_t* __restrict__ st, long cells,
                                                          uint64_t* __restrict__ masks, int* __restrict__ block_counts) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  es_flag_block((c < cells) && (st[c] & F32_UNSURE), c, masks, block_counts);
}

// ordered list of the flagged cells: (k, omega) pairs for the fp64 point kernel and the cell index to scatter back to
__global__ __launch_bounds__(256) void unsure_gather_kernel(const double* __restrict__ kv, const double* __restrict__ wv,
                                                            int nw, int w_mode, long cells,
                                                            const uint64_t* __restrict__ masks,
                                                            const int* __restrict__ block_off, int capacity,
                                                            double* __restrict__ pk, double* __restrict__ pw,
                                                            long* __restrict__ pcell) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int pos = es_flagged_pos(masks, block_off, c, cells, capacity);
  if (pos < 0) return;
  const long row = c / nw;
  const int j = (int)(c - row * nw);
  const double k = kv[row];
  pk[pos] = k;
  pw[pos] = pick_w(wv, w_mode, k, (int)row, nw, j);
  pcell[pos] = c;
}

__global__ __launch_bounds__(256) void scatter_points_kernel(const long* __restrict__ pcell, const double* __restrict__ pD,
                                                             const uint8_t* __restrict__ pst, const int* __restrict__ d_n,
                                                             int n_max, double* __restrict__ D, uint8_t* __restrict__ st) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)es_count(d_n, n_max)) return;
  D[pcell[i]] = pD[i];
  st[pcell[i]] = pst[i];
}

// both ends of the first n brackets as (k, omega) pairs: [0, n) lower ends, [n, 2n) upper ends; the point count 2n goes
// to *d_npts for the fp64 evaluation that follows (d_n and d_npts are words of one array: no __restrict__)
__global__ __launch_bounds__(256) void bracket_end_points_kernel(es_root_table tab, const int* d_n, int n_max, int* d_npts,
                                                                 double* __restrict__ pk, double* __restrict__ pw) {
  const int n = es_count(d_n, n_max);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *d_npts = 2 * n;
  if (i >= n) return;
  pk[i] = tab.d_k[i]; pk[n + i] = tab.d_k[i];
  pw[i] = tab.d_w_lo[i]; pw[n + i] = tab.d_w_hi[i];
}

// fp64 values at the bracket ends replace the screening values the refinement starts from; a bracket whose fp64 ends do
// not change sign (or are not both ES_PT_OK) would be a failure of the screening bound: counted, never hidden
__global__ __launch_bounds__(256) void bracket_end_values_kernel(const double* __restrict__ pD, const uint8_t* __restrict__ pst,
                                                                 const int* d_n, int n_max, double* __restrict__ d_lo,
                                                                 double* __restrict__ d_hi, int* violations) {
  const int n = es_count(d_n, n_max);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double a = pD[i], b = pD[n + i];
  d_lo[i] = a;
  d_hi[i] = b;
  if (!(pst[i] == ES_PT_OK && pst[n + i] == ES_PT_OK && a * b < 0.0)) atomicAdd(violations, 1);
}

// flag + scan + emit + refine, everything enqueued, no host synchronisation: the bracket count stays in ctx->d_total
int find_roots_enqueue(es_context* ctx, const es_problem* prob, const double* d_k, int nk, const double* d_w, int nw,
                       int w_mode, const double* d_D, const uint8_t* d_status, int n_bisect, double tol_percent,
                       const es_root_table* table) {
  const long cells = (long)nk * nw;
  int rc = es_ensure_scan_scratch(ctx, (size_t)cells);
  if (rc) return rc;
  const int nblocks = (int)((cells + 255) / 256);
  hipLaunchKernelGGL(bracket_flag_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, d_D, d_status, nw, cells,
                     ctx->d_masks, ctx->d_block_counts);
  ES_HIP_CHECK(ctx, hipGetLastError());
  rc = es_scan_block_counts_async(ctx, nblocks);
  if (rc) return rc;
  if (table->capacity > 0) {
    hipLaunchKernelGGL(bracket_emit_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, d_k, d_w, nw, w_mode, cells,
                       d_D, ctx->d_masks, ctx->d_block_counts, *table, table->d_w, table->d_resid);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  return ES_SUCCESS;
}

int check_find_roots_args(es_context* ctx, const es_problem* prob, int nk, int nw, int w_mode, int n_bisect,
                          const es_root_table* table) {
  int rc = check_problem(ctx, prob);
  if (rc) return rc;
  rc = check_refine_rule(ctx);
  if (rc) return rc;
  ES_REQUIRE(ctx, table, "null pointer");
  ES_REQUIRE(ctx, nk >= 0 && nw >= 0 && n_bisect >= 0 && table->capacity >= 0, "negative size");
  ES_REQUIRE(ctx, w_mode >= 0 && w_mode <= 2, "w_mode");
  return check_root_table(ctx, table);
}
}  // namespace

extern "C" int es_shoot_find_roots(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                   const double* d_w, int nw, int w_mode, const double* d_D,
                                   const uint8_t* d_status, int n_bisect, double tol_percent, es_root_table* table,
                                   int* h_count) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, h_count, "null pointer");
  int rc = check_find_roots_args(ctx, prob, nk, nw, w_mode, n_bisect, table);
  if (rc) return rc;
  *h_count = 0;
  if ((long)nk * nw == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w && d_D && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  rc = find_roots_enqueue(ctx, prob, d_k, nk, d_w, nw, w_mode, d_D, d_status, n_bisect, tol_percent, table);
  if (rc) return rc;
  // the one read-back of this entry point: the count it returns through a host pointer also sizes the refinement launch
  ES_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_total, ctx->d_total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ES_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const int total = *ctx->h_total;
  *h_count = total;
  const int n = total < table->capacity ? total : table->capacity;
  if (n > 0) {
    rc = dispatch_refine(ctx, prob, *table, nullptr, n, n, n_bisect, tol_percent);
    if (rc) return rc;
  }
  return total > table->capacity ? ES_ERR_CAPACITY : ES_SUCCESS;
}

extern "C" int es_shoot_find_roots_async(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                         const double* d_w, int nw, int w_mode, const double* d_D,
                                         const uint8_t* d_status, int n_bisect, double tol_percent,
                                         es_root_table* table, int32_t* d_count) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, d_count, "null pointer");
  int rc = check_find_roots_args(ctx, prob, nk, nw, w_mode, n_bisect, table);
  if (rc) return rc;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if ((long)nk * nw == 0) {
    ES_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), ctx->stream));
    return ES_SUCCESS;
  }
  ES_REQUIRE(ctx, d_k && d_w && d_D && d_status, "null pointer");
  rc = find_roots_enqueue(ctx, prob, d_k, nk, d_w, nw, w_mode, d_D, d_status, n_bisect, tol_percent, table);
  if (rc) return rc;
  ES_HIP_CHECK(ctx, hipMemcpyAsync(d_count, ctx->d_total, sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
  if (table->capacity > 0) {
    // refinement sized for the table capacity, count taken from the caller's device word (ctx->d_total is reused by the
    // next call on this context); the expected count for the variant choice: half the capacity (callers size the
    // table at about twice the brackets they expect)
    rc = dispatch_refine(ctx, prob, *table, d_count, table->capacity, table->capacity / 2, n_bisect, tol_percent);
    if (rc) return rc;
  }
  return ES_SUCCESS;
}

namespace {
// The argument checks of the screened searches, before anything is enqueued or written, in two halves (the synchronous
// call zeroes its host outputs between them).  `counts`: where the call reports its counts (h_count or d_counts).
int check_screened_args(es_context* ctx, const es_problem* prob, int nk, int nw, int w_mode, int n_bisect,
                        const es_root_table* table, const void* counts) {
  int rc = check_mixed_args(ctx, prob, nk, nw, w_mode);
  if (rc) return rc;
  rc = check_refine_rule(ctx);
  if (rc) return rc;
  ES_REQUIRE(ctx, table && counts, "null pointer");
  ES_REQUIRE(ctx, n_bisect >= 0 && table->capacity >= 0, "negative size");
  ES_REQUIRE(ctx, table->capacity <= (1 << 30), "table capacity above 2^30 (the bracket-end count is an int32)");
  return ES_SUCCESS;
}

int check_screened_arrays(es_context* ctx, long cells, const double* d_k, const double* d_w, const double* d_D,
                          const uint8_t* d_status, const es_root_table* table) {
  if (cells == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w && d_D && d_status, "null pointer");
  return check_root_table(ctx, table);
}

// The mixed search on a screened grid (everything of include/eigensolver_amd.h behind the fp32 march), arguments checked,
// for the synchronous and the asynchronous entry points alike.  c[0 .. 3]: the count words (brackets, unsure points,
// bracket-end points, unconfirmed brackets), device memory in both modes.
//   h == nullptr, device-count mode (the asynchronous searches, c = the caller's d_counts): nothing is read back.  Every
//     stage is launched for the grid or for the table capacity and reads its count from its word; the per-point scratch
//     holds max(cells, 2 capacity) points.
//   h != nullptr, host-count mode (es_shoot_find_roots_screened, c / h = the context's words and their pinned mirror): the
//     total of each scan is read back into h and IS the launch bound of the stages that follow (d_n = nullptr) and the size
//     of their scratch; a stage whose bound is 0 is skipped.  h[3] is read after the refinement is enqueued, with the last
//     synchronisation of the call; h[2] is set on the host.
int screened_search(es_context* ctx, const es_problem* prob, const double* d_k, int nk, const double* d_w, int nw,
                    int w_mode, int n_bisect, double tol_percent, double* d_D, uint8_t* d_status,
                    const es_root_table* table, int32_t* c, int32_t* h) {
  const long cells = (long)nk * nw;
  const int cap = table->capacity;
  if (h) h[0] = h[1] = h[2] = h[3] = 0;
  ES_HIP_CHECK(ctx, hipMemsetAsync(c, 0, 4 * sizeof(int32_t), ctx->stream));
  if (cells == 0) return ES_SUCCESS;
  int rc = es_ensure_scan_scratch(ctx, (size_t)cells);
  if (rc) return rc;
  // per-point scratch, 33 bytes per point; the unsure points and the bracket ends follow each other on the stream and
  // share it
  double *pk = nullptr, *pw = nullptr, *pD = nullptr; long* pcell = nullptr; uint8_t* pst = nullptr;
  auto carve = [&](size_t npts) -> int {
    auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t bd = align(npts * sizeof(double));
    const int r = es_ensure_scratch(ctx, 4 * bd + align(npts));
    if (r) return r;
    char* b = (char*)ctx->d_scratch;
    pk = (double*)b; pw = (double*)(b + bd); pD = (double*)(b + 2 * bd); pcell = (long*)(b + 3 * bd);
    pst = (uint8_t*)(b + 4 * bd);
    return ES_SUCCESS;
  };
  auto read_back = [&](int word) -> int {
    ES_HIP_CHECK(ctx, hipMemcpyAsync(h + word, c + word, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ES_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ES_SUCCESS;
  };
  const dim3 grid_blocks = es_blocks(cells);
  if (!h && (rc = carve((size_t)cells > 2 * (size_t)cap ? (size_t)cells : 2 * (size_t)cap))) return rc;
  // 1. flag the unsure points and scan: count to c[1]
  hipLaunchKernelGGL(unsure_flag_kernel, grid_blocks, dim3(256), 0, ctx->stream, d_status, cells, ctx->d_masks,
                     ctx->d_block_counts);
  ES_HIP_CHECK(ctx, hipGetLastError());
  rc = es_scan_counts_async(ctx, ctx->d_block_counts, (int)grid_blocks.x, c + 1);
  if (rc) return rc;
  long n_pts = cells;                                            // bound of the unsure points
  if (h) {
    if ((rc = read_back(1))) return rc;
    n_pts = h[1];
    if (n_pts > 0 && (rc = carve((size_t)n_pts))) return rc;
  }
  // 2. gather them, re-evaluate in fp64, scatter back
  if (n_pts > 0) {
    hipLaunchKernelGGL(unsure_gather_kernel, grid_blocks, dim3(256), 0, ctx->stream, d_k, d_w, nw, w_mode, cells,
                       ctx->d_masks, ctx->d_block_counts, es_bound(n_pts), pk, pw, pcell);
    ES_HIP_CHECK(ctx, hipGetLastError());
    rc = dispatch_points(ctx, prob, pk, pw, h ? nullptr : c + 1, n_pts, pD, nullptr, pst);
    if (rc) return rc;
    hipLaunchKernelGGL(scatter_points_kernel, es_blocks(n_pts), dim3(256), 0, ctx->stream, pcell, pD, pst,
                       h ? nullptr : c + 1, es_bound(n_pts), d_D, d_status);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  // 3. flag the brackets on the merged array (signs and statuses are now those of the fp64 path) and scan: count to c[0]
  hipLaunchKernelGGL(bracket_flag_kernel, grid_blocks, dim3(256), 0, ctx->stream, d_D, d_status, nw, cells,
                     ctx->d_masks, ctx->d_block_counts);
  ES_HIP_CHECK(ctx, hipGetLastError());
  rc = es_scan_counts_async(ctx, ctx->d_block_counts, (int)grid_blocks.x, c);
  if (rc) return rc;
  int n_br = cap;                                                // bound of the brackets written and refined
  if (h) {
    if ((rc = read_back(0))) return rc;
    if (h[0] < cap) n_br = h[0];
  }
  if (n_br == 0) return ES_SUCCESS;
  const int* d_n = h ? nullptr : c;
  // 4. emit the brackets, then both ends of every bracket in fp64: the refinement starts from the numbers of the fp64 path
  hipLaunchKernelGGL(bracket_emit_kernel, grid_blocks, dim3(256), 0, ctx->stream, d_k, d_w, nw, w_mode, cells,
                     d_D, ctx->d_masks, ctx->d_block_counts, *table, table->d_w, table->d_resid);
  ES_HIP_CHECK(ctx, hipGetLastError());
  if (h && (rc = carve(2 * (size_t)n_br))) return rc;
  hipLaunchKernelGGL(bracket_end_points_kernel, es_blocks(n_br), dim3(256), 0, ctx->stream, *table, d_n, n_br, c + 2, pk, pw);
  ES_HIP_CHECK(ctx, hipGetLastError());
  rc = dispatch_points(ctx, prob, pk, pw, h ? nullptr : c + 2, 2 * (long)n_br, pD, nullptr, pst);
  if (rc) return rc;
  hipLaunchKernelGGL(bracket_end_values_kernel, es_blocks(n_br), dim3(256), 0, ctx->stream, pD, pst, d_n, n_br, table->d_w,
                     table->d_resid, c + 3);
  ES_HIP_CHECK(ctx, hipGetLastError());
  if (h) {
    h[2] = 2 * n_br;
    ES_HIP_CHECK(ctx, hipMemcpyAsync(h + 3, c + 3, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  // 5. refine in fp64; with the count on the device the launches are sized for the capacity and the expected count is
  // half of it, as in es_shoot_find_roots_async
  rc = dispatch_refine(ctx, prob, *table, d_n, n_br, h ? n_br : cap / 2, n_bisect, tol_percent);
  if (rc) return rc;
  if (h) ES_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ES_SUCCESS;
}
}  // namespace

// Steps 2 - 5 of the mixed search on a grid screened by es_shoot_screen_grid.
extern "C" int es_shoot_find_roots_screened(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                            const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent,
                                            double* d_D, uint8_t* d_status, es_root_table* table, int* h_count,
                                            int* h_stats) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_screened_args(ctx, prob, nk, nw, w_mode, n_bisect, table, h_count);
  if (rc) return rc;
  *h_count = 0;
  if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = 0;
  const long cells = (long)nk * nw;
  if (cells == 0) return ES_SUCCESS;
  rc = check_screened_arrays(ctx, cells, d_k, d_w, d_D, d_status, table);
  if (rc) return rc;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int32_t* h = ctx->h_screen;
  rc = screened_search(ctx, prob, d_k, nk, d_w, nw, w_mode, n_bisect, tol_percent, d_D, d_status, table, ctx->d_screen,
                       ctx->h_screen);
  *h_count = h[0];
  if (h_stats) { h_stats[0] = h[1]; h_stats[1] = h[2]; h_stats[2] = h[3]; }
  if (rc) return rc;
  if (h[3] != 0) {
    ctx->last_error = "fp32 screening: a bracket was not confirmed by the fp64 values at its ends";
    return ES_ERR_SCREENING;
  }
  return h[0] > table->capacity ? ES_ERR_CAPACITY : ES_SUCCESS;
}

extern "C" int es_shoot_find_roots_mixed(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                         const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent,
                                         double* d_D, uint8_t* d_status, es_root_table* table, int* h_count,
                                         int* h_stats) {
  int rc = es_shoot_screen_grid(ctx, prob, d_k, nk, d_w, nw, w_mode, d_D, d_status);
  if (rc) return rc;
  return es_shoot_find_roots_screened(ctx, prob, d_k, nk, d_w, nw, w_mode, n_bisect, tol_percent, d_D, d_status, table,
                                      h_count, h_stats);
}

// The same with the counts on the device: every check before anything is enqueued, nothing read back.
extern "C" int es_shoot_find_roots_screened_async(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                                  const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent,
                                                  double* d_D, uint8_t* d_status, es_root_table* table,
                                                  int32_t* d_counts) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_screened_args(ctx, prob, nk, nw, w_mode, n_bisect, table, d_counts);
  if (rc) return rc;
  rc = check_screened_arrays(ctx, (long)nk * nw, d_k, d_w, d_D, d_status, table);
  if (rc) return rc;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return screened_search(ctx, prob, d_k, nk, d_w, nw, w_mode, n_bisect, tol_percent, d_D, d_status, table, d_counts, nullptr);
}

extern "C" int es_shoot_find_roots_mixed_async(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                               const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent,
                                               double* d_D, uint8_t* d_status, es_root_table* table, int32_t* d_counts) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_screened_args(ctx, prob, nk, nw, w_mode, n_bisect, table, d_counts);
  if (rc) return rc;
  rc = check_screened_arrays(ctx, (long)nk * nw, d_k, d_w, d_D, d_status, table);
  if (rc) return rc;
  rc = es_shoot_screen_grid(ctx, prob, d_k, nk, d_w, nw, w_mode, d_D, d_status);
  if (rc) return rc;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return screened_search(ctx, prob, d_k, nk, d_w, nw, w_mode, n_bisect, tol_percent, d_D, d_status, table, d_counts, nullptr);
}

// ---- exchange record packing (multi-GPU root-table gather) ---------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void pack_records_kernel(es_root_table tab, int count_host, const int* __restrict__ d_count,
                                                           double m, const int64_t* __restrict__ rows_global, int cap,
                                                           double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;          // row of the send buffer: 0 = header, 1.. = records
  if (i > cap) return;
  const int count = es_count(d_count, count_host);       // the async call passes INT32_MAX: no cap on the count it reports
  double* o = out + (size_t)i * 6;
  int n = count < cap ? count : cap;                     // records written: the receiver compares the count with it
  if (n > tab.capacity) n = tab.capacity;
  if (n < 0) n = 0;
  if (i == 0) {
    o[0] = (double)count; o[1] = (double)n; o[2] = o[3] = o[4] = o[5] = 0.0;
    return;
  }
  const int r = i - 1;
  if (r < n) {
    const int row = tab.d_row[r];
    o[0] = tab.d_k[r]; o[1] = tab.d_w[r]; o[2] = m; o[3] = tab.d_resid[r]; o[4] = (double)tab.d_flag[r];
    o[5] = rows_global ? (double)rows_global[row] : (double)row;
  } else {
    o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.0;
  }
}
}  // namespace

extern "C" int es_root_table_pack(es_context* ctx, const es_root_table* table, int count, double m,
                                  const int64_t* d_rows_global, int cap, double* d_out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, table && d_out && count >= 0 && cap >= 0, "pack arguments");
  ES_REQUIRE(ctx, cap == 0 || count == 0 || (table->d_k && table->d_w && table->d_resid && table->d_row && table->d_flag),
             "null root table arrays");
  ES_REQUIRE(ctx, (count < cap ? count : cap) <= table->capacity, "count exceeds the table");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(pack_records_kernel, dim3((cap + 1 + 255) / 256), dim3(256), 0, ctx->stream, *table, count, nullptr, m,
                     d_rows_global, cap, d_out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_root_table_pack_async(es_context* ctx, const es_root_table* table, const int32_t* d_count, double m,
                                        const int64_t* d_rows_global, int cap, double* d_out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, table && d_out && d_count && cap >= 0, "pack arguments");
  ES_REQUIRE(ctx, cap == 0 || (table->d_k && table->d_w && table->d_resid && table->d_row && table->d_flag),
             "null root table arrays");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(pack_records_kernel, dim3((cap + 1 + 255) / 256), dim3(256), 0, ctx->stream, *table, INT32_MAX, d_count, m,
                     d_rows_global, cap, d_out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
