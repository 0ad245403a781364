// Internal declarations shared by the translation units of libeigensolver_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/eigensolver_amd.h"

struct es_context {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string last_error;
  // scratch for bracket compaction (grown on demand, never shrunk)
  uint64_t* d_masks = nullptr;     size_t masks_cap = 0;      // one ballot mask per 64 cells
  int* d_block_counts = nullptr;   size_t blocks_cap = 0;     // per-256-cell block counts / exclusive offsets
  int* d_total = nullptr;                                     // device-side total count
  int* h_total = nullptr;                                     // pinned host mirror
  // the four count words of es_shoot_find_roots_screened (the async searches use the caller's) and their pinned mirror
  int32_t* d_screen = nullptr;
  int32_t* h_screen = nullptr;
  // general call scratch (worker tables and frame stacks, refinement start data): grown on demand, never shrunk;
  // calls on one context are serialised by its stream, so one buffer suffices
  void* d_scratch = nullptr;       size_t scratch_cap = 0;
  // live-column list of es_shoot_eval_grid_ex(ES_EVAL_SKIP_CONTINUUM): [0] = count, [1..] = column indices; per-column
  // dead flags behind it
  int* d_cols = nullptr;           size_t cols_cap = 0;
  uint8_t* d_coldead = nullptr;
  // es_context_grid_timer: event pairs around the launches of the dominant (grid march) kernels on this stream
  bool timer_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> timer_events;
  // es_context_set_refine_rule: ES_REFINE_SECTION / ES_REFINE_HYBRID, read by every root search at its refinement step
  int refine_rule = ES_REFINE_SECTION;
  // ES_REFINE_HYBRID: state of the one-lane phase, fallback root table, its index list, scan words and the fallback count,
  // all sized by the table capacity of the call (grown on demand, never shrunk; its own buffer because the screened
  // searches still hold pointers into d_scratch when they reach the refinement)
  void* d_hybrid = nullptr;        size_t hybrid_cap = 0;
  unsigned long long* d_refine_stats = nullptr;               // es_context_refine_stats: four device words
};

// Bracket a launch of a grid-march kernel with HIP events on the context's stream (no-ops unless the timer is on).
void es_timer_begin(es_context* ctx);
void es_timer_end(es_context* ctx);

#define ES_HIP_CHECK(ctx, expr)                                                                 \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                    \
      return ES_ERR_HIP;                                                                        \
    }                                                                                           \
  } while (0)

#define ES_REQUIRE(ctx, cond, msg)                                                              \
  do {                                                                                          \
    if (!(cond)) {                                                                              \
      if (ctx) (ctx)->last_error = std::string("invalid argument: ") + (msg);                   \
      return ES_ERR_INVALID_ARG;                                                                \
    }                                                                                           \
  } while (0)

// Grow ctx->d_scratch to at least `bytes` (synchronises the stream before freeing the old buffer).
int es_ensure_scratch(es_context* ctx, size_t bytes);

// Grow ctx->d_hybrid to at least `bytes`, as es_ensure_scratch grows d_scratch.
int es_ensure_hybrid_scratch(es_context* ctx, size_t bytes);

// Exclusive scan of `nblocks` per-block counts in place, total to *d_total_out; enqueued.
int es_scan_counts_async(es_context* ctx, int* d_counts, int nblocks, int* d_total_out);

// Grow the compaction scratch so that `cells` cells fit.
int es_ensure_scan_scratch(es_context* ctx, size_t cells);

// Ordered compaction of flagged cells (flags live as 64-bit wave ballots in ctx->d_masks):
//   step 1 (done by the caller's flag kernel): masks[c/64], block_counts[c/256]
//   step 2: exclusive scan of block_counts -> offsets, total
// Returns the total through ctx->h_total after a stream sync.
int es_scan_block_counts(es_context* ctx, int nblocks, int* h_total_out);
// The scan alone, enqueued: offsets in ctx->d_block_counts, total in ctx->d_total, nothing read back.
int es_scan_block_counts_async(es_context* ctx, int nblocks);

// The count convention of every kernel that takes (d_n, n_max): the launch is sized for n_max; the count is *d_n, read from
// device memory and capped at n_max, or n_max itself when d_n == nullptr (the host knows the count).
// d_n is a count that a stage of this library wrote: it is never negative, so only the cap is applied.
__device__ __forceinline__ int es_count(const int* d_n, int n_max) {
  return d_n ? (*d_n < n_max ? *d_n : n_max) : n_max;
}

// The same convention for the entry points that take the count word of an _async search straight from the caller (branch
// labels, root slopes): min(max(*d_count, 0), n), so a word the caller never had a search fill in cannot index backwards.
__device__ __forceinline__ int es_count_clamped(const int32_t* d_count, int n) {
  if (!d_count) return n;
  const int c = *d_count;
  return c < n ? (c < 0 ? 0 : c) : n;
}

// Ordered compaction of flagged slots, device side.  The format: bit l of masks[s / 64] is the flag of slot s = 64 (s / 64) + l
// and block_counts[s / 256] counts the flags of a block of 256 slots (after the scan: the flags in front of the block).
// es_flag_block writes it, es_cell_rank and es_flagged_pos read it.

// Producer: called by all 256 threads of a flag workgroup (it has a barrier), thread t with the flag of slot
// `slot` = 256 blockIdx.x + t.  Returns the number of flags of the block to thread 0 (0 to every other thread).
__device__ __forceinline__ int es_flag_block(bool flag, long slot, uint64_t* __restrict__ masks,
                                             int* __restrict__ block_counts) {
  __shared__ int wave_cnt[4];
  const uint64_t m = __ballot(flag);
  if ((threadIdx.x & 63) == 0) {
    masks[slot >> 6] = m;
    wave_cnt[threadIdx.x >> 6] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x != 0) return 0;
  const int total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
  block_counts[blockIdx.x] = total;
  return total;
}

// Position of a flagged cell inside the ordered output, from the masks and the scanned block offsets.
__device__ __forceinline__ int es_cell_rank(const uint64_t* __restrict__ masks, const int* __restrict__ block_off,
                                            long cell) {
  const long blk = cell >> 8;
  const int wave_in_blk = (int)((cell >> 6) & 3);
  const int lane = (int)(cell & 63);
  int pos = block_off[blk];
  const uint64_t* m = masks + (blk << 2);
  for (int w = 0; w < wave_in_blk; ++w) pos += __popcll(m[w]);
  const uint64_t lower = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  pos += __popcll(m[wave_in_blk] & lower);
  return pos;
}

// Consumer guard of an emit / gather kernel: the position of slot `slot` in the ordered output, or -1 for a slot that is
// out of range (>= n_slots), not flagged, or at or beyond the capacity of the output.
__device__ __forceinline__ int es_flagged_pos(const uint64_t* __restrict__ masks, const int* __restrict__ block_off,
                                              long slot, long n_slots, int capacity) {
  if (slot >= n_slots) return -1;
  if (!((masks[slot >> 6] >> (slot & 63)) & 1ull)) return -1;
  const int pos = es_cell_rank(masks, block_off, slot);
  return pos < capacity ? pos : -1;
}
