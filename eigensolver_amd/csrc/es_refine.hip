// K5: refinement of the brackets of a root table (dispatch_refine, es_shoot_host.hpp); the rule itself: es_refine_rule.hpp.
//  * refine_kernel<FAM, LANES, CHR, SECTIONS_ONLY, ONE>: LANES = 16 lanes per bracket, 17-section rounds steered by a wave
//    ballot (uniform trip count -> no divergence); refine_polish_kernel: two secant steps with one lane per bracket and
//    the final classification with the reference's acceptance measure.  Both cylinder families launch one round / one step
//    per launch (ONE); the bracket count may stay on the device (es_shoot_find_roots_async).
//  * ES_REFINE_HYBRID: refine_superlinear_kernel and the hybrid_* kernels of its fallback.
#include <cstdlib>
#include <cmath>

#include "es_shoot_host.hpp"
#include "es_refine_rule.hpp"

namespace {
using namespace es_shoot_shared;

// Bracket refinement by (LANES+1)-section: LANES lanes share one bracket (64/LANES brackets per wave).  Per round the
// lanes evaluate D at the LANES interior points lo + (hi-lo)*(j+1)/(LANES+1); a ballot collects "sign differs from
// D(lo)" and the first set bit picks the sub-interval that keeps the sign change next to lo (the one a scan from lo
// would find, as the reference's left-to-right 3-point refinement does).  n_rounds = ceil(n_bisect ln2 / ln(LANES+1))
// rounds shrink the bracket at least as much as n_bisect bisections would; uniform trip count, no divergence.
// The kernel is bound by the number of SEQUENTIAL marches of one point per lane, not by throughput, as long as the
// launch stays below a few waves per SIMD: LANES = 16 (17-section, 4 rounds for n_bisect = 16) up to 32768 brackets,
// The section rule is FIXED (17-section, 16 lanes per bracket: 4 rounds for n_bisect = 16): it must not depend on the bracket
// count of the call, or a grid tiled over N ranks -- fewer brackets per call -- would be refined by another rule than
// the same grid on one rank and the merged root table would no longer be the N = 1 table bit for bit (round 2 switched
// to 9-section above 32768 brackets per call; the device-side count of es_shoot_find_roots_async could not even know).
// ES_REFINE_SECTIONS = 5 / 9 / 17 in the environment selects another rule for the whole process (tuning aid, honoured by
// the port); the port mirrors the default.
constexpr int kRefineSections = 17;
constexpr int kSharedMin = 0;      // brackets from which the wave-shared node entries are used (untwisted cylinder): always

// Workgroups of 4 waves share ONE LDS staging of the (k-independent) base table: 3.6 KB of LDS per wave instead of 14.4,
// so occupancy is no longer LDS-bound and the compiler aims for the register footprint of the point kernel -- which is
// what lets refinement waves fit beside the grid kernel's when consecutive steps are pipelined over two streams.
constexpr int REFINE_WAVES = 4;

// WPE = 3 (<= 168 VGPRs: 165 for the untwisted cylinder, no spill; two grid waves of 168 and one refinement wave share a
// SIMD's 512 registers) except for the twisted family, which needs 234 and would spill (WPE = 2).
// CHR > 0: the node entries of a bracket are formed once per chunk of CHR steps by the wave into its own LDS table and
// shared by the LANES lanes of the bracket (shoot_point_wavegroup); CHR = 0: every lane forms its own (shoot_point).
// SECTIONS_ONLY (n_polish < 0, what launch_refine uses whenever there is a section round): no status is needed from the
// evaluations (shoot_point<FAM, false>).
template <int FAM, int LANES, int CHR = 0, bool SECTIONS_ONLY = false, bool ONE = false,
          int WPE = ((FAM == FAM_CYLT || !ONE) ? 2 : 3)>
__global__ __launch_bounds__(64 * REFINE_WAVES) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void refine_kernel(ShootDev P, es_root_table tab, double* d_lo, double* d_hi, const int* __restrict__ d_n, int n_max,
                   int n_rounds, int n_polish, double tol_percent) {                      // d_lo / d_hi alias table columns
  // bracket count: from device memory (es_shoot_find_roots_async: the host never reads it; the launch is sized for
  // n_max = the table capacity and the workgroups beyond the count return at once) or n_max itself
  const int n = es_count(d_n, n_max);
  if ((int)(blockIdx.x * REFINE_WAVES * (64 / LANES)) >= n) return;                       // workgroup-uniform
  constexpr int GROUPS = 64 / LANES;
  constexpr int WTBL = GROUPS * (2 * (CHR > 0 ? CHR : 1) + 1) * FamTraits<FAM>::NE;      // doubles per wave
  __shared__ double es_point_lds[CHR > 0 ? REFINE_WAVES * WTBL : FamTraits<FAM>::NB * (2 * es_shoot_shared::CH + 1)];
  const int lane = threadIdx.x & 63;
  const int g = lane / LANES, j = lane % LANES;
  const int i = (blockIdx.x * REFINE_WAVES + ((int)threadIdx.x >> 6)) * GROUPS + g;
  const bool in = i < n;
  const double k = in ? tab.d_k[i] : 1.0;
  es_bracket b = {in ? tab.d_w_lo[i] : 1.0, in ? tab.d_w_hi[i] : 2.0, in ? d_lo[i] : 1.0, in ? d_hi[i] : -1.0};
  const double frac = es_section_frac<LANES>(j);
  double D = 0.0, rel = 0.0; uint8_t st = 0;
  double root = b.lo;
  // ONE evaluation site for the section rounds and the polish steps (the determinant evaluation is inlined: a single
  // copy keeps the kernel at the register footprint of the point kernel plus the bracket state, so that refinement
  // waves fit beside the grid kernel's when consecutive steps are pipelined over two streams)
  const int n_final = (n_polish > 0) ? n_polish : (n_polish == 0 ? 1 : 0);
  // ONE: a single section round per launch (the host launches the kernel n_rounds times; lo / hi / D(lo) / D(hi) travel
  // through the table columns, the same doubles).  A loop over rounds around the inlined determinant evaluation lets the
  // compiler hoist every round-invariant value of that code -- 64-bit literals of the Bessel polynomials, kernel
  // arguments -- out of it and carry them through the march (see es_tile_index).
  const int n_it = ONE ? 1 : n_rounds + n_final;
  for (int it = 0; it < n_it; ++it) {
    const bool section = ONE ? true : it < n_rounds;
    double x;
    if (section) x = es_section_point(b, frac);
    else if (n_polish > 0) x = es_secant_point(b);                     // every lane of the group the same
    else x = es_section_point(b, 0.5);                                 // n_polish = 0: report the bracket mid-point
    if (CHR > 0) shoot_point_wavegroup<FAM, (CHR > 0 ? CHR : 1), GROUPS>(P, k, x, D, rel, st, es_point_lds + ((int)threadIdx.x >> 6) * WTBL);
    else if (SECTIONS_ONLY) shoot_point<FAM, false>(P, k, x, x, D, rel, st, es_point_lds);
    else shoot_point<FAM>(P, k, x, x, D, rel, st, es_point_lds);
    if (section) {
      b = es_section_update<LANES>(b, x, D, g);
    } else {
      root = x;
      if (n_polish > 0) b = es_secant_update(b, x, D);
    }
  }
  if (in && j == 0) {
    tab.d_w_lo[i] = b.lo;
    tab.d_w_hi[i] = b.hi;
    if (n_polish < 0) {                                // section rounds only: D at the ends goes on to refine_polish_kernel
      d_lo[i] = b.flo;
      d_hi[i] = b.fhi;
    } else {
      tab.d_w[i] = root;
      tab.d_resid[i] = rel;
      tab.d_flag[i] = es_accept_flag(st, rel, tol_percent);
    }
  }
}

// The polish steps of refine_kernel with ONE lane per bracket (same arithmetic, bit for bit): in refine_kernel all LANES
// lanes of a bracket evaluate the same secant point, so two of its six marches do a sixteenth of the work they cost.
// ONE: a single polish step per launch (see refine_kernel), `n_polish` = 1 on the last of them, 0 before: the bracket and D
// at its ends go back to the columns they came from until the last step writes root, residual and flag.
template <int FAM, bool ONE = false, int WPE = ((FAM == FAM_CYLT || !ONE) ? 2 : 3)>
__global__ __launch_bounds__(64 * REFINE_WAVES) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void refine_polish_kernel(ShootDev P, es_root_table tab, double* d_lo, double* d_hi, const int* __restrict__ d_n,
                          int n_max, int n_polish, double tol_percent) {   // d_lo / d_hi alias table columns (no restrict)
  ES_POINT_LDS(FAM);
  const int n = es_count(d_n, n_max);
  if ((int)(blockIdx.x * (64 * REFINE_WAVES)) >= n) return;                               // workgroup-uniform
  const int i = blockIdx.x * (64 * REFINE_WAVES) + (int)threadIdx.x;
  const bool in = i < n;
  const double k = in ? tab.d_k[i] : 1.0;
  es_bracket b = {in ? tab.d_w_lo[i] : 1.0, in ? tab.d_w_hi[i] : 2.0, in ? d_lo[i] : 1.0, in ? d_hi[i] : -1.0};
  double D = 0.0, rel = 0.0; uint8_t st = 0;
  double root = b.lo;
  const int n_it = ONE ? 1 : n_polish;
  for (int it = 0; it < n_it; ++it) {
    const double x = es_secant_point(b);
    shoot_point<FAM>(P, k, x, x, D, rel, st, es_point_lds);
    root = x;
    b = es_secant_update(b, x, D);
  }
  if (in) {
    tab.d_w_lo[i] = b.lo;
    tab.d_w_hi[i] = b.hi;
    if (ONE && n_polish == 0) {                        // not the last step: state for the next launch
      d_lo[i] = b.flo;
      d_hi[i] = b.fhi;
    } else {
      tab.d_w[i] = root;
      tab.d_resid[i] = rel;
      tab.d_flag[i] = es_accept_flag(st, rel, tol_percent);
    }
  }
}

// ---- ES_REFINE_HYBRID (include/eigensolver_amd.h): S section rounds, one lane per bracket, section rule as the fallback --
// All three constants are part of the rule, which is fixed per bracket (see kRefineSections): tests/refine_hybrid_model.py
// restates them.
constexpr int kHybridSections = 1;          // S: 17-section rounds before the one-lane phase (1 or 2)
constexpr int kHybridSteps = 8;             // M: evaluations of the one-lane phase at most
constexpr double kHybridEps = 1e-12;        // relative step / width at which an iterate counts as converged

// State of the one-lane phase between its launches; `info`: bits 0-1 the end the last step retained (1 lower, 2 upper,
// 0 none yet), bits 2-3 HYB_ACTIVE / HYB_KEPT / HYB_FAILED (the fallback takes every bracket that is not HYB_KEPT).
struct HybridState {
  double* lo; double* hi; double* flo; double* fhi; double* xprev;
  int* info;
};
constexpr int HYB_ACTIVE = 0, HYB_KEPT = 1, HYB_FAILED = 2;

// One lane per bracket, modelled on refine_polish_kernel<FAM, true>: one inlined evaluation site, count from device memory,
// launch sized for the capacity, ONE step per launch (`step` = 0 .. kHybridSteps - 1) with the state in S.  A loop over the
// steps inside the kernel was built for every family and dropped: the compiler hoists the step-invariant values of the
// inlined march out of it (see refine_kernel), about 50 more VGPRs for the cylinder families, and every looped form, the
// slabs' included, had a private segment of 36 - 100 bytes per lane; the one-step form has none.  A bracket still
// HYB_ACTIVE after the last step is simply not kept.
// Step 0 reads the state the section rounds left in the table columns (d_lo / d_hi = D at the ends); a table row is written
// ONLY for a bracket the phase keeps: every other row still holds that state when the fallback gathers it.
// "Still iterating" is voted over the WORKGROUP, not the wave (__syncthreads_or): shoot_point stages the base table with all
// threads of the workgroup between barriers, so a wave may not stay out of an evaluation alone; a workgroup whose brackets
// are all finished returns at once.  stats: es_context_refine_stats.
template <int FAM, int WPE = (FAM == FAM_CYL0 ? 3 : 2)>
__global__ __launch_bounds__(64 * REFINE_WAVES) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void refine_superlinear_kernel(ShootDev P, es_root_table tab, const double* d_lo, const double* d_hi, HybridState S,
                               const int* __restrict__ d_n, int n_max, int step, double tol_percent,
                               unsigned long long* stats) {
  ES_POINT_LDS(FAM);
  const int n = es_count(d_n, n_max);
  if ((int)(blockIdx.x * (64 * REFINE_WAVES)) >= n) return;                               // workgroup-uniform
  const int i = blockIdx.x * (64 * REFINE_WAVES) + (int)threadIdx.x;
  const bool in = i < n;
  const bool first = step == 0;
  const int info = (in && !first) ? S.info[i] : 0;
  const bool active = in && ((info >> 2) == HYB_ACTIVE);
  if (!__syncthreads_or(active ? 1 : 0)) return;                                          // workgroup-uniform
  const double k = in ? tab.d_k[i] : 1.0;
  double lo, hi, flo, fhi, xprev;
  if (first) {
    lo = in ? tab.d_w_lo[i] : 1.0;
    hi = in ? tab.d_w_hi[i] : 2.0;
    flo = in ? d_lo[i] : 1.0;
    fhi = in ? d_hi[i] : -1.0;
    xprev = NAN;
  } else {
    lo = active ? S.lo[i] : 1.0;
    hi = active ? S.hi[i] : 2.0;
    flo = active ? S.flo[i] : 1.0;
    fhi = active ? S.fhi[i] : -1.0;
    xprev = active ? S.xprev[i] : NAN;
  }
  int side = info & 3, status = info >> 2;
  double D = 0.0, rel = 0.0; uint8_t st = 0;
  double x = lo - flo * (hi - lo) / (fhi - flo);
  if (!(x > lo && x < hi)) x = lo + (hi - lo) * 0.5;                                      // NaN included
  shoot_point<FAM>(P, k, x, x, D, rel, st, es_point_lds);
  if (active) {
    if (D == D) {
      // Illinois: an end retained twice in a row has its value halved (the sign, which is all the bracket needs, stays)
      if (D * flo < 0.0) { hi = x; fhi = D; if (side == 1) flo *= 0.5; side = 1; }
      else { lo = x; flo = D; if (side == 2) fhi *= 0.5; side = 2; }
      const double ax = fabs(x);
      if (D == 0.0 || fabs(x - xprev) <= kHybridEps * ax || (hi - lo) <= kHybridEps * ax)
        status = (st == ES_PT_OK && rel < tol_percent) ? HYB_KEPT : HYB_FAILED;           // classified at the iterate that met the test
    } else {
      status = HYB_FAILED;
    }
    if (status == HYB_KEPT) {
      tab.d_w_lo[i] = lo;
      tab.d_w_hi[i] = hi;
      tab.d_w[i] = x;
      tab.d_resid[i] = rel;
      tab.d_flag[i] = 1;
    } else if (status == HYB_ACTIVE) {
      S.lo[i] = lo; S.hi[i] = hi; S.flo[i] = flo; S.fhi[i] = fhi; S.xprev[i] = x;
    }
    S.info[i] = side | (status << 2);
  }
  const int n_eval = __popcll(__ballot(active)), n_kept = __popcll(__ballot(active && status == HYB_KEPT));
  if ((threadIdx.x & 63) == 0) {
    if (first && n_eval) atomicAdd(stats + 0, (unsigned long long)n_eval);               // step 0: every bracket is active
    if (n_kept) atomicAdd(stats + 1, (unsigned long long)n_kept);
    if (n_eval) atomicAdd(stats + 3, (unsigned long long)n_eval);
  }
}

// Fallback of the hybrid rule: the brackets the one-lane phase did not keep, in order.  Flags as 64-bit ballots and counts
// per 256 brackets over the whole launch (sized for the capacity: blocks behind the count write zeros, the scan reads them).
__global__ __launch_bounds__(256) void hybrid_flag_kernel(const int* __restrict__ info, const int* __restrict__ d_n,
                                                          int n_max, uint64_t* __restrict__ masks,
                                                          int* __restrict__ block_counts, unsigned long long* stats) {
  const int n = es_count(d_n, n_max);
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const bool flag = i < n && (info[i] >> 2) != HYB_KEPT;
  const int c = es_flag_block(flag, (long)i, masks, block_counts);                        // the block's total, to thread 0
  if (c) atomicAdd(stats + 2, (unsigned long long)c);
}

// row `pos` of the fallback table = bracket idx[pos] with the state the section rounds left in its row
__global__ __launch_bounds__(256) void hybrid_gather_kernel(es_root_table tab, es_root_table ftab, int* __restrict__ idx,
                                                            const uint64_t* __restrict__ masks,
                                                            const int* __restrict__ block_off,
                                                            const int* __restrict__ d_n, int n_max) {
  const int n = es_count(d_n, n_max);
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const int pos = es_flagged_pos(masks, block_off, (long)i, (long)n, ftab.capacity);
  if (pos < 0) return;
  ftab.d_k[pos] = tab.d_k[i];
  ftab.d_w_lo[pos] = tab.d_w_lo[i];
  ftab.d_w_hi[pos] = tab.d_w_hi[i];
  ftab.d_w[pos] = tab.d_w[i];                                                             // D at the lower end
  ftab.d_resid[pos] = tab.d_resid[i];                                                     // D at the upper end
  ftab.d_row[pos] = tab.d_row[i];
  idx[pos] = i;
}

__global__ __launch_bounds__(256) void hybrid_scatter_kernel(es_root_table ftab, es_root_table tab,
                                                             const int* __restrict__ idx,
                                                             const int* __restrict__ d_nf, int n_max) {
  const int nf = es_count(d_nf, n_max);
  const int j = blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= nf) return;
  const int i = idx[j];
  if (i < 0 || i >= tab.capacity) return;
  tab.d_w[i] = ftab.d_w[j];
  tab.d_w_lo[i] = ftab.d_w_lo[j];
  tab.d_w_hi[i] = ftab.d_w_hi[j];
  tab.d_resid[i] = ftab.d_resid[j];
  tab.d_flag[i] = ftab.d_flag[j];
}

// d_n: bracket count in device memory (nullptr: n_max IS the count); n_max: launch bound (count known on the host, or the
// table capacity); n_hint: what the count is expected to be (selects between variants that give identical results).
// `rounds` section rounds (np < 0: sections only, D at the ends stays in d_lo / d_hi), then, if `polish`, the polish steps:
// the section rule is one call with all its rounds; the hybrid rule splits the same launches in two calls around its
// one-lane phase (the state between two section rounds is the four doubles per bracket in the table either way).
template <int FAM>
int launch_refine_steps(es_context* ctx, const es_problem* prob, const es_root_table& tab, double* d_lo, double* d_hi,
                        const int* d_n, int n_max, int n_hint, int sections, int rounds, int np, bool polish, double tol) {
  // 17-section of the untwisted cylinder with np < 0 (sections only): node entries shared inside the wave, 32 steps per
  // chunk (14.6 KB of LDS per wave).  Bit-identical to the per-lane entries, so the choice could follow the bracket count
  // (ES_REFINE_SHARED_MIN); measured in round 3 with the count on the device (same box, tile of an E-GPU run, ms per
  // step shared / per-lane: E = 1 22.05 / 22.29, E = 2 11.35 / 11.28, E = 4 5.85 / 5.98, E = 8 3.19 / 3.29): no
  // crossover worth a rule, the shared form is the default at every count.  The twisted family (16 entries per node:
  // 17 KB per wave at 16 steps per chunk) lost 7 % on configs[4] in round 2 and, measured again with the cheaper round-3
  // coefficient set (67.5 KB of LDS per workgroup, 181 VGPRs), 11 % (86.2 against 77.4 ms per step): per-lane entries stay.
  constexpr int CHR = (FAM == FAM_CYL0) ? 32 : 0;
  int shared_min = kSharedMin;
  if (const char* ev = getenv("ES_REFINE_SHARED_MIN")) shared_min = atoi(ev);
  const bool shared_entries = CHR > 0 && np < 0 && n_hint >= shared_min && !getenv("ES_REFINE_PRIVATE_ENTRIES");
  auto blocks = [&](int per_wg) { return dim3((n_max + per_wg - 1) / per_wg); };
  // One section round / polish step per launch for the twisted family (refine_kernel: 255 -> 194 registers; configs[4]
  // 74.2 -> 72.6 ms per step on one box).  Measured for the others too, registers 167 -> 102: no gain on configs[2] and [3]
  // (7.58 / 7.58, 20.81 / 20.82 ms), a loss on configs[1] (2.92 -> 3.05 ms: six short launches per search instead of two);
  // a register cap of 168 for the twisted kernels (three waves per SIMD, 14 - 18 spilled values) made no difference
  // (72.4 / 72.6).  ES_REFINE_ROUNDS_IN_KERNEL=1: the single launch (A/B aid).
  constexpr bool ONE_ROUND_FAM = (FAM == FAM_CYLT || FAM == FAM_CYL0);
  const bool one_round = ONE_ROUND_FAM && !getenv("ES_REFINE_ROUNDS_IN_KERNEL");
#define ES_REFINE(LANES_, CHR_, SO_, PER_WG_)                                                                           \
  if (SO_ && one_round) {                                                                                               \
    if constexpr (ONE_ROUND_FAM && SO_) {                                                                               \
      for (int r_ = 0; r_ < rounds; ++r_)                                                                               \
        hipLaunchKernelGGL((refine_kernel<FAM, LANES_, CHR_, true, true>), blocks(PER_WG_), dim3(64 * REFINE_WAVES), 0, \
                           ctx->stream, prob->dev, tab, d_lo, d_hi, d_n, n_max, 1, np, tol);                            \
    }                                                                                                                   \
  } else                                                                                                                \
    hipLaunchKernelGGL((refine_kernel<FAM, LANES_, CHR_, SO_, false>), blocks(PER_WG_), dim3(64 * REFINE_WAVES), 0,     \
                       ctx->stream, prob->dev, tab, d_lo, d_hi, d_n, n_max, rounds, np, tol)
  if (sections == 17 && shared_entries) ES_REFINE(16, CHR, true, 4 * REFINE_WAVES);       // shared entries imply np < 0
  else if (np < 0) {
    if (sections == 17) ES_REFINE(16, 0, true, 4 * REFINE_WAVES);
    else if (sections == 9) ES_REFINE(8, 0, true, 8 * REFINE_WAVES);
    else ES_REFINE(4, 0, true, 16 * REFINE_WAVES);
  } else {
    if (sections == 17) ES_REFINE(16, 0, false, 4 * REFINE_WAVES);
    else if (sections == 9) ES_REFINE(8, 0, false, 8 * REFINE_WAVES);
    else ES_REFINE(4, 0, false, 16 * REFINE_WAVES);
  }
#undef ES_REFINE
  ES_HIP_CHECK(ctx, hipGetLastError());
  if (np < 0 && polish) {
    if (one_round) {
      if constexpr (ONE_ROUND_FAM) {
        for (int p_ = 0; p_ < ES_REFINE_POLISH; ++p_)
          hipLaunchKernelGGL((refine_polish_kernel<FAM, true>), blocks(64 * REFINE_WAVES), dim3(64 * REFINE_WAVES), 0, ctx->stream,
                             prob->dev, tab, d_lo, d_hi, d_n, n_max, p_ == ES_REFINE_POLISH - 1 ? 1 : 0, tol);
      }
    } else
      hipLaunchKernelGGL((refine_polish_kernel<FAM, false>), blocks(64 * REFINE_WAVES), dim3(64 * REFINE_WAVES), 0, ctx->stream,
                         prob->dev, tab, d_lo, d_hi, d_n, n_max, ES_REFINE_POLISH, tol);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  return ES_SUCCESS;
}

// ES_REFINE_SECTIONS in the environment (tuning aid, honoured by the port as well): 5, 9 or 17
int refine_sections() {
  int sections = kRefineSections;
  if (const char* ev = getenv("ES_REFINE_SECTIONS")) {
    const int v = atoi(ev);
    if (v == 5 || v == 9 || v == 17) sections = v;
  }
  return sections;
}

// ES_REFINE_HYBRID with more rounds than kHybridSections (include/eigensolver_amd.h).  Everything is enqueued and sized for
// n_max; the number of fallback brackets never leaves the device.
template <int FAM>
int launch_refine_hybrid(es_context* ctx, const es_problem* prob, const es_root_table& tab, const int* d_n, int n_max,
                         int n_hint, int rounds, double tol) {
  if (n_max <= 0) return ES_SUCCESS;
  // carve the context's hybrid buffer: one-lane state, fallback table, index list, scan words, fallback count
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t cap = (size_t)n_max;
  const size_t bd = align(cap * sizeof(double)), bi = align(cap * sizeof(int)), bf = align(cap);
  const int nblk = (n_max + 255) / 256;
  const size_t bm = align((size_t)nblk * 4 * sizeof(uint64_t)), bc = align((size_t)(nblk + 1) * sizeof(int));
  int rc = es_ensure_hybrid_scratch(ctx, 10 * bd + 3 * bi + bf + bm + bc + 256);
  if (rc) return rc;
  char* b = (char*)ctx->d_hybrid;
  auto take = [&](size_t bytes) { char* p = b; b += bytes; return p; };
  HybridState S;
  S.lo = (double*)take(bd); S.hi = (double*)take(bd); S.flo = (double*)take(bd); S.fhi = (double*)take(bd);
  S.xprev = (double*)take(bd);
  S.info = (int*)take(bi);
  es_root_table ftab;
  ftab.d_k = (double*)take(bd); ftab.d_w = (double*)take(bd); ftab.d_w_lo = (double*)take(bd);
  ftab.d_w_hi = (double*)take(bd); ftab.d_resid = (double*)take(bd);
  ftab.d_row = (int32_t*)take(bi); ftab.d_flag = (uint8_t*)take(bf);
  ftab.capacity = n_max;
  int* idx = (int*)take(bi);
  uint64_t* masks = (uint64_t*)take(bm);
  int* counts = (int*)take(bc);
  int* d_nf = (int*)take(256);
  // 1. S section rounds, the launches of the section rule
  rc = launch_refine_steps<FAM>(ctx, prob, tab, tab.d_w, tab.d_resid, d_n, n_max, n_hint, kRefineSections, kHybridSections,
                                -1, false, tol);
  if (rc) return rc;
  // 2. one lane per bracket, one step per launch
  const dim3 wg(64 * REFINE_WAVES), grid((n_max + 64 * REFINE_WAVES - 1) / (64 * REFINE_WAVES));
  for (int s_ = 0; s_ < kHybridSteps; ++s_)
    hipLaunchKernelGGL((refine_superlinear_kernel<FAM>), grid, wg, 0, ctx->stream, prob->dev, tab, tab.d_w, tab.d_resid, S,
                       d_n, n_max, s_, tol, ctx->d_refine_stats);
  ES_HIP_CHECK(ctx, hipGetLastError());
  // 3. fallback: gather in order, the remaining rounds and the polish steps on the scratch table, scatter back
  hipLaunchKernelGGL(hybrid_flag_kernel, dim3(nblk), dim3(256), 0, ctx->stream, S.info, d_n, n_max, masks, counts,
                     ctx->d_refine_stats);
  ES_HIP_CHECK(ctx, hipGetLastError());
  rc = es_scan_counts_async(ctx, counts, nblk, d_nf);
  if (rc) return rc;
  hipLaunchKernelGGL(hybrid_gather_kernel, dim3(nblk), dim3(256), 0, ctx->stream, tab, ftab, idx, masks, counts, d_n, n_max);
  ES_HIP_CHECK(ctx, hipGetLastError());
  rc = launch_refine_steps<FAM>(ctx, prob, ftab, ftab.d_w, ftab.d_resid, d_nf, n_max, n_hint, kRefineSections,
                                rounds - kHybridSections, -1, true, tol);
  if (rc) return rc;
  hipLaunchKernelGGL(hybrid_scatter_kernel, dim3(nblk), dim3(256), 0, ctx->stream, ftab, tab, idx, d_nf, n_max);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

template <int FAM>
int launch_refine(es_context* ctx, const es_problem* prob, const es_root_table& tab, double* d_lo, double* d_hi,
                  const int* d_n, int n_max, int n_hint, int n_bisect, double tol) {
  const int sections = refine_sections();
  const int rounds = es_section_rounds(n_bisect, sections);
  if (ctx->refine_rule == ES_REFINE_HYBRID) {
    const int rc = check_refine_rule(ctx);
    if (rc) return rc;
    if (rounds > kHybridSections) return launch_refine_hybrid<FAM>(ctx, prob, tab, d_n, n_max, n_hint, rounds, tol);
  }
  // section rounds with LANES lanes per bracket, then the polish steps with one lane per bracket (d_lo / d_hi carry D at
  // the ends of the narrowed bracket from one kernel to the other)
  const int np = (ES_REFINE_POLISH > 0 && rounds > 0) ? -1 : ES_REFINE_POLISH;
  return launch_refine_steps<FAM>(ctx, prob, tab, d_lo, d_hi, d_n, n_max, n_hint, sections, rounds, np, true, tol);
}
}  // namespace

int check_refine_rule(es_context* ctx) {
  if (ctx->refine_rule == ES_REFINE_HYBRID && refine_sections() != kRefineSections) {
    ctx->last_error = "ES_REFINE_HYBRID is defined for 17-section only (ES_REFINE_SECTIONS is set to another rule)";
    return ES_ERR_UNSUPPORTED;
  }
  return ES_SUCCESS;
}

int dispatch_refine(es_context* ctx, const es_problem* prob, const es_root_table& tab, const int* d_n, int n_max, int n_hint,
                    int n_bisect, double tol) {
  // the d_w / d_resid columns double as scratch for D at the two bracket ends until refinement overwrites them
#define CALL_REFINE(F) launch_refine<F>(ctx, prob, tab, tab.d_w, tab.d_resid, d_n, n_max, n_hint, n_bisect, tol)
  ES_DISPATCH_FAMILY(prob->dev.family, CALL_REFINE)
#undef CALL_REFINE
}
