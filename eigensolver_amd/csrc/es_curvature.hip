// Dispersion curvature (include/eigensolver_amd.h section 21): the determinant D = outer - inner of es_shoot_eval_points with
// its exact first AND second partial derivatives in omega and k, and the wavenumber at which the curvature d2 omega / dk2 of
// a branch changes sign -- an extremum of the group speed.  The evaluation is jet_march_of of es_jet.hpp over the
// second-order jets of es_jet2.hpp: the formula text of es_shoot_device.hpp at one more scalar type.  All four families run
// the six-component jet Jet2<2> directly (no spill, no private segment: tests/test_root_curvature_codeobj.py).
//
// One pair (one bracket) per lane, 64-lane workgroups.  Node base fields come by scalar loads; nothing is staged in LDS and
// there is no barrier, so a lane that has finished simply goes inactive.
#include "es_jet2.hpp"

namespace {
using namespace es_shoot_shared;
using JetC = Jet2<2>;      // (D, D_w, D_k, D_ww, D_wk, D_kk): j.v, j.d[0], j.d[1], h[0], h[1], h[2]

__device__ __forceinline__ void store6(double* __restrict__ out, size_t n, int i, const JetC& a, bool good) {
  if (!out) return;
  out[i] = good ? a.j.v : NAN;
  out[n + i] = good ? a.j.d[0] : NAN;
  out[2 * n + i] = good ? a.j.d[1] : NAN;
#pragma unroll
  for (int p = 0; p < 3; ++p) out[(3 + p) * n + i] = good ? a.h[p] : NAN;
}

template <int FAM>
__global__ __launch_bounds__(64) void root_curvature_kernel(ShootDev P, const double* __restrict__ kv,
                                                            const double* __restrict__ wv, int n,
                                                            const int32_t* __restrict__ d_count, double* __restrict__ outer,
                                                            double* __restrict__ inner, uint8_t* __restrict__ status) {
  const int cnt = es_count_clamped(d_count, n);                // n stays the row length of the [6][n] outputs
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;                                        // no barrier below: lanes past the count leave at once
  // not tracked: ES_PT_CONTINUUM is not looked at (as root_slopes_kernel)
  const JetMatchT<JetC> M = jet_march_of<FAM, JetC, false>(P, kv[i], wv[i]);
  const bool good = M.status == ES_PT_OK && jet_finite(M.outer) && jet_finite(M.inner);
  store6(outer, (size_t)n, i, M.outer, good);
  store6(inner, (size_t)n, i, M.inner, good);
  if (status) status[i] = (uint8_t)M.status;
}

// A point of a branch: omega polished by Newton at fixed k, then one second-order evaluation there.
struct BranchPoint {
  double k, w, cg, q, rel;
  uint8_t st;
  bool ok;                 // the polish met no leaky or singular point
};

// Newton in omega at fixed k from w, at most 8 steps, until |s| <= 1e-14 |omega| (the rule and the failure conditions of
// root_newton_kernel, no step cap); then c_g = -D_k / D_w and q = d2 omega / dk2 = -(D_kk + 2 D_wk c_g + D_ww c_g^2) / D_w
// with the status and residual of finish_point.
template <int FAM> __device__ __forceinline__ BranchPoint branch_point(const ShootDev& P, double k, double w) {
  BranchPoint B;
  B.k = k;
  B.ok = true;
  for (int it = 0; it < 8; ++it) {
    const JetMatch<1> E = jet_march<FAM, 1, false>(P, k, w);
    const double D = E.outer.v - E.inner.v, Dw = E.outer.d[0] - E.inner.d[0];
    if (E.status != ES_PT_OK || !isfinite(D) || !isfinite(Dw) || Dw == 0.0) {
      B.ok = false;
      break;
    }
    const double s = -D / Dw;
    w += s;
    if (fabs(s) <= 1e-14 * fabs(w)) break;                     // relative alone, as root_newton_kernel
  }
  B.w = w;
  JetMatchT<JetC> E;
  bool crossed;
  if (fam_has_bands<FAM>() && P.use_bands) {
    E = jet_march_of<FAM, JetC, false>(P, k, w);
    crossed = band_crossed(P, k, w);
  } else {
    E = jet_march_of<FAM, JetC, true>(P, k, w);
    crossed = E.crossed;
  }
  const JetC Dj = E.outer - E.inner;
  Mismatch M;
  M.outer = E.outer.j.v;
  M.inner = E.inner.j.v;
  M.d = Dj.j.v;
  ExteriorLite X;
  X.status = E.status;
  double D;
  finish_point(P, M, X, crossed, D, B.rel, B.st);
  const bool has_value = B.st == ES_PT_OK || B.st == ES_PT_CONTINUUM;
  B.cg = -Dj.j.d[1] / Dj.j.d[0];
  B.q = -(Dj.h[2] + 2.0 * Dj.h[1] * B.cg + Dj.h[0] * B.cg * B.cg) / Dj.j.d[0];
  if (!has_value) B.cg = B.q = B.rel = NAN;
  return B;
}

__device__ __forceinline__ bool signs_differ(double a, double b) { return (a < 0.0 && b > 0.0) || (a > 0.0 && b < 0.0); }

// Regula falsi with the Illinois modification on q(k) between the two ends of a bracket.  One loop evaluates the low end
// (step 0), the high end (step 1) and then the iterates, so that each march is inlined once.
template <int FAM>
__global__ __launch_bounds__(64) void cg_extremum_kernel(ShootDev P, const double* __restrict__ k_lo,
                                                         const double* __restrict__ w_lo, const double* __restrict__ k_hi,
                                                         const double* __restrict__ w_hi, int n,
                                                         const int32_t* __restrict__ d_count, int max_iter, double tol_percent,
                                                         double* __restrict__ k_out, double* __restrict__ w_out,
                                                         double* __restrict__ cg_out, double* __restrict__ q_out,
                                                         double* __restrict__ resid, int32_t* __restrict__ iters_out,
                                                         int32_t* __restrict__ flag_out, uint8_t* __restrict__ status) {
  const int cnt = es_count_clamped(d_count, n);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  BranchPoint a, b;                  // the ends, a.k < b.k; an iterate replaces one of them
  double fa = 0.0, fb = 0.0;         // the ordinates regula falsi uses: q of the ends, halved by the Illinois rule
  int side = 0, iters = 0;           // which end the last iterate replaced (-1 low, +1 high)
  bool all_ok = true, changed = false;
  bool high = false;                 // the point reported is b (else a)
  double kc = k_lo[i], wc = w_lo[i];
  for (int step = 0;; ++step) {
    const BranchPoint c = branch_point<FAM>(P, kc, wc);
    all_ok = all_ok && c.ok;
    if (step == 0) {
      a = c;
      kc = k_hi[i];
      wc = w_hi[i];
      continue;
    }
    if (step == 1) {
      b = c;
      changed = signs_differ(a.q, b.q);
      // no sign change (or no step allowed): the end with the smaller |q|, a finite one before a non-finite one
      high = !(fabs(a.q) <= fabs(b.q) || !isfinite(b.q));
      fa = a.q;
      fb = b.q;
      if (!changed || max_iter == 0) break;
    } else {
      ++iters;
      high = signs_differ(c.q, fa);                            // the sign of the high end's q: replaces it (a failed iterate
      if (high) {                                              // takes the low end's place and ends the iteration)
        b = c;
        fb = c.q;
        if (side == 1) fa *= 0.5;
        side = 1;
      } else {
        a = c;
        fa = c.q;
        if (side == -1) fb *= 0.5;
        side = -1;
      }
      if (!c.ok || !isfinite(c.q) || c.q == 0.0) break;
      if (b.k - a.k <= 1e-12 * fabs(c.k) || iters >= max_iter) break;
    }
    kc = b.k - fb * (b.k - a.k) / (fb - fa);
    if (!(kc > a.k && kc < b.k)) kc = 0.5 * (a.k + b.k);
    // omega from the second-order Taylor prediction of the nearer end
    const bool low = kc - a.k <= b.k - kc;
    const double dk = kc - (low ? a.k : b.k);
    wc = (low ? a.w : b.w) + (low ? a.cg : b.cg) * dk + 0.5 * (low ? a.q : b.q) * dk * dk;
  }
  const double rel = high ? b.rel : a.rel;
  const uint8_t st = high ? b.st : a.st;
  k_out[i] = high ? b.k : a.k;
  w_out[i] = high ? b.w : a.w;
  cg_out[i] = high ? b.cg : a.cg;
  q_out[i] = high ? b.q : a.q;
  resid[i] = rel;
  iters_out[i] = iters;
  flag_out[i] = (changed && all_ok && st == ES_PT_OK && rel < tol_percent) ? 1 : 0;
  if (status) status[i] = st;
}

template <int FAM>
int launch_curvature(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                     const int32_t* d_count, double* d_outer, double* d_inner, uint8_t* d_status) {
  hipLaunchKernelGGL((root_curvature_kernel<FAM>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, d_k, d_w, n,
                     d_count, d_outer, d_inner, d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

template <int FAM>
int launch_extrema(es_context* ctx, const es_problem* prob, const double* d_k_lo, const double* d_w_lo, const double* d_k_hi,
                   const double* d_w_hi, int n, const int32_t* d_count, int max_iter, double tol_percent, double* d_k,
                   double* d_w, double* d_cg, double* d_q, double* d_resid, int32_t* d_iters, int32_t* d_flag,
                   uint8_t* d_status) {
  hipLaunchKernelGGL((cg_extremum_kernel<FAM>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, d_k_lo, d_w_lo,
                     d_k_hi, d_w_hi, n, d_count, max_iter, tol_percent, d_k, d_w, d_cg, d_q, d_resid, d_iters, d_flag,
                     d_status);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace

extern "C" int es_shoot_root_curvature(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                                       const int32_t* d_count, double* d_outer, double* d_inner, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define ES_CURVATURE(F) launch_curvature<F>(ctx, prob, d_k, d_w, n, d_count, d_outer, d_inner, d_status)
  ES_DISPATCH_FAMILY(prob->dev.family, ES_CURVATURE)
#undef ES_CURVATURE
}

extern "C" int es_shoot_cg_extrema(es_context* ctx, const es_problem* prob, const double* d_k_lo, const double* d_w_lo,
                                   const double* d_k_hi, const double* d_w_hi, int n, const int32_t* d_count, int max_iter,
                                   double tol_percent, double* d_k, double* d_w, double* d_cg, double* d_q, double* d_resid,
                                   int32_t* d_iters, int32_t* d_flag, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, n >= 0, "negative size");
  ES_REQUIRE(ctx, max_iter >= 0, "max_iter");
  ES_REQUIRE(ctx, tol_percent > 0.0, "tol_percent must be positive");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k_lo && d_w_lo && d_k_hi && d_w_hi && d_k && d_w && d_cg && d_q && d_resid && d_iters && d_flag,
             "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define ES_EXTREMA(F) launch_extrema<F>(ctx, prob, d_k_lo, d_w_lo, d_k_hi, d_w_hi, n, d_count, max_iter, tol_percent, d_k, \
                                        d_w, d_cg, d_q, d_resid, d_iters, d_flag, d_status)
  ES_DISPATCH_FAMILY(prob->dev.family, ES_EXTREMA)
#undef ES_EXTREMA
}
