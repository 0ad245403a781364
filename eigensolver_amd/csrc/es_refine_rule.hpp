// The ES_REFINE_SECTION rule, ONE text: refine_kernel, refine_polish_kernel (es_refine.hip) and cyl_uniform_refine_kernel
// (es_cyl_uniform.hip) are written on it, so a search refined through the shooting path on one rank and through the closed
// form on another is refined by one rule.  Needs nothing but HIP and ES_PT_OK.  (bench.py, the NumPy models under tests/
// and oracle/c/shoot_port.c restate it on purpose.)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/eigensolver_amd.h"

// a bracket and D at its ends; passed and returned by value: the four doubles stay in registers
struct es_bracket { double lo, hi, flo, fhi; };

// (LANES+1)-section: lane j of a bracket evaluates the interior point lo + (hi-lo)*(j+1)/(LANES+1); frac = 0.5: the mid-point
template <int LANES>
__device__ __forceinline__ double es_section_frac(int j) { return (double)(j + 1) / (double)(LANES + 1); }
__device__ __forceinline__ double es_section_point(es_bracket b, double frac) { return b.lo + (b.hi - b.lo) * frac; }

// One section round of group g of a wave (its lanes g * LANES ..; called by all lanes of the wave), x = the lane's point and D
// its value: a ballot collects "sign differs from D(lo)", the first set bit picks the sub-interval next to lo.
template <int LANES>
__device__ __forceinline__ es_bracket es_section_update(es_bracket b, double x, double D, int g) {
  const bool diff = (D * b.flo < 0.0);               // NaN products compare false, as in the reference
  const unsigned long long bal = __ballot(diff);
  const unsigned long long bits = (LANES == 64) ? bal : ((bal >> (LANES * g)) & ((1ull << (LANES & 63)) - 1ull));
  const int first = bits ? (__ffsll((long long)bits) - 1) : LANES;       // first point whose sign differs from D(lo)
  const int src_hi = g * LANES + (first < LANES ? first : LANES - 1);
  const int src_lo = g * LANES + (first > 0 ? first - 1 : 0);
  const double x_hi = __shfl(x, src_hi), d_hi_new = __shfl(D, src_hi);
  const double x_lo = __shfl(x, src_lo), d_lo_new = __shfl(D, src_lo);
  if (first < LANES) { b.hi = x_hi; b.fhi = d_hi_new; }
  if (first > 0) { b.lo = x_lo; b.flo = (d_lo_new == d_lo_new) ? d_lo_new : b.flo; }
  return b;
}

// Newton-type polish in fp64: regula-falsi (secant through the bracket ends).
// A secant point that rounding puts ON or just outside an end means that end is the root to the last bit (|f|
// there is rounding noise): stay at the end with the smaller |f| -- bisecting at that stage would throw the
// root half a bracket away.  Only a NaN estimate falls back to the mid-point.
__device__ __forceinline__ double es_secant_point(es_bracket b) {
  double x = b.lo - b.flo * (b.hi - b.lo) / (b.fhi - b.flo);
  if (!(x > b.lo && x < b.hi)) x = (x == x) ? ((fabs(b.flo) <= fabs(b.fhi)) ? b.lo : b.hi) : b.lo + (b.hi - b.lo) * 0.5;
  return x;
}
__device__ __forceinline__ es_bracket es_secant_update(es_bracket b, double x, double D) {
  if (D * b.flo < 0.0) { b.hi = x; b.fhi = D; } else if (D == D) { b.lo = x; b.flo = D; }
  return b;
}
// the flag byte of a root: status and the reference's acceptance measure at the last evaluation
__device__ __forceinline__ uint8_t es_accept_flag(uint8_t st, double rel, double tol) { return (st == ES_PT_OK && rel < tol) ? 1 : 0; }

// `sections`-section rounds equivalent to n_bisect halvings: sections^R >= 2^n_bisect
__host__ __device__ inline int es_section_rounds(int n_bisect, int sections) {
  int rounds = 0;
  for (double span = 1.0, need = ldexp(1.0, n_bisect < 1000 ? n_bisect : 1000); span < need; span *= (double)sections) ++rounds;
  return rounds;
}
