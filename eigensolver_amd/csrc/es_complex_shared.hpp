// Shared by the complex-frequency translation units (es_complex.hip: values, roots, eigenfunctions; es_complex_slopes.hip:
// jets and Newton): the complex scalar `cx` with its operators, the k-dependent constants of a lane and the argument check.
#pragma once
#include "es_shoot_shared.hpp"

namespace es_complex_shared {
using namespace es_shoot_shared;

struct cx {
  double re, im;
};
__device__ __forceinline__ cx mk(double a, double b = 0.0) { return cx{a, b}; }
__device__ __forceinline__ cx operator+(cx a, cx b) { return cx{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cx operator-(cx a, cx b) { return cx{a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cx operator-(cx a) { return cx{-a.re, -a.im}; }
__device__ __forceinline__ cx operator*(cx a, cx b) { return cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cx operator*(double s, cx a) { return cx{s * a.re, s * a.im}; }
__device__ __forceinline__ cx operator/(cx a, cx b) {
  const double n = b.re * b.re + b.im * b.im;
  return cx{(a.re * b.re + a.im * b.im) / n, (a.im * b.re - a.re * b.im) / n};
}
__device__ __forceinline__ cx operator-(double s, cx a) { return cx{s - a.re, -a.im}; }
__device__ __forceinline__ cx operator+(double s, cx a) { return cx{s + a.re, a.im}; }
__device__ __forceinline__ double cabs2(cx a) { return a.re * a.re + a.im * a.im; }
__device__ __forceinline__ double cabs_(cx a) { return hypot(a.re, a.im); }
__device__ __forceinline__ bool cfinite(cx a) { return isfinite(a.re) && isfinite(a.im); }
// principal square root (Re >= 0)
__device__ __forceinline__ cx csqrt_(cx z) {
  const double r = hypot(z.re, z.im);
  if (r == 0.0) return cx{0.0, 0.0};
  double a = sqrt(0.5 * (r + fabs(z.re)));
  double b = 0.5 * z.im / a;
  if (z.re >= 0.0) return cx{a, b};
  return cx{fabs(b), copysign(a, z.im)};
}
__device__ __forceinline__ cx cexp_(cx z) {
  const double e = exp(z.re);
  double s, c;
  sincos(z.im, &s, &c);
  return cx{e * c, e * s};
}

struct CxConsts {
  double k, k2, kc2, kvA2, kcT2, k4c, S_i;
  int variant;
};

__device__ __forceinline__ CxConsts cx_consts(const ShootDev& P, int variant, double k) {
  CxConsts C;
  C.k = k; C.k2 = k * k;
  C.kc2 = C.k2 * P.c2_i; C.kvA2 = C.k2 * P.vA2_i; C.kcT2 = C.k2 * P.cT2_i;
  C.k4c = C.k2 * C.k2 * P.cT2_i * P.c2_i;
  C.S_i = P.S_i; C.variant = variant;
  return C;
}

inline int check_cx(es_context* ctx, const es_problem* prob, int variant) {
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, variant == ES_CX_SFX || variant == ES_CX_SFG, "variant");
  if (prob->dev.family != FAM_SLABF) {
    ctx->last_error = "complex frequencies are implemented for ES_GEOM_SLAB_FLOW problems only";
    return ES_ERR_UNSUPPORTED;
  }
  return ES_SUCCESS;
}

}  // namespace es_complex_shared
