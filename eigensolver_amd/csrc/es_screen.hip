#include <cstdlib>
#include <cmath>

#include "es_shoot_host.hpp"

namespace {
using namespace es_shoot_shared;

// =====================================================================================================================
// shoot_grid_f32_kernel, es_shoot_screen_grid: the fp32 screening march of es_shoot_find_roots_mixed (es_roots.hip).
//
// fp32 screening of the (k, omega) grid (BASELINE.json configs[4]: "fp32 bracket + fp64 refine").
//
// The bracket search only needs the SIGN of D at the grid points and the per-point status.  shoot_grid_f32_kernel
// marches the interior in fp32 (node entries formed in fp64 per row and rounded once into the LDS table; exterior and
// boundary algebra stay fp64) and marks every point at which fp32 cannot vouch for sign or status as UNSURE
// (status bit 0x80):
//   * a watched term of the coefficient set (Om^2 - omega_A^2, Om^2 - omega_c^2; C3 for the twisted family) comes
//     within F32_TAU_NODE (1e-3) of zero relative to the size of its parts at some node (near-singular coefficient: large
//     relative error in fp32, and the sign tracking that decides ES_PT_CONTINUUM is not reliable);
//   * |D| < F32_TAU_D * max(|outer|, |inner|)  (a root is close: the sign is within the fp32 error of the march);
//   * |outer| < F32_TAU_POLE * |inner|          (a pole of D is close: the sign of 1/r2 is within that error);
//   * a non-finite fp32 result.
// es_shoot_find_roots_mixed() re-evaluates the unsure points in fp64 (shoot_points_kernel, the arithmetic of the fp64
// grid kernel bit for bit), detects the brackets on the merged array, re-evaluates BOTH ENDS of every bracket in fp64
// (so the refinement starts from exactly the numbers the fp64 path has) and refines in fp64.
constexpr float F32_TAU_NODE = 1e-3f;
constexpr double F32_TAU_D = 5e-2;
constexpr double F32_TAU_POLE = 5e-2;                  // (F32_UNSURE: es_shoot_host.hpp, the root search reads the bit)

// All fp32 arithmetic of the march is written on PAIRS of points (clang ext-vector float2 -> v_pk_fma_f32 /
// v_pk_mul_f32 / v_pk_add_f32: two points per instruction); node entries are wave-uniform scalars broadcast to both
// halves by the packed instructions' operand selects.
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f v2(float x) { return (v2f){x, x}; }
__device__ __forceinline__ v2f vfma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f vabs(v2f a) { return __builtin_elementwise_abs(a); }
__device__ __forceinline__ v2f vmin(v2f a, v2f b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ v2f vmax(v2f a, v2f b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ v2f vrcp(v2f a) { return (v2f){__builtin_amdgcn_rcpf(a.x), __builtin_amdgcn_rcpf(a.y)}; }

struct CoefF { v2f a11, a12, a21, a22; };
struct CoefPreF { v2f n11, n12, n21, n22, den; };

// What the screening pass knows about the watched terms of the coefficient set:
//   band families (status known exactly from W = omega/k): per point the minimum over the nodes of |t1 t2| = |den| / (rho S)
//     -- how close Om^2 came to omega_A^2 or omega_c^2 (1 instruction per point and node);
//   tracked families: t1 = (omega - e0)^2 - omega_A^2 is negative at node j exactly for omega inside the interval
//     (e0_j - |omega_A,j|, e0_j + |omega_A,j|), t2 likewise with omega_c: the workgroup accumulates, while it stages the
//     node entries of its row, the extremes of the interval ends over all nodes -- min / max of the lower ends, min / max of
//     the upper ends, max of 1 / half-width (RowBands) -- and judges every point against these ten numbers AFTER the march
//     (round 2 kept running minima and maxima of t1 and t2 per point and node: 56 of the 560 VALU instructions of a loop
//     iteration).  With S = tau (omega^2 + omega_A^2(boundary)) and delta = S max_j(1 / a_j): all t_j > S if omega is more
//     than delta outside every interval, all t_j < -S if it is more than delta inside every interval; anything else -- the
//     continuum points and a margin around the band edges -- goes to fp64, which decides with the per-node tracking of
//     the fp64 kernels.  Twisted family in addition, per point: the extremes of C3 over the nodes (the fp64 kernel watches the sign of C3 D; D keeps its sign at a vouched-for point) and the minimum of
//     |C3| - tau |D (rho t1 + r d/dr[..])| (how close C3 came to zero relative to its leading part).
template <bool TRACK>
struct ScreenF {
  v2f mn = {3.0e38f, 3.0e38f};                          // !TRACK: min |t1 t2|
  v2f c3m = {3.0e38f, 3.0e38f};
  v2f c3lo = {3.0e38f, 3.0e38f}, c3hi = {-3.0e38f, -3.0e38f};   // extremes of C3 over the nodes (twisted family)
};

// extremes over the nodes of a row of the intervals in which t1 (index 0) and t2 (index 1) are negative; fp32, rounded
// OUTWARDS (a bound that is off by an ulp must err on the side of "unsure")
struct RowBands {
  float lo_min[2] = {3.0e38f, 3.0e38f}, lo_max[2] = {-3.0e38f, -3.0e38f};
  float hi_min[2] = {3.0e38f, 3.0e38f}, hi_max[2] = {-3.0e38f, -3.0e38f};
  float inv_a[2] = {0.0f, 0.0f};
  __device__ __forceinline__ static float down(double x) { const float f = (float)x; return f - fabsf(f) * 2.4e-7f - 1e-37f; }
  __device__ __forceinline__ static float up(double x) { const float f = (float)x; return f + fabsf(f) * 2.4e-7f + 1e-37f; }
  __device__ __forceinline__ void add(int t, double centre, double a) {
    const double lo = centre - a, hi = centre + a;
    lo_min[t] = fminf(lo_min[t], down(lo)); lo_max[t] = fmaxf(lo_max[t], up(lo));
    hi_min[t] = fminf(hi_min[t], down(hi)); hi_max[t] = fmaxf(hi_max[t], up(hi));
    inv_a[t] = fmaxf(inv_a[t], (a > 0.0) ? up(1.0 / a) : 3.0e38f);
  }
  // all lanes of the workgroup end up with the extremes over the whole workgroup; `red` = 10 * (T / 64) floats of LDS
  __device__ __forceinline__ void reduce(float* red, int T) {
    float v[10] = {lo_min[0], lo_min[1], hi_min[0], hi_min[1], -lo_max[0], -lo_max[1], -hi_max[0], -hi_max[1], -inv_a[0], -inv_a[1]};
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v[i] = fminf(v[i], __shfl_xor(v[i], off));
    const int wave = threadIdx.x >> 6, nwaves = T >> 6;
    __syncthreads();                                   // the LDS table of the last chunk is no longer read
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int i = 0; i < 10; ++i) red[wave * 10 + i] = v[i];
    __syncthreads();
    for (int wv = 0; wv < nwaves; ++wv)
#pragma unroll
      for (int i = 0; i < 10; ++i) v[i] = fminf(v[i], red[wv * 10 + i]);
    lo_min[0] = v[0]; lo_min[1] = v[1]; hi_min[0] = v[2]; hi_min[1] = v[3];
    lo_max[0] = -v[4]; lo_max[1] = -v[5]; hi_max[0] = -v[6]; hi_max[1] = -v[7]; inv_a[0] = -v[8]; inv_a[1] = -v[9];
  }
  // 0: every t_j of term t is certainly > S;  1: certainly < -S;  -1: cannot tell.
  // t = (|Om| - a)(|Om| + a): outside an interval by d, t > d (d + 2 a), i.e. > S once d >= sqrt(S) or d >= S / (2 a);
  // inside by d, -t > d a, i.e. > S once d >= S / a.
  __device__ __forceinline__ int sign_of(int t, double w, double S) const {
    const double d_in = S * (double)inv_a[t];
    const double d_out = fmin(sqrt(S), 0.5 * d_in);
    if (w < (double)lo_min[t] - d_out || w > (double)hi_max[t] + d_out) return 0;
    if (w > (double)lo_max[t] + d_in && w < (double)hi_min[t] - d_in) return 1;
    return -1;
  }
  // the same for ONE node (interval centre e0, half-width a, both fp64): +1 / -1 certain sign of t there, 0 cannot tell
  __device__ __forceinline__ static int node_sign(double w, double S, double e0, double a) {
    const double d = fabs(w - e0) - a;
    if (d >= fmin(sqrt(S), a > 0.0 ? 0.5 * S / a : INFINITY) * (1.0 + 1e-6)) return 1;
    if (a > 0.0 && -d >= (S / a) * (1.0 + 1e-6)) return -1;
    return 0;
  }
};

// per-row scalars of the flow slab in fp32 (KScal: k^2 c^2, k^2 vA^2, k^2 cT^2, k^4 cT^2 c^2; S_i)
struct SlabScalF { float kc2, kvA2, kcT2, k4c, S; };

// Units of the march.  The fp32 march runs on speeds / V and densities / R, V = 2^ev and R = 4^er chosen per problem
// (es_problem::f32_ev, f32_er), so that its products (t1 t2 ~ omega^4, their product over two nodes ~ omega^8, C3 ~
// rho^2 omega^8) stay inside the 8 bits of exponent whatever units the caller uses: with speeds in m/s the product of the
// two denominators of a step overflowed, v_rcp_f32 returned 0 and the march went on with finite, wrong coefficients.
// Node entry f of make_entry has the dimension speed^a density^b; entry_unit_exp is the binary exponent of V^a R^b.  The
// entries are divided by it in fp64 before their one rounding to fp32, omega by V, the flow slab's row scalars alike; every
// threshold after the march is formed from these normalised numbers.  A power of two changes no mantissa, so at any units
// the march delivers what it delivers at the normalised ones.  What goes back to the fp64 boundary algebra is the adjoint
// pair at its true scale: a12 = [u1]/[u2] per length has the dimension V^2 R (cylinders: P / xi_r), 1 / (V^2 R) (density
// slab: Vx / (F Vx')) or none (flow slab), a21 the inverse, and with r1 = r1~ the second component is r2 = r2~ [u1]/[u2]
// (ratio_unit_exp) for both start values of the march, (1, 0) and (a11, a12).
template <int FAM>
__device__ __forceinline__ int entry_unit_exp(int f, int ev, int er) {
  if (FAM == FAM_CYL0) {
    const int a[7] = {1, 2, 2, 0, -2, 0, 2}, b2[7] = {0, 0, 0, 2, -2, -2, -2};
    return a[f] * ev + b2[f] * er;
  } else if (FAM == FAM_CYLT) {
    const int a[16] = {1, 2, 2, 2, 0, 2, 2, 3, 2, 1, 2, 2, 2, 2, 0, 0}, b2[16] = {0, 0, 0, 2, 2, 2, 2, 2, 2, 2, 0, 0, 2, 0, 0, 0};
    return a[f] * ev + b2[f] * er;
  } else if (FAM == FAM_SLABD) {
    const int a[5] = {2, 2, 2, 2, 0}, b2[5] = {0, 0, 0, 2, 2};
    return a[f] * ev + b2[f] * er;
  }
  return ev;                                           // flow slab: k U, k U', k U'', 2 k U'
}
template <int FAM>
__device__ __forceinline__ int ratio_unit_exp(int ev, int er) {
  return (FAM == FAM_CYL0 || FAM == FAM_CYLT) ? 2 * (ev + er) : (FAM == FAM_SLABD) ? -2 * (ev + er) : 0;
}

// C1P = c1_power of the twisted family as a template parameter: a runtime select between Om and Om^2 costs two
// v_cndmask_b32 per pair and node (the kernel branches once per chunk instead).
template <int FAM, bool TRACK, int C1P = 1>
__device__ __forceinline__ void coef_pre_f32(const float* e, v2f w, CoefPreF& C, ScreenF<TRACK>& sc,
                                             const SlabScalF& ss) {
  if (FAM == FAM_SLABD) {
    // density slab (coef_pre<FAM_SLABD>): u' = v / F, v' = F m0 u; watched terms n1, n2, n3 (band family: the smallest
    // of their magnitudes over the nodes says how close a coefficient came to a singular point)
    const v2f w2 = w * w;
    const v2f n1 = v2(e[0]) - w2, n2 = v2(e[1]) - w2, n3 = v2(e[2]) - w2;
    sc.mn = vmin(sc.mn, vmin(vmin(vabs(n1), vabs(n2)), vabs(n3)));
    C.n11 = v2(0.0f); C.n22 = v2(0.0f);
    C.n12 = n1;
    C.n21 = v2(e[4]) * n3;
    C.den = v2(e[3]) * n2;
    return;
  }
  if (FAM == FAM_SLABF) {
    // flow slab (coef_pre<FAM_SLABF>): m0, D, coeff of SF-G:416-427 over the common denominator S t Om^2 n1; watched terms
    // n1, t, n3 and Om (as Om^2, on the scale of the others)
    const v2f Om = w - v2(e[0]);
    const v2f Om2 = Om * Om;
    const v2f t = Om2 - v2(ss.kcT2), n1 = v2(ss.kc2) - Om2, n3 = v2(ss.kvA2) - Om2;
    sc.mn = vmin(sc.mn, vmin(vmin(vabs(n1), vabs(t)), vmin(vabs(n3), Om2)));
    const v2f St = v2(ss.S) * t;
    const v2f G = vfma(St, t, v2(ss.k4c));
    const v2f X = Om * n1;
    const v2f OX = Om * X;
    const v2f g2 = v2(e[3]) * G;
    C.n11 = v2(0.0f);
    C.n12 = v2(1.0f);
    C.n22 = g2 * Om;
    C.n21 = -vfma(v2(e[2]), St * X, vfma(-g2, v2(e[1]), (n1 * n3) * OX));
    C.den = St * OX;
    return;
  }
  const v2f Om = w - v2(e[0]);
  const v2f Om2 = Om * Om;
  const v2f t1 = Om2 - v2(e[1]);
  const v2f t2 = Om2 - v2(e[2]);
  const v2f t12 = t1 * t2;
  if (!TRACK) sc.mn = vmin(sc.mn, vabs(t12));
  if (FAM == FAM_CYL0) {
    C.n11 = v2(0.0f);
    C.n12 = v2(e[3]) * t1;
    C.n21 = vfma(v2(e[5]), t2, v2(e[6]));
    C.n22 = v2(e[4]);
    C.den = t12;
  } else {
    const v2f D = v2(e[3]) * t12;
    const v2f Q = vfma(Om, v2(e[7]), vfma(Om2, v2(e[6]), -(t1 * v2(e[5]))));
    const v2f T = vfma(v2(e[9]), Om, v2(e[8]));
    const v2f OmP = (C1P == 2) ? Om2 : Om;
    const v2f t2T = t2 * T;
    const v2f C1 = vfma(Q, OmP, -(v2(e[10]) * t2T));
    const v2f C2 = vfma(Om2, Om2, -(v2(e[11]) * t2));
    const v2f c3a = D * vfma(v2(e[4]), t1, v2(e[12]));
    const v2f C3 = c3a + vfma(Q, Q, -(v2(e[13]) * t2T * T));
    // third watched term of the fp64 kernel: the sign of F = r D / C3, i.e. of C3 D.  A point is only vouched for when t1
    // and t2 keep one sign over all nodes (RowBands), and e[3] = rho S > 0: D = e[3] t1 t2 then keeps its sign and C3 D
    // changes sign exactly where C3 does -- C3 itself is tracked (no product per node).
    // (its extremes over the nodes: with the two nodes of a step one v_min3_f32 and one v_max3_f32 per point, where OR-ing
    // and AND-ing the sign bits took four integer instructions)
    sc.c3lo.x = fminf(sc.c3lo.x, C3.x); sc.c3hi.x = fmaxf(sc.c3hi.x, C3.x);
    sc.c3lo.y = fminf(sc.c3lo.y, C3.y); sc.c3hi.y = fmaxf(sc.c3hi.y, C3.y);
    // |C3| - tau |c3a| per component with the source modifiers of the unpacked v_fma_f32 (the packed form has no |x|
    // modifier: four v_and_b32 and a v_pk_fma_f32 per pair and node)
    sc.c3m.x = fminf(sc.c3m.x, fmaf(-F32_TAU_NODE, fabsf(c3a.x), fabsf(C3.x)));
    sc.c3m.y = fminf(sc.c3m.y, fmaf(-F32_TAU_NODE, fabsf(c3a.y), fabsf(C3.y)));
    C.n11 = v2(0.0f);                                   // a11 = -a22: not formed (rk4_step_adjoint_f32 negates a22)
    C.n22 = C1;
    C.n12 = C3 * v2(e[15]);
    C.n21 = -(v2(e[14]) * C2);
    C.den = D;
  }
}

template <int FAM>
__device__ __forceinline__ void coef_finish_f32(const CoefPreF& C, v2f inv, CoefF& A) {
  if (FAM == FAM_CYL0) {
    A.a11 = v2(0.0f); A.a22 = v2(0.0f); A.a12 = C.n12; A.a21 = vfma(C.n21, inv, C.n22);
  } else if (FAM == FAM_SLABD) {
    A.a11 = v2(0.0f); A.a22 = v2(0.0f); A.a12 = C.n12 * inv; A.a21 = C.n21;
  } else if (FAM == FAM_SLABF) {
    A.a11 = v2(0.0f); A.a12 = v2(1.0f); A.a21 = C.n21 * inv; A.a22 = C.n22 * inv;
  } else {
    A.a11 = v2(0.0f); A.a22 = C.n22 * inv; A.a12 = C.n12 * inv; A.a21 = C.n21 * inv;       // a11 = -a22
  }
}

template <int FAM>
__device__ __forceinline__ void rk4_step_adjoint_f32(v2f& p, v2f& q, const CoefF& B0, const CoefF& Bm, const CoefF& B1,
                                                     float h, float h2, float h6, float h3) {
#define ES_RHS_TF(A, pp, qq, kp, kq)                                                            \
  if (FAM == FAM_CYLT)       { kp = vfma(-A.a22, pp, A.a21 * qq); kq = vfma(A.a22, qq, A.a12 * pp); } \
  else if (FAM == FAM_SLABF) { kp = A.a21 * qq;                  kq = vfma(A.a22, qq, pp); }         \
  else                       { kp = A.a21 * qq;                  kq = A.a12 * pp; }
  v2f k1p, k1q, k2p, k2q, k3p, k3q, k4p, k4q, tp, tq;
  ES_RHS_TF(B0, p, q, k1p, k1q);
  tp = vfma(v2(h2), k1p, p); tq = vfma(v2(h2), k1q, q);
  ES_RHS_TF(Bm, tp, tq, k2p, k2q);
  tp = vfma(v2(h2), k2p, p); tq = vfma(v2(h2), k2q, q);
  ES_RHS_TF(Bm, tp, tq, k3p, k3q);
  tp = vfma(v2(h), k3p, p); tq = vfma(v2(h), k3q, q);
  ES_RHS_TF(B1, tp, tq, k4p, k4q);
  p = vfma(v2(h6), k1p + k4p, vfma(v2(h3), k2p + k3p, p));
  q = vfma(v2(h6), k1q + k4q, vfma(v2(h3), k2q + k3q, q));
#undef ES_RHS_TF
}

// One RK4 step of the fp32 march for the NP pairs of a lane.  `node` = the fp32 entries of node 2J in the LDS table,
// those of the mid-point 2J + 1 follow NES floats later (node-major table: every entry of a step sits at a constant
// offset from ONE uniform address -- ds_read_b128 with immediate offsets; the field-major table of round 2 needed a
// base register of its own per field: 16 v_mov_b32 + 25 s_add_i32 per loop iteration of the twisted family).
template <int FAM, int NP, bool TRACK, int C1P>
__device__ __forceinline__ void f32_step(const float* node, const v2f* wf, v2f* zp, v2f* zq, const CoefF* BIN, CoefF* BOUT,
                                         ScreenF<TRACK>* scr, const SlabScalF& ss, float h, float h2, float h6, float h3) {
  constexpr int NE = FamTraits<FAM>::NE;
  constexpr int NES = (NE + 3) & ~3;
  float em[NE], e1[NE];
#pragma unroll
  for (int f = 0; f < NE; ++f) { e1[f] = node[f]; em[f] = node[NES + f]; }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    CoefPreF Cm, C1;
    coef_pre_f32<FAM, TRACK, C1P>(em, wf[p], Cm, scr[p], ss);
    coef_pre_f32<FAM, TRACK, C1P>(e1, wf[p], C1, scr[p], ss);
    const v2f inv = vrcp(Cm.den * C1.den);
    CoefF Bm;
    coef_finish_f32<FAM>(Cm, C1.den * inv, Bm);
    coef_finish_f32<FAM>(C1, Cm.den * inv, BOUT[p]);
    rk4_step_adjoint_f32<FAM>(zp[p], zq[p], BIN[p], Bm, BOUT[p], h, h2, h6, h3);
  }
}

// The steps of one LDS chunk (nst of them, from the far end of the chunk towards the boundary).  The adjoint march is
// renormalised: fp32 has 8 bits of exponent, an evanescent interior grows like e^{kappa (1 - r_ax)} (1e30 and more at
// large k).  Both components are scaled by a power of two whenever they leave [2^-40, 2^40]; the boundary algebra only
// uses the ratio r1 : r2 and the (rescaled) target of the axis condition.
template <int FAM, int NP, bool TRACK, int C1P>
__device__ __forceinline__ void f32_march_chunk(const float* lds, int nst, bool first, bool sausage_axis, const v2f* wf,
                                                v2f* zp, v2f* zq, int* zexp, CoefF* B0, CoefF* B1, ScreenF<TRACK>* scr,
                                                const SlabScalF& ss, float h, float h2, float h6, float h3) {
  constexpr int NE = FamTraits<FAM>::NE;
  constexpr int NES = (NE + 3) & ~3;
  if (first) {                                         // far end of the march: coefficients of the last node, start values
    float eL[NE];
#pragma unroll
    for (int f = 0; f < NE; ++f) eL[f] = lds[2 * nst * NES + f];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      CoefPreF C;
      coef_pre_f32<FAM, TRACK, C1P>(eL, wf[p], C, scr[p], ss);
      coef_finish_f32<FAM>(C, v2(1.0f) / C.den, B0[p]);
      if ((FAM == FAM_CYL0 || FAM == FAM_CYLT) && sausage_axis) {
        zp[p] = (FAM == FAM_CYLT) ? -B0[p].a22 : B0[p].a11;
        zq[p] = B0[p].a12;
      } else { zp[p] = v2(1.0f); zq[p] = v2(0.0f); }
    }
  }
  // steps in pairs with the roles of B0 / B1 swapped (no coefficient copies); CH is even, so only the last chunk of an
  // odd march has a single leading step
  int j = nst - 1;
  if (nst & 1) {
    f32_step<FAM, NP, TRACK, C1P>(lds + 2 * j * NES, wf, zp, zq, B0, B1, scr, ss, h, h2, h6, h3);
#pragma unroll
    for (int p = 0; p < NP; ++p) B0[p] = B1[p];
    --j;
  }
  for (; j >= 1; j -= 2) {
    f32_step<FAM, NP, TRACK, C1P>(lds + 2 * j * NES, wf, zp, zq, B0, B1, scr, ss, h, h2, h6, h3);
    f32_step<FAM, NP, TRACK, C1P>(lds + 2 * (j - 1) * NES, wf, zp, zq, B1, B0, scr, ss, h, h2, h6, h3);
    if (((j - 1) & 31) == 0) {                         // renormalise every 32 steps
#pragma unroll
      for (int p = 0; p < 2 * NP; ++p) {
        float a = (p & 1) ? zp[p >> 1].y : zp[p >> 1].x;
        float b = (p & 1) ? zq[p >> 1].y : zq[p >> 1].x;
        const float mag = fmaxf(fabsf(a), fabsf(b));
        if (mag > 1.0995116e12f || (mag < 9.094947e-13f && mag > 0.0f)) {       // outside [2^-40, 2^40]
          int ex;
          (void)frexpf(mag, &ex);
          a = ldexpf(a, -ex);
          b = ldexpf(b, -ex);
          zexp[p] += ex;
          if (p & 1) { zp[p >> 1].y = a; zq[p >> 1].y = b; } else { zp[p >> 1].x = a; zq[p >> 1].x = b; }
        }
      }
    }
  }
}

// The closed-form exterior (fp64 Bessel code, ~100 VGPRs) is evaluated AFTER the march, when the loop state is dead;
// before the march only the sign of m_e is needed to know which lanes have something to march.
template <int FAM, int PTS, int MAXT, bool TRACK, int WPE>
__global__ __launch_bounds__(MAXT) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void shoot_grid_f32_kernel(ShootDev P, const double* __restrict__ kv, int nk, const double* __restrict__ wv, int nw,
                           int w_mode, int ev, int er, double* __restrict__ Dout, uint8_t* __restrict__ stout) {
  static_assert(PTS % 2 == 0, "points are processed in pairs");
  constexpr int NP = PTS / 2;
  constexpr int NE = FamTraits<FAM>::NE;
  constexpr int NES = (NE + 3) & ~3;                   // floats per node in the LDS table (16-byte rows)
  __shared__ __align__(16) float lds[NES * (2 * CH + 1)];
  const int T = blockDim.x;
  const int nsteps = P.n_nodes - 1;
  const float h = (float)P.h, h2 = (float)(0.5 * P.h), h6 = (float)(P.h / 6.0), h3 = (float)(P.h / 3.0);
  const int nseg = (nw + T * PTS - 1) / (T * PTS);
  const long ntiles = (long)nk * nseg;
  for (long tile = es_tile_index(), once = 1; once && tile < ntiles; once = 0) {
    const int seg = (int)(tile / nk);                  // segment-major, as in shoot_grid_kernel (XCD balance)
    const int row = (int)(tile - (long)seg * nk);
    const int w0 = seg * T * PTS;
    const double k = kv[row];
    const KScal s = make_kscal(P, k);
    const SlabScalF ss = {(float)ldexp(s.kc2, -2 * ev), (float)ldexp(s.kvA2, -2 * ev), (float)ldexp(s.kcT2, -2 * ev),
                          (float)ldexp(s.k4c, -4 * ev), (float)ldexp(P.S_i, -2 * ev)};
    v2f wf[NP], zp[NP], zq[NP];
    int zexp[PTS];                                     // accumulated power-of-two scaling of (zp, zq), per point
    CoefF B0[NP], B1[NP];
    ScreenF<TRACK> scr[NP];
    bool lane_live = false;
#pragma unroll
    for (int p = 0; p < PTS; ++p) {
      const int iw = w0 + p * T + (int)threadIdx.x;
      const double w = (iw < nw) ? pick_w(wv, w_mode, k, row, nw, iw) : 1.0;
      const float wn = (float)ldexp(w, -ev);            // omega / V
      if (p & 1) wf[p >> 1].y = wn; else wf[p >> 1].x = wn;
      // m_e > 0 (evanescent exterior) and, for the band families, not inside a continuum band: worth a march
      const double Oe = (FAM == FAM_SLABD || FAM == FAM_SLABF) ? (w - k * P.U_e) : w;
      const double k2 = k * k, w2 = Oe * Oe;
      const double m_e = ((k2 * P.vAe2 - w2) * (k2 * P.ce2 - w2)) / (P.Se * (k2 * P.cTe2 - w2));
      const bool dead = !TRACK && band_crossed(P, k, w);
      lane_live = lane_live || (iw < nw && m_e > 0.0 && !dead);
      zexp[p] = 0;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) { zp[p] = v2(0.0f); zq[p] = v2(0.0f); }
    const bool wave_live = __any(lane_live);
    const bool wg_live = __syncthreads_or(wave_live ? 1 : 0) != 0;
    const int nchunks = wg_live ? (nsteps + CH - 1) / CH : 0;
    const bool sausage_axis = P.axis_bc == ES_AXIS_SAUSAGE;
    RowBands bands;
    for (int c = nchunks - 1; c >= 0; --c) {
      const int c0 = c * CH;
      const int nst = (nsteps - c0 < CH) ? (nsteps - c0) : CH;
      __syncthreads();
      for (int i = threadIdx.x; i < 2 * nst + ES_FAR_NODE(c, nchunks); i += T) {   // far node: first chunk only (es_shoot_grid_body.hpp)
        double b[FamTraits<FAM>::NB], e[NE];
        load_base<FAM>(P, 2 * c0 + i, b);
        make_entry<FAM>(b, s, e);                      // fp64, brought to the units of the march, rounded to fp32 once
#pragma unroll
        for (int f = 0; f < NE; ++f) e[f] = ldexp(e[f], -entry_unit_exp<FAM>(f, ev, er));
        float ef32[NES];
#pragma unroll
        for (int f = 0; f < NES; ++f) ef32[f] = (f < NE) ? (float)e[f] : 0.0f;
#pragma unroll
        for (int f = 0; f < NES; f += 4)
          *reinterpret_cast<float4*>(&lds[i * NES + f]) = make_float4(ef32[f], ef32[f + 1], ef32[f + 2], ef32[f + 3]);
        if (TRACK) {                                   // where t1 / t2 are negative at this node: omega within a of e0
          bands.add(0, e[0], sqrt(e[1]));
          bands.add(1, e[0], sqrt(e[2]));
        }
      }
      __syncthreads();
      if (!wave_live) continue;
      if (FAM == FAM_CYLT && P.c1_power == 2)
        f32_march_chunk<FAM, NP, TRACK, 2>(lds, nst, c == nchunks - 1, sausage_axis, wf, zp, zq, zexp, B0, B1, scr, ss, h, h2, h6, h3);
      else
        f32_march_chunk<FAM, NP, TRACK, 1>(lds, nst, c == nchunks - 1, sausage_axis, wf, zp, zq, zexp, B0, B1, scr, ss, h, h2, h6, h3);
    }
    if (TRACK && wg_live) bands.reduce(lds, T);        // workgroup-uniform condition (the reduction has barriers)
    // the exterior code below needs products of k the prologue has already formed (k^2 vA_e^2, ...): reused, they would
    // sit in registers across the whole march -- and did not fit (five spilled doubles per lane, 10 MB of scratch writes
    // per launch).  An opaque copy of k makes the compiler form them again here.
    double kx = k;
    asm volatile("" : "+v"(kx));
    double bf[FamTraits<FAM>::NB], ef[NE];
    load_base<FAM>(P, 0, bf);
    make_entry<FAM>(bf, s, ef);
    // the watched terms are judged in the units of the march: efn, emid, elast are entries 0 - 2 of the boundary node and of
    // two more sampled nodes (e0, omega_A^2, omega_c^2; the slabs read efn[0] alone) over their units
    double efn[3], emid[3] = {0.0, 0.0, 0.0}, elast[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int f = 0; f < 3; ++f) efn[f] = ldexp(ef[f], -entry_unit_exp<FAM>(f, ev, er));
    if (TRACK) {
      double et[NE];
      load_base<FAM>(P, P.npts / 2, bf);
      make_entry<FAM>(bf, s, et);
#pragma unroll
      for (int f = 0; f < 3; ++f) emid[f] = ldexp(et[f], -entry_unit_exp<FAM>(f, ev, er));
      load_base<FAM>(P, P.npts - 1, bf);
      make_entry<FAM>(bf, s, et);
#pragma unroll
      for (int f = 0; f < 3; ++f) elast[f] = ldexp(et[f], -entry_unit_exp<FAM>(f, ev, er));
      load_base<FAM>(P, 0, bf);
    }
    const double r2_unit = ldexp(1.0, ratio_unit_exp<FAM>(ev, er));
#pragma unroll
    for (int p = 0; p < PTS; ++p) {
      const int iw = w0 + p * T + (int)threadIdx.x;
      if (iw >= nw) continue;
      const double w = pick_w(wv, w_mode, kx, row, nw, iw);
      const ExteriorLite X = exterior_lite(P, kx, w, w);
      const bool hi_half = (p & 1);
      const ScreenF<TRACK>& sc = scr[p >> 1];
      const float zpp = hi_half ? zp[p >> 1].y : zp[p >> 1].x;
      const float zqq = hi_half ? zq[p >> 1].y : zq[p >> 1].x;
      // r = (r1, r2) * 2^zexp: the common factor multiplies the homogeneous part of the axis condition; its target
      // (bc_const * xi_e, non-zero only for the twisted kink condition) is divided by it instead
      ShootDev Pl = P;
      Pl.bc_const = P.bc_const_raw * ldexp(1.0, -zexp[p]);
      Pl.slab_sign = P.slab_sign * ldexp(1.0, -zexp[p]);          // slabs: (slab_sign - r1) / r2 with r = (r1, r2) 2^zexp
      const double r1 = (double)zpp, r2 = (double)zqq * r2_unit;   // the adjoint pair at its true scale (up to 2^zexp)
      const Mismatch M = boundary_algebra<FAM>(Pl, s, w, X, r1, r2, ef);
      // watched terms: certain sign / certain crossing / unsure (see ScreenF), in the units of the march
      const double wn = ldexp(w, -ev);
      const float S = F32_TAU_NODE * (float)(wn * wn + efn[1]);
      bool crossed, node_unsure;
      if (!TRACK) {                                     // band families: the status is exact (fp64 test on W = omega/k)
        crossed = band_crossed(P, kx, w);
        const float mnp = hi_half ? sc.mn.y : sc.mn.x;
        if (FAM == FAM_SLABD || FAM == FAM_SLABF) {
          // slabs: the smallest magnitude of a watched term over the nodes against tau x the scale of these terms
          // (omega^2 + k^2 c^2; the flow slab's omega is the Doppler-shifted one at the boundary)
          const double Omb = (FAM == FAM_SLABF) ? (wn - efn[0]) : wn;
          const float sz = (float)(Omb * Omb + ((FAM == FAM_SLABF) ? ldexp(s.kc2, -2 * ev) : efn[0]));
          node_unsure = !crossed && !(mnp > F32_TAU_NODE * sz);
        } else {
        // an evaluated point with a coefficient close to a singular point: |t1 t2| below tau (omega^2 + omega_A^2)^2 at
        // some node, i.e. ONE of the two factors within tau of zero relative to its size
        const float sz = (float)(wn * wn + efn[1]);
        node_unsure = !crossed && !(mnp > F32_TAU_NODE * sz * sz);
        }
      } else {
        const float c3m = hi_half ? sc.c3m.y : sc.c3m.x;
        const float c3lo = hi_half ? sc.c3lo.y : sc.c3lo.x, c3hi = hi_half ? sc.c3hi.y : sc.c3hi.x;
        // t1, t2: certainly of one sign at every node (judged from the row's interval extremes); or certainly of BOTH signs
        // inside the domain, seen at three sampled nodes (boundary, middle, far end: one of them certainly negative, another
        // certainly positive => ES_PT_CONTINUUM whatever happens in between -- most of a continuum band of a monotone
        // profile); anything else is the margin fp64 decides
        const bool sure12 = bands.sign_of(0, wn, (double)S) >= 0 && bands.sign_of(1, wn, (double)S) >= 0;
        bool cross12 = false;
        if (!sure12) {
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int s0 = RowBands::node_sign(wn, (double)S, efn[0], sqrt(efn[1 + t]));
            const int s1 = RowBands::node_sign(wn, (double)S, emid[0], sqrt(emid[1 + t]));
            const int s2 = RowBands::node_sign(wn, (double)S, elast[0], sqrt(elast[1 + t]));
            cross12 = cross12 || ((s0 < 0 || s1 < 0 || s2 < 0) && (s0 > 0 || s1 > 0 || s2 > 0));
          }
        }
        if (cross12) {
          crossed = true; node_unsure = false;
        } else if (sure12 && (FAM != FAM_CYLT || c3m >= 0.0f)) {
          crossed = (FAM == FAM_CYLT) && (c3lo < 0.0f) && (c3hi >= 0.0f);   // C3 takes both signs (c3m >= 0: never within tau of 0)
          node_unsure = false;
        } else {
          crossed = false; node_unsure = true;
        }
      }
      double D, rel; uint8_t st;
      finish_point(P, M, X, crossed, D, rel, st);
      if (!TRACK && crossed && X.status == ES_PT_OK) { st = ES_PT_CONTINUUM; D = NAN; }   // not marched: no D to judge
      bool unsure = false;
      if (X.status == ES_PT_OK && crossed) {
        unsure = TRACK && !isfinite(M.d);               // fp64 reports ES_PT_NONFINITE before ES_PT_CONTINUUM: let it decide
      } else if (X.status == ES_PT_OK) {
        double scale = fmax(fabs(M.outer), fabs(M.inner));
        if (FAM == FAM_SLABD || FAM == FAM_SLABF) {
          // slabs: the inner term is (slab_sign - r1) x ..., and r1 -- an element of the transfer matrix of an oscillating
          // solution -- comes close to +-1: the fp32 error of r1 is then measured against the terms BEFORE the cancellation.
          // The same algebra with the sign of slab_sign chosen so that nothing cancels gives that magnitude.
          ShootDev Pb = Pl;
          Pb.slab_sign = (zpp >= 0.0f) ? -fabs(Pl.slab_sign) : fabs(Pl.slab_sign);
          const Mismatch Mb = boundary_algebra<FAM>(Pb, s, w, X, r1, r2, ef);
          scale = fmax(scale, fabs(Mb.inner));
        }
        unsure = node_unsure || !isfinite(M.d) || !(fabs(M.d) > F32_TAU_D * scale) ||
                 !(fabs(M.outer) > F32_TAU_POLE * fabs(M.inner));
      }
      const size_t o = (size_t)row * nw + iw;
      Dout[o] = D;
      stout[o] = unsure ? (uint8_t)(st | F32_UNSURE) : st;
    }
  }
}

template <int FAM>
int launch_grid_f32(es_context* ctx, const es_problem* prob, const double* d_k, int nk, const double* d_w, int nw,
                    int w_mode, double* d_D, uint8_t* d_status) {
  if constexpr (FAM == FAM_CYL0 || FAM == FAM_CYLT) {
    es_timer_begin(ctx);
    constexpr int PTS = 4;
    int T = ((nw + PTS - 1) / PTS + 63) / 64 * 64;
    if (T < 64) T = 64;
    if (T > 256) T = 256;
    const long tiles = (long)nk * ((nw + T * PTS - 1) / (T * PTS));
    const dim3 grid = es_tile_grid(tiles);
    const bool bands = fam_has_bands<FAM>() && prob->dev.use_bands;
    // register caps: 128 VGPRs (4 waves per SIMD) for the untwisted family, 168 (3 waves) for the twisted one
    if constexpr (FAM == FAM_CYL0) {
      int v0 = 0;
      if (const char* ev = getenv("ES_F32_VARIANT")) v0 = atoi(ev);             // tuning aid
      if (bands && v0 == 1)
        hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, PTS, 256, false, 3>), grid, dim3(T), 0, ctx->stream,
                           prob->dev, d_k, nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
      else if (bands && v0 == 2)
        hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, PTS, 256, false, 2>), grid, dim3(T), 0, ctx->stream,
                           prob->dev, d_k, nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
      else if (bands && v0 == 3) {
        int T8 = ((nw + 7) / 8 + 63) / 64 * 64;
        if (T8 < 64) T8 = 64;
        if (T8 > 256) T8 = 256;
        const long t8 = (long)nk * ((nw + T8 * 8 - 1) / (T8 * 8));
        hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, 8, 256, false, 2>), es_tile_grid(t8),
                           dim3(T8), 0, ctx->stream, prob->dev, d_k, nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
      } else if (bands)
        hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, PTS, 256, false, 4>), grid, dim3(T), 0, ctx->stream,
                           prob->dev, d_k, nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
      else
        hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, PTS, 256, true, 4>), grid, dim3(T), 0, ctx->stream,
                           prob->dev, d_k, nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
    } else {
      // measured on configs[4] (1024^2, N = 2000), packed fp32: 4 points per lane at 2 waves per SIMD (no spills) 4.5 ms;
      // the same capped at 168 registers (3 waves, spills) 5.6 ms; 2 points per lane at 4 waves 4.7 ms; fp64 9.4 ms
      int variant = 1;
      if (const char* ev = getenv("ES_F32_VARIANT")) variant = atoi(ev);        // tuning aid
      if (variant == 1) {
        hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, PTS, 256, true, 2>), grid, dim3(T), 0, ctx->stream,
                           prob->dev, d_k, nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
      } else if (variant == 2) {
        int T2 = ((nw + 1) / 2 + 63) / 64 * 64;
        if (T2 < 64) T2 = 64;
        if (T2 > 256) T2 = 256;
        const long tiles2 = (long)nk * ((nw + T2 * 2 - 1) / (T2 * 2));
        hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, 2, 256, true, 4>), es_tile_grid(tiles2),
                           dim3(T2), 0, ctx->stream, prob->dev, d_k, nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
      } else {
        hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, PTS, 256, true, 3>), grid, dim3(T), 0, ctx->stream,
                           prob->dev, d_k, nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
      }
    }
    es_timer_end(ctx);
    ES_HIP_CHECK(ctx, hipGetLastError());
    return ES_SUCCESS;
  } else {
    // slab families: band problems only (their status is exact from the phase speed; a profile whose node intervals do not
    // overlap falls back to per-node tracking in fp64, which the fp32 pass has no counterpart of)
    if (!prob->dev.use_bands) {
      ctx->last_error = "fp32 screening of a slab needs connected continuum bands (per-node sign tracking: fp64 only)";
      return ES_ERR_UNSUPPORTED;
    }
    es_timer_begin(ctx);
    constexpr int PTS = 4;
    int T = ((nw + PTS - 1) / PTS + 63) / 64 * 64;
    if (T < 64) T = 64;
    if (T > 256) T = 256;
    const long tiles = (long)nk * ((nw + T * PTS - 1) / (T * PTS));
    const dim3 grid = es_tile_grid(tiles);
    hipLaunchKernelGGL((shoot_grid_f32_kernel<FAM, PTS, 256, false, 3>), grid, dim3(T), 0, ctx->stream, prob->dev, d_k,
                       nk, d_w, nw, w_mode, prob->f32_ev, prob->f32_er, d_D, d_status);
    es_timer_end(ctx);
    ES_HIP_CHECK(ctx, hipGetLastError());
    return ES_SUCCESS;
  }
}
}  // namespace

int check_mixed_args(es_context* ctx, const es_problem* prob, int nk, int nw, int w_mode) {
  int rc = check_problem(ctx, prob);
  if (rc) return rc;
  ES_REQUIRE(ctx, nk >= 0 && nw >= 0, "negative size");
  ES_REQUIRE(ctx, w_mode >= 0 && w_mode <= 2, "w_mode");
  const int fam = prob->dev.family;
  if (fam < FAM_CYL0 || fam > FAM_SLABF) return ES_ERR_UNSUPPORTED;
  if ((fam == FAM_SLABD || fam == FAM_SLABF) && !prob->dev.use_bands) {
    ctx->last_error = "fp32 screening of a slab needs connected continuum bands (per-node sign tracking: fp64 only)";
    return ES_ERR_UNSUPPORTED;
  }
  return ES_SUCCESS;
}

// Step 1 of the mixed search alone: the fp32 screening march, enqueued (no read-back).
extern "C" int es_shoot_screen_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk, const double* d_w,
                                    int nw, int w_mode, double* d_D, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  int rc = check_mixed_args(ctx, prob, nk, nw, w_mode);
  if (rc) return rc;
  if ((long)nk * nw == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w && d_D && d_status, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define CALL_GRID_F32(F) launch_grid_f32<F>(ctx, prob, d_k, nk, d_w, nw, w_mode, d_D, d_status)
  ES_DISPATCH_FAMILY(prob->dev.family, CALL_GRID_F32)
#undef CALL_GRID_F32
}
