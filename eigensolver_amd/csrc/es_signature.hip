// Branch label of a (k, omega) pair: the number of sign changes of the interior eigenfunction rows, their maxima and where
// they sit (include/eigensolver_amd.h section 10).  What the reference's analysis scripts stand in for with hand-picked
// phase-speed cut-offs per data set (analysis_cylinder_flow_coronal.py:244-372: fast_sausage_branch1/2/3, slow_body_kink, ...).
// One (k, omega) pair per lane and the two marches of eigen_interior_kernel (es_eigenfunction.hip) -- same node entries,
// same coefficient sets, same RK4 step, same expressions for value and flux, so the entries reduced here are the ones that
// kernel writes -- but nothing is written per node: four integers and two doubles per row pair live in registers and each
// lane stores once per output at the end.
#include "es_shoot_shared.hpp"

namespace {
using namespace es_shoot_shared;

// Running reduction of one row.  DOWN: the march visits the nodes N-1 ... 0 (cylinders: from the axis node out to the
// boundary), so a later entry has the smaller index and >= keeps the smallest index that attains the maximum; the count of
// sign changes does not depend on the direction.
struct RowTrack {
  double peak = -1.0;      // max |x| so far; no entry yet: below every |x|
  int node = -1;
  int last = 0;            // sign of the last entry kept, 0: none yet
  int changes = 0;
  template <bool DOWN>
  __device__ __forceinline__ void add(double x, int j) {
    const int s = (x > 0.0) - (x < 0.0);                       // 0 for +-0 and NaN: the entry is skipped
    changes += ((s * last) < 0) ? 1 : 0;
    last = s ? s : last;
    const double a = fabs(x);
    const bool up = DOWN ? (a >= peak) : (a > peak);           // a NaN compares false: skipped here too
    peak = up ? a : peak;
    node = up ? j : node;
  }
};

template <int FAM>
__global__ __launch_bounds__(64) void mode_signature_kernel(ShootDev P, const double* __restrict__ kv,
                                                            const double* __restrict__ wv, int n,
                                                            const int32_t* __restrict__ d_count,
                                                            int32_t* __restrict__ nodes_value, int32_t* __restrict__ nodes_flux,
                                                            int32_t* __restrict__ peak_node_value,
                                                            int32_t* __restrict__ peak_node_flux,
                                                            double* __restrict__ peak_value, double* __restrict__ peak_flux,
                                                            uint8_t* __restrict__ status) {
  constexpr int NE = FamTraits<FAM>::NE;
  constexpr int NB = FamTraits<FAM>::NB;
  constexpr bool DIAG = FamTraits<FAM>::DIAG;
  constexpr bool CYL = (FAM == FAM_CYL0 || FAM == FAM_CYLT);
  if (d_count) {                                               // the count of an _async search: min(max(*d_count, 0), n)
    const int c = *d_count;
    n = c < n ? (c < 0 ? 0 : c) : n;
  }
  if ((int)(blockIdx.x * blockDim.x) >= n) return;             // the whole wave lies past the count
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const double k = in ? kv[i] : 1.0;
  const double w = in ? wv[i] : 1.0;
  const KScal s = make_kscal(P, k);
  const int nsteps = P.n_nodes - 1;
  const double h = P.h, h2 = 0.5 * P.h, h6 = P.h / 6.0, h3 = P.h / 3.0;
  SignTrack trk;
  double b[NB], e[NE], e2[NE];
  const ExteriorLite X = exterior_lite(P, k, w, w);
  const bool ok = X.status == ES_PT_OK;
  double u, v, flux_scale = 1.0;     // flux = v * flux_scale (density slab) ; see reduce
  RowTrack tv, tf;
  auto reduce = [&](int node, const double* en) {              // value and flux of a node: `store` of eigen_interior_kernel
    double f;
    if (CYL) {
      const double x = P.xb + (double)node * P.h;
      f = v / x;                                                  // xi_r = Xi / r
    } else if (FAM == FAM_SLABD) {
      f = v * flux_scale;
    } else {
      const double Om = w - en[0];
      const double Om2 = Om * Om;
      f = P.rho_i * P.S_i * (s.kcT2 - Om2) / (Om * (s.kc2 - Om2)) * v;    // P_Ti(x) Vx', SF-G:433
    }
    tv.add<CYL>(u, node);
    tf.add<CYL>(f, node);
  };
  if (CYL) {
    // axis node: coefficient set and the two columns of the axis state
    load_base<FAM>(P, 2 * nsteps, b);
    make_entry<FAM>(b, s, e);
    Coef Aax;
    coefficients<FAM>(e, P, s, w, Aax, trk);
    double target = 0.0, d0 = 0.0, d1 = 1.0;
    if (P.axis_bc == ES_AXIS_KINK) target = P.bc_const_raw * X.outer;                  // P(r_ax) = c xi_e, CF:795
    else if (P.axis_bc == ES_AXIS_ROTATION_KINK) target = -(P.bc_const_raw * X.outer);  // CR-KF:695-698
    else { d0 = Aax.a12; d1 = -Aax.a11; }                                              // P'(r_ax) = 0, CD-C:1082-1085
    // (1) columns e = (1, 0) and d to the boundary: steps of -h over the same node and mid-point entries
    double p1 = 1.0, x1 = 0.0, p2 = d0, x2 = d1;
    Coef A0 = Aax;
    for (int j = nsteps - 1; j >= 0; --j) {
      Coef Am, A1;
      load_base<FAM>(P, 2 * j + 1, b);
      make_entry<FAM>(b, s, e);
      load_base<FAM>(P, 2 * j, b);
      make_entry<FAM>(b, s, e2);
      coefficients2<FAM>(e, e2, P, s, w, Am, A1, trk);
      rk4_step_forward<DIAG>(p1, x1, A0, Am, A1, -h, -h2, -h6, -h3);
      rk4_step_forward<DIAG>(p2, x2, A0, Am, A1, -h, -h2, -h6, -h3);
      A0 = A1;
    }
    const double beta = (X.yb - target * p1) / p2;                                     // P(r_b) = P_b
    // (2) the axis state marched out again, reducing every node
    u = target + beta * d0;
    v = beta * d1;
    A0 = Aax;
    reduce(nsteps, e);
    for (int j = nsteps - 1; j >= 0; --j) {
      Coef Am, A1;
      load_base<FAM>(P, 2 * j + 1, b);
      make_entry<FAM>(b, s, e);
      load_base<FAM>(P, 2 * j, b);
      make_entry<FAM>(b, s, e2);
      coefficients2<FAM>(e, e2, P, s, w, Am, A1, trk);
      rk4_step_forward<DIAG>(u, v, A0, Am, A1, -h, -h2, -h6, -h3);
      A0 = A1;
      reduce(j, e2);
    }
  } else {
    // (1) adjoint march: the row of the transfer matrix picked by the far-end condition -> boundary state (u_b, v_b)
    load_base<FAM>(P, 2 * nsteps, b);
    make_entry<FAM, fam_scaled<FAM>()>(b, s, e);
    Coef B0;
    coefficients<FAM>(e, P, s, w, B0, trk);
    double zp, zq;
    adjoint_start(P, B0, zp, zq);
    for (int j = nsteps - 1; j >= 0; --j) {
      Coef Bm, B1;
      load_base<FAM>(P, 2 * j + 1, b);
      make_entry<FAM, fam_scaled<FAM>()>(b, s, e);
      load_base<FAM>(P, 2 * j, b);
      make_entry<FAM, fam_scaled<FAM>()>(b, s, e2);
      coefficients2<FAM>(e, e2, P, s, w, Bm, B1, trk);
      adjoint_step_normalised<FAM>(zp, zq, B0, Bm, B1, h, h2, h6, h3);      // z at its true scale
      B0 = B1;
    }
    // boundary state from the same algebra as the determinant
    if (FAM == FAM_SLABD) {
      u = X.yb;
      v = (P.slab_sign - zp) * u / zq;         // v = F Vx' ; P_T = v / w
      flux_scale = 1.0 / w;
    } else {
      const double Omb = w - e2[0];
      u = X.yb * Omb / X.Oe;
      v = (P.slab_sign - zp) * u / zq;         // v = Vx' ; P_T = P_Ti(x) v
    }
    // (2) forward march from the boundary, reducing every node
    load_base<FAM>(P, 0, b);
    make_entry<FAM>(b, s, e);
    Coef A0;
    coefficients<FAM>(e, P, s, w, A0, trk);
    reduce(0, e);
    for (int j = 0; j < nsteps; ++j) {
      Coef Am, A1;
      load_base<FAM>(P, 2 * j + 1, b);
      make_entry<FAM>(b, s, e);
      load_base<FAM>(P, 2 * j + 2, b);
      make_entry<FAM>(b, s, e2);
      coefficients2<FAM>(e, e2, P, s, w, Am, A1, trk);
      rk4_step_forward<DIAG>(u, v, A0, Am, A1, h, h2, h6, h3);
      A0 = A1;
      reduce(j + 1, e2);
    }
  }
  if (!in) return;
  // one store per output and lane, lane i at entry i
  if (nodes_value) nodes_value[i] = ok ? tv.changes : -1;
  if (nodes_flux) nodes_flux[i] = ok ? tf.changes : -1;
  if (peak_node_value) peak_node_value[i] = ok ? tv.node : -1;
  if (peak_node_flux) peak_node_flux[i] = ok ? tf.node : -1;
  if (peak_value) peak_value[i] = (ok && tv.node >= 0) ? tv.peak : NAN;
  if (peak_flux) peak_flux[i] = (ok && tf.node >= 0) ? tf.peak : NAN;
  if (status) status[i] = (uint8_t)X.status;
}

template <int FAM>
int launch_signature(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                     const int32_t* d_count, int32_t* nv, int32_t* nf, int32_t* pnv, int32_t* pnf, double* pv, double* pf,
                     uint8_t* st) {
  hipLaunchKernelGGL((mode_signature_kernel<FAM>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, d_k, d_w, n,
                     d_count, nv, nf, pnv, pnf, pv, pf, st);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

}  // namespace

extern "C" int es_shoot_mode_signature(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                                       const int32_t* d_count, int32_t* d_nodes_value, int32_t* d_nodes_flux,
                                       int32_t* d_peak_node_value, int32_t* d_peak_node_flux, double* d_peak_value,
                                       double* d_peak_flux, uint8_t* d_status) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, n >= 0, "negative size");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
#define ES_SIG(F) launch_signature<F>(ctx, prob, d_k, d_w, n, d_count, d_nodes_value, d_nodes_flux, d_peak_node_value, \
                                      d_peak_node_flux, d_peak_value, d_peak_flux, d_status)
  switch (prob->dev.family) {
    case FAM_CYL0: return ES_SIG(FAM_CYL0);
    case FAM_CYLT: return ES_SIG(FAM_CYLT);
    case FAM_SLABD: return ES_SIG(FAM_SLABD);
    case FAM_SLABF: return ES_SIG(FAM_SLABF);
    default: return ES_ERR_UNSUPPORTED;
  }
#undef ES_SIG
}
