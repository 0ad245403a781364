// Eigenfunctions at given (k, omega): what the reference's analysis scripts recompute at a chosen root
// (analysis_cylinder_flow_coronal.py:813-924).  One (k, omega) pair per lane for the interior, the two RK4 marches of
// interior_rows (es_interior_march.hpp, which says why the cylinder marches run outwards) with every node written;
// one (pair, exterior point) per lane for the closed-form exterior.
// A pair whose exterior is not ES_PT_OK (leaky, non-finite) gets NaN in all four of its value / flux rows.
#include "es_interior_march.hpp"

namespace {
using namespace es_shoot_shared;

template <int FAM>
__global__ __launch_bounds__(64) void eigen_interior_kernel(ShootDev P, const double* __restrict__ kv,
                                                            const double* __restrict__ wv, int n,
                                                            double* __restrict__ val, double* __restrict__ flux) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const double k = in ? kv[i] : 1.0;
  const double w = in ? wv[i] : 1.0;
  const ExteriorLite X = exterior_lite(P, k, w, w);
  const bool ok = X.status == ES_PT_OK;
  interior_rows<FAM>(P, k, w, X, [&](int node, double value, double f) {
    if (!in) return;
    const size_t o = (size_t)i * P.n_nodes + node;
    val[o] = ok ? value : NAN;
    flux[o] = ok ? f : NAN;
  });
}


// exterior: cylinders P = a I_m + b K_m, slabs Vx = a e^{mu x} + b e^{-mu x}; relative to the boundary value (+-1)
__global__ __launch_bounds__(256) void eigen_exterior_kernel(ShootDev P, const double* __restrict__ kv,
                                                             const double* __restrict__ wv, int n, int n_ext,
                                                             double* __restrict__ xs, double* __restrict__ val,
                                                             double* __restrict__ flux) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)n * n_ext) return;
  const int i = (int)(t / n_ext), j = (int)(t - (long)i * n_ext);
  const double k = kv[i], w = wv[i];
  const bool cyl = (P.family == FAM_CYL0 || P.family == FAM_CYLT);
  const Exterior X = cyl ? exterior_cylinder(P, k, w, w) : exterior_slab(P, k, w);
  const double sgn = (P.xb < 0.0) ? -1.0 : 1.0;
  const double R = P.R_factor / k;
  // np.linspace(sgn*R, sgn*1, n_ext)[j]
  const double step = (sgn * 1.0 - sgn * R) / (double)(n_ext - 1);
  const double x = (j == n_ext - 1) ? sgn * 1.0 : sgn * R + (double)j * step;
  double v = NAN, f = NAN;
  if (X.status == ES_PT_OK) {
    const double mu = sqrt(X.m_e);
    const double ax = fabs(x);
    if (cyl) {
      const int m = P.m_ext;
      const double dn = (double)m;
      const double xR = mu * R, xb = mu, xx = mu * ax;
      double KR, KR1, Kb, Kb1, Kx, Kx1, IR, IR1, Ib, Ib1, Ix, Ix1;
      esb::ke_pair(m, xR, KR, KR1); esb::ke_pair(m, xb, Kb, Kb1); esb::ke_pair(m, xx, Kx, Kx1);
      const double dKR = -KR1 + (dn / xR) * KR, dKx = -Kx1 + (dn / xx) * Kx;
      const double g = P.ic1 / (sgn * mu);
      double a_s = 0.0, b_s;
      double Ibv = 0.0, Ixv = 0.0, dIxv = 0.0;
      if (xR - xb < 40.0) {
        esb::ie_pair(m, xR, IR, IR1); esb::ie_pair(m, xb, Ib, Ib1); esb::ie_pair(m, xx, Ix, Ix1);
        const double dIR = IR1 + (dn / xR) * IR;
        a_s = -(P.ic0 * dKR - g * KR);
        b_s = -(g * IR - P.ic0 * dIR);
        Ibv = Ib; Ixv = Ix; dIxv = Ix1 + (dn / xx) * Ix;
      } else {
        const double rI = 1.0 - 0.5 / xR - (4.0 * dn * dn - 1.0) / (8.0 * xR * xR);
        b_s = -(g - P.ic0 * rI);
      }
      const double E2b = exp(-2.0 * (xR - xb)), E2x = exp(-2.0 * (xR - xx));
      const double den = fabs(b_s * Kb + E2b * a_s * Ibv);
      const double dec = exp(-(xx - xb));
      v = dec * (b_s * Kx + E2x * a_s * Ixv) / den;
      const double dv = sgn * mu * dec * (b_s * dKx + E2x * a_s * dIxv) / den;
      f = X.cst * dv;                                          // xi_e = xi_e_const * P'
    } else {
      const double E2x = exp(-2.0 * mu * (R - ax)), E2b = exp(-2.0 * mu * (R - 1.0));
      const double gp = P.ic0 + P.ic1 / mu, gm = P.ic0 - P.ic1 / mu;
      const double den = fabs(gp + E2b * gm);
      const double dec = exp(-mu * (ax - 1.0));
      v = dec * (gp + E2x * gm) / den;
      const double dv = mu * dec * (gp - E2x * gm) / den;
      f = X.cst * dv;                                          // left_P = p_e_const * Vx'
    }
  }
  xs[t] = x;
  val[t] = v;
  flux[t] = f;
}

template <int FAM>
int launch_interior(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n, double* v,
                    double* f) {
  hipLaunchKernelGGL((eigen_interior_kernel<FAM>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, prob->dev, d_k, d_w,
                     n, v, f);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

int dispatch_interior(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n, double* v,
                      double* f) {
#define CALL_INTERIOR(F) launch_interior<F>(ctx, prob, d_k, d_w, n, v, f)
  ES_DISPATCH_FAMILY(prob->dev.family, CALL_INTERIOR)
#undef CALL_INTERIOR
}

}  // namespace

extern "C" int es_shoot_eigenfunction(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w,
                                      int n, double* d_int_value, double* d_int_flux, int n_ext, double* d_ext_x,
                                      double* d_ext_value, double* d_ext_flux) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  ES_REQUIRE(ctx, n >= 0 && n_ext >= 0, "negative size");
  ES_REQUIRE(ctx, n_ext == 0 || n_ext >= 2, "n_ext must be 0 or >= 2");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w && d_int_value && d_int_flux, "null pointer");
  ES_REQUIRE(ctx, n_ext == 0 || (d_ext_x && d_ext_value && d_ext_flux), "null exterior arrays");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rc = dispatch_interior(ctx, prob, d_k, d_w, n, d_int_value, d_int_flux);
  if (rc) return rc;
  if (n_ext > 0) {
    const long tot = (long)n * n_ext;
    hipLaunchKernelGGL(eigen_exterior_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream,
                       prob->dev, d_k, d_w, n, n_ext, d_ext_x, d_ext_value, d_ext_flux);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  return ES_SUCCESS;
}
