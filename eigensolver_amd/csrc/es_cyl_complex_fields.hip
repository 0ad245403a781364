// K16b: perturbation fields of an unstable cylinder mode, ready for VTK (include/eigensolver_amd.h section 16): section 7 at
// complex frequency.  The CPU restatement is tests/cyl_complex_eigen_model.py.
//   es_cyl_complex_polarisation     the amplitude text of es_cyl_field_text.hpp at the complex scalar: omega, P and xi_r of
//                                   es_cyl_complex_eigenfunction -> seven complex amplitudes; one lane per (mode, radial point)
//   es_cyl_complex_field_synthesis  complex amplitudes of one mode -> float32 frames [t][variable][z][theta][r] of
//                                   Re[A Theta e^{i (k z - w t)}], the growth factor e^{Im w t} included; bound by store
//                                   bandwidth.  Angular tables and mesh points are those of section 7 (field_tables_kernel,
//                                   field_points_kernel), the (z, t) table is zt_tables<true> of es_field_shared.hpp.
#include "es_cyl_field_text.hpp"

namespace {

__global__ __launch_bounds__(256) void cyleig_polarisation_kernel(PolArgs a) { polarisation_point<esb::cz>(a); }

// One wave per workgroup; lane l owns the four radial columns c0 + 4 l .. c0 + 4 l + 3 of a 256-column chunk and keeps their
// 7 x 4 complex amplitudes in registers (112 VGPRs: one wave per SIMD).  Grid, loop order and stores are those of
// field_synthesis_kernel (es_fields.hip).  With EC = e^{w_im t} cos(k z - w_re t), ES = e^{w_im t} sin(k z - w_re t) and the
// angular factor Theta of a variable its value is A_re (Theta EC) - A_im (Theta ES): at w_im = 0 and A_im = 0 the expression
// of section 7, grouping included.  tab: 2 n_z n_t doubles of zt_tables<true>, then the 4 n_theta angular doubles.
template <bool SWAP>
__global__ __launch_bounds__(64) void cyleig_field_synthesis_kernel(const double* __restrict__ amp, int n_r, int n_theta,
                                                                   int n_z, int n_t, const double* __restrict__ tab,
                                                                   uint32_t mask, int n_sel, double v_scale,
                                                                   int z_ref_angle, int theta_chunk, float* __restrict__ out) {
  const int col = (int)blockIdx.x * 256 + (int)threadIdx.x * 4;
  int ncol = n_r - col;                                // live columns of this lane: <= 0 none, >= 4 all
  if (ncol > 4) ncol = 4;
  double Ar[ES_AMP_COUNT][4], Ai[ES_AMP_COUNT][4];
#pragma unroll
  for (int c = 0; c < ES_AMP_COUNT; ++c) {
    const double s = (c >= ES_AMP_V_R) ? v_scale : 1.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t o = 2 * ((size_t)c * n_r + col + e);
      Ar[c][e] = (e < ncol) ? amp[o] * s : 0.0;
      Ai[c][e] = (e < ncol) ? amp[o + 1] * s : 0.0;
    }
  }
  const size_t n_zt = (size_t)n_z * n_t;
  const double* ECt = tab;
  const double* ESt = tab + n_zt;
  const double* cm = tab + 2 * n_zt;
  const double* sm = cm + n_theta;
  const double* c1 = cm + 2 * (size_t)n_theta;
  const double* s1 = cm + 3 * (size_t)n_theta;
  const int j0 = (int)blockIdx.z * theta_chunk;
  const int j1 = (j0 + theta_chunk < n_theta) ? j0 + theta_chunk : n_theta;
  for (size_t zt = blockIdx.y; zt < n_zt; zt += gridDim.y) {
    const size_t tau = zt / n_z, l = zt - tau * n_z;
    const double EC = ECt[zt], ES = ESt[zt];
    int slot = 0;
    // variable outer, theta rows inner (field_synthesis_kernel says why)
#pragma unroll
    for (int v = 0; v < ES_VAR_COUNT; ++v) {
      if (!((mask >> v) & 1u)) continue;
      const size_t row0 = ((tau * n_sel + slot) * n_z + l) * n_theta;
      ++slot;
      for (int j = j0; j < j1; ++j) {
        const double fc = cm[j] * EC, gc = cm[j] * ES;     // cos(m theta) {EC, ES}
        const double fs = -sm[j] * EC, gs = -sm[j] * ES;   // -sin(m theta) {EC, ES}
        const double fz = z_ref_angle ? fs : fc, gz = z_ref_angle ? gs : gc;
        const double ct = c1[j], st = s1[j];
#define ES_RE(C, F, G) (Ar[C][e] * (F) - Ai[C][e] * (G))
        double val[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          switch (v) {
            case ES_VAR_XI_R: val[e] = ES_RE(ES_AMP_XI_R, fc, gc); break;
            case ES_VAR_XI_PHI: val[e] = ES_RE(ES_AMP_XI_PHI, fs, gs); break;
            case ES_VAR_P_T: val[e] = ES_RE(ES_AMP_P_T, fc, gc); break;
            case ES_VAR_V_R: val[e] = ES_RE(ES_AMP_V_R, fc, gc); break;
            case ES_VAR_V_PHI: val[e] = ES_RE(ES_AMP_V_PHI, fs, gs); break;
            case ES_VAR_XI_X: val[e] = ES_RE(ES_AMP_XI_R, fc, gc) * ct - ES_RE(ES_AMP_XI_PHI, fs, gs) * st; break;
            case ES_VAR_XI_Y: val[e] = ES_RE(ES_AMP_XI_R, fc, gc) * st + ES_RE(ES_AMP_XI_PHI, fs, gs) * ct; break;
            case ES_VAR_V_X: val[e] = ES_RE(ES_AMP_V_R, fc, gc) * ct - ES_RE(ES_AMP_V_PHI, fs, gs) * st; break;
            case ES_VAR_V_Y: val[e] = ES_RE(ES_AMP_V_R, fc, gc) * st + ES_RE(ES_AMP_V_PHI, fs, gs) * ct; break;
            case ES_VAR_V_Z: val[e] = ES_RE(ES_AMP_V_Z, fz, gz); break;
            default: val[e] = ES_RE(ES_AMP_XI_Z, fz, gz); break;
          }
        }
#undef ES_RE
        float* dst = out + (row0 + j) * (size_t)n_r + col;
        if (ncol <= 0) continue;
        // col is a multiple of 4: the lane's address is 16-byte aligned iff the row's is (uniform over the wave)
        if (ncol == 4 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
          float4 q;
          q.x = to_f32(val[0], SWAP); q.y = to_f32(val[1], SWAP); q.z = to_f32(val[2], SWAP); q.w = to_f32(val[3], SWAP);
          *reinterpret_cast<float4*>(dst) = q;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < ncol) dst[e] = to_f32(val[e], SWAP);
        }
      }
    }
  }
}

}  // namespace

extern "C" int es_cyl_complex_polarisation(es_context* ctx, const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                                           int n_nodes, const double* d_int_value, const double* d_int_flux, int n_ext,
                                           const double* d_ext_x, const double* d_ext_value, const double* d_ext_flux,
                                           const es_field_profiles* pr, int m, double rho_e, double vA_e, double c_e,
                                           double cT_e, int flags, double* d_radius, double* d_amp) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  PolArgs a;
  unsigned blocks;
  bool none;
  const int rc = polarisation_args(ctx, d_k, d_w_re, n, n_nodes, d_int_value, d_int_flux, n_ext, d_ext_x, d_ext_value,
                                   d_ext_flux, pr, m, rho_e, vA_e, c_e, cT_e, flags, d_radius, d_amp, a, blocks, none);
  if (rc || none) return rc;
  ES_REQUIRE(ctx, d_w_im != nullptr, "null pointer");
  a.w_im = d_w_im;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cyleig_polarisation_kernel, dim3(blocks), dim3(256), 0, ctx->stream, a);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_cyl_complex_field_synthesis(es_context* ctx, const double* d_radius, const double* d_amp, int n_r, int m,
                                              double k, double w_re, double w_im, const double* d_theta, int n_theta,
                                              const double* d_z, int n_z, const double* d_t, int n_t, uint32_t var_mask,
                                              double v_scale, int flags, float* d_points, float* d_out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  bool none;
  int rc = synthesis_args(ctx, d_radius, d_amp, n_r, m, d_theta, n_theta, d_z, n_z, d_t, n_t, var_mask, flags, d_points, d_out,
                          none);
  if (rc || none) return rc;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t n_zt = (size_t)n_z * n_t;
  // one scratch block: the (z, t) table first, where zt_tables puts it, the angular tables behind it
  rc = es_ensure_scratch(ctx, (2 * n_zt + 4 * (size_t)n_theta) * sizeof(double));
  if (rc) return rc;
  double* tab = static_cast<double*>(ctx->d_scratch);
  if (n_zt > 0) {
    rc = zt_tables<true>(ctx, d_z, n_z, d_t, n_t, k, w_re, w_im, &tab);
    if (rc) return rc;
  }
  double* ang = tab + 2 * n_zt;
  hipLaunchKernelGGL(field_tables_kernel, dim3((unsigned)((n_theta + 255) / 256)), dim3(256), 0, ctx->stream, d_theta, n_theta,
                     d_z, 0, d_t, 0, (double)m, k, w_re, ang);            // n_z = n_t = 0: the angular part alone
  ES_HIP_CHECK(ctx, hipGetLastError());
  const bool swap = (flags & ES_FIELD_BIG_ENDIAN) != 0;
  if (d_points) {
    rc = field_points(ctx, d_radius, n_r, n_theta, d_z, n_z, ang, swap, d_points);
    if (rc) return rc;
  }
  if (n_t == 0) return ES_SUCCESS;
  const int n_sel = __builtin_popcount(var_mask);
  SynthesisGrid G;
  rc = synthesis_grid(ctx, n_r, n_theta, n_zt, G);
  if (rc) return rc;
  const int zref = (flags & ES_FIELD_Z_REFERENCE_ANGLE) ? 1 : 0;
  if (swap)
    hipLaunchKernelGGL(cyleig_field_synthesis_kernel<true>, G.grid, dim3(64), 0, ctx->stream, d_amp, n_r, n_theta, n_z, n_t, tab,
                       var_mask, n_sel, v_scale, zref, G.theta_chunk, d_out);
  else
    hipLaunchKernelGGL(cyleig_field_synthesis_kernel<false>, G.grid, dim3(64), 0, ctx->stream, d_amp, n_r, n_theta, n_z, n_t, tab,
                       var_mask, n_sel, v_scale, zref, G.theta_chunk, d_out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
