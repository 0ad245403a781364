// Perturbation fields of a cylinder mode, ready for VTK (include/eigensolver_amd.h section 7): what the reference's movie /
// vtk export scripts do after the eigenfunction solve (Cylinder/Non-uniform density/Coronal/Movies/Export_vtk.py:764-818
// amplitudes, :930-950 the four-deep mesh loop; the same expressions in Gaussian_flow_export_vtk.py:796-852 and
// v01_p1_kink_export_vtk.py:2179-2238).
//   es_cyl_polarisation     (P, xi_r) of es_shoot_eigenfunction -> xi_r, xi_phi, xi_z, P_T, v_r, v_phi, v_z on the radial
//                           grid spatial = concatenate(ix[::-1], lx[::-1]); one lane per (mode, radial point)
//   es_cyl_field_synthesis  amplitudes of one mode -> float32 frames [t][variable][z][theta][r]; bound by store bandwidth
// Four oddities of the reference that the interface leaves to the caller:
//   1. q of the first term of xi_z is the constant c_i0^2/(c_i0^2 + vA_i0^2), not the local ratio   -> profile array q
//   2. s_z is d(v_z/r)/dr (Export_vtk.py:812-813), not dv_z/dr                                       -> profile array s_z
//   3. the exterior xi_z carries a factor omega^2 the interior expression does not                   -> ES_FIELD_REFERENCE
//   4. the z-components get the angular factor -sin(m theta) (:940)                          -> ES_FIELD_Z_REFERENCE_ANGLE
// The density perturbation of the scripts is not computed (step of np.gradient that is not the grid's, division by
// time[t]: :854-863, :950).
// The amplitude formulas, the angular tables, the mesh points and the argument checks are the text of es_cyl_field_text.hpp,
// shared with the complex-frequency calls of es_cyl_complex_fields.hip (section 16).
#include "es_cyl_field_text.hpp"

namespace {

// (P, xi_r) -> seven amplitudes: the text of es_cyl_field_text.hpp at the real scalar
__global__ __launch_bounds__(256) void polarisation_kernel(PolArgs a) { polarisation_point<double>(a); }

// ---- amplitudes -> frames -------------------------------------------------------------------------------------------
// One wave per workgroup; lane l owns the four radial columns c0 + 4 l .. c0 + 4 l + 3 of a 256-column chunk and keeps
// their amplitudes in registers.  blockIdx.y walks the (z, t) pairs, blockIdx.z chunks of theta rows; every row of every
// selected variable (variable outer, row inner) is one 16-byte store per lane when the row starts on a 16-byte boundary
// (always, when n_r is a multiple of 4 and the buffer is aligned), four 4-byte stores otherwise.  Nothing is read back.
template <bool SWAP>
__global__ __launch_bounds__(64) void field_synthesis_kernel(const double* __restrict__ amp, int n_r, int n_theta, int n_z,
                                                            int n_t, const double* __restrict__ tab, uint32_t mask,
                                                            int n_sel, double v_scale, int z_ref_angle, int theta_chunk,
                                                            float* __restrict__ out) {
  const int col = (int)blockIdx.x * 256 + (int)threadIdx.x * 4;
  int ncol = n_r - col;                                // live columns of this lane: <= 0 none, >= 4 all
  if (ncol > 4) ncol = 4;
  double A[ES_AMP_COUNT][4];
#pragma unroll
  for (int c = 0; c < ES_AMP_COUNT; ++c) {
    const double s = (c >= ES_AMP_V_R) ? v_scale : 1.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) A[c][e] = (e < ncol) ? amp[(size_t)c * n_r + col + e] * s : 0.0;
  }
  const double* cm = tab;
  const double* sm = tab + n_theta;
  const double* c1 = tab + 2 * (size_t)n_theta;
  const double* s1 = tab + 3 * (size_t)n_theta;
  const double* Czt = tab + 4 * (size_t)n_theta;
  const int j0 = (int)blockIdx.z * theta_chunk;
  const int j1 = (j0 + theta_chunk < n_theta) ? j0 + theta_chunk : n_theta;
  const size_t n_zt = (size_t)n_z * n_t;
  for (size_t zt = blockIdx.y; zt < n_zt; zt += gridDim.y) {
    const size_t tau = zt / n_z, l = zt - tau * n_z;
    const double C = Czt[zt];
    int slot = 0;
    // variable outer, theta rows inner: consecutive stores of a wave go to consecutive rows of one variable, and the
    // waves of the neighbouring column chunks fill the same rows, so the stream into each variable's plane is contiguous
#pragma unroll
    for (int v = 0; v < ES_VAR_COUNT; ++v) {
      if (!((mask >> v) & 1u)) continue;
      const size_t row0 = ((tau * n_sel + slot) * n_z + l) * n_theta;
      ++slot;
      for (int j = j0; j < j1; ++j) {
        const double fc = cm[j] * C;                   // cos(m theta) cos(k z - w t)
        const double fs = -sm[j] * C;                  // -sin(m theta) cos(k z - w t)
        const double fz = z_ref_angle ? fs : fc;
        const double ct = c1[j], st = s1[j];
        double val[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          switch (v) {
            case ES_VAR_XI_R: val[e] = A[ES_AMP_XI_R][e] * fc; break;
            case ES_VAR_XI_PHI: val[e] = A[ES_AMP_XI_PHI][e] * fs; break;
            case ES_VAR_P_T: val[e] = A[ES_AMP_P_T][e] * fc; break;
            case ES_VAR_V_R: val[e] = A[ES_AMP_V_R][e] * fc; break;
            case ES_VAR_V_PHI: val[e] = A[ES_AMP_V_PHI][e] * fs; break;
            case ES_VAR_XI_X: val[e] = (A[ES_AMP_XI_R][e] * fc) * ct - (A[ES_AMP_XI_PHI][e] * fs) * st; break;
            case ES_VAR_XI_Y: val[e] = (A[ES_AMP_XI_R][e] * fc) * st + (A[ES_AMP_XI_PHI][e] * fs) * ct; break;
            case ES_VAR_V_X: val[e] = (A[ES_AMP_V_R][e] * fc) * ct - (A[ES_AMP_V_PHI][e] * fs) * st; break;
            case ES_VAR_V_Y: val[e] = (A[ES_AMP_V_R][e] * fc) * st + (A[ES_AMP_V_PHI][e] * fs) * ct; break;
            case ES_VAR_V_Z: val[e] = A[ES_AMP_V_Z][e] * fz; break;
            default: val[e] = A[ES_AMP_XI_Z][e] * fz; break;
          }
        }
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

extern "C" int es_cyl_polarisation(es_context* ctx, const double* d_k, const double* d_w, int n, int n_nodes,
                                   const double* d_int_value, const double* d_int_flux, int n_ext,
                                   const double* d_ext_x, const double* d_ext_value, const double* d_ext_flux,
                                   const es_field_profiles* pr, int m, double rho_e, double vA_e, double c_e,
                                   double cT_e, int flags, double* d_radius, double* d_amp) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  PolArgs a;
  unsigned blocks;
  bool none;
  const int rc = polarisation_args(ctx, d_k, d_w, n, n_nodes, d_int_value, d_int_flux, n_ext, d_ext_x, d_ext_value, d_ext_flux,
                                   pr, m, rho_e, vA_e, c_e, cT_e, flags, d_radius, d_amp, a, blocks, none);
  if (rc || none) return rc;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(polarisation_kernel, dim3(blocks), dim3(256), 0, ctx->stream, a);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_cyl_field_synthesis(es_context* ctx, const double* d_radius, const double* d_amp, int n_r, int m,
                                      double k, double w, const double* d_theta, int n_theta, const double* d_z,
                                      int n_z, const double* d_t, int n_t, uint32_t var_mask, double v_scale, int flags,
                                      float* d_points, float* d_out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  bool none;
  int rc = synthesis_args(ctx, d_radius, d_amp, n_r, m, d_theta, n_theta, d_z, n_z, d_t, n_t, var_mask, flags, d_points, d_out,
                          none);
  if (rc || none) return rc;
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t n_zt = (size_t)n_z * n_t;
  const size_t ntab = 4 * (size_t)n_theta + n_zt;
  rc = es_ensure_scratch(ctx, ntab * sizeof(double));
  if (rc) return rc;
  double* tab = static_cast<double*>(ctx->d_scratch);
  const size_t nmax = (size_t)n_theta > n_zt ? (size_t)n_theta : n_zt;
  hipLaunchKernelGGL(field_tables_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, ctx->stream, d_theta,
                     n_theta, d_z, n_z, d_t, n_t, (double)m, k, w, tab);
  ES_HIP_CHECK(ctx, hipGetLastError());
  const bool swap = (flags & ES_FIELD_BIG_ENDIAN) != 0;
  if (d_points) {
    rc = field_points(ctx, d_radius, n_r, n_theta, d_z, n_z, tab, swap, d_points);
    if (rc) return rc;
  }
  if (n_t == 0) return ES_SUCCESS;
  const int n_sel = __builtin_popcount(var_mask);
  SynthesisGrid G;
  rc = synthesis_grid(ctx, n_r, n_theta, n_zt, G);
  if (rc) return rc;
  const int zref = (flags & ES_FIELD_Z_REFERENCE_ANGLE) ? 1 : 0;
  if (swap)
    hipLaunchKernelGGL(field_synthesis_kernel<true>, G.grid, dim3(64), 0, ctx->stream, d_amp, n_r, n_theta, n_z, n_t, tab,
                       var_mask, n_sel, v_scale, zref, G.theta_chunk, d_out);
  else
    hipLaunchKernelGGL(field_synthesis_kernel<false>, G.grid, dim3(64), 0, ctx->stream, d_amp, n_r, n_theta, n_z, n_t, tab,
                       var_mask, n_sel, v_scale, zref, G.theta_chunk, d_out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
