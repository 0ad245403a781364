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
#include "es_field_shared.hpp"

namespace {

// ---- (P, xi_r) -> seven amplitudes ----------------------------------------------------------------------------------
struct PolArgs {
  const double* k; const double* w;
  const double* iv; const double* ifl;                 // interior value / flux, n x N, node 0 = boundary
  const double* ex; const double* ev; const double* ef; // exterior x / value / flux, n x n_ext, far field -> boundary
  es_field_profiles p;
  int n, N, n_ext, m, flags;
  double rho_e, vAe2, ce2, cTe2;
  double* radius; double* amp;
};

__global__ __launch_bounds__(256) void polarisation_kernel(PolArgs a) {
  const size_t n_r = (size_t)a.N + (size_t)a.n_ext;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)a.n * n_r) return;
  const size_t i = t / n_r;
  const int j = (int)(t - i * n_r);
  const double k = a.k[i], w = a.w[i], dm = (double)a.m;
  double r, xi_r, xi_phi, xi_z, P, v_r, v_phi, v_z;
  if (j < a.N) {
    const int node = a.N - 1 - j;                       // ix[::-1]: from the axis node out to the boundary
    const size_t o = i * (size_t)a.N + node;
    P = a.iv[o]; xi_r = a.ifl[o];
    r = a.p.r[node];
    const double rho = a.p.rho[node], Bz = a.p.Bz[node], Bphi = a.p.Bphi[node], vz = a.p.vz[node],
                 vphi = a.p.vphi[node];
    const double Om = w - dm * vphi / r - k * vz;       // shift_freq, Export_vtk.py:617-618
    const double Om2 = Om * Om;
    const double mB = dm * Bphi / r;
    const double f = mB + k * Bz;                       // f_B, :606-607
    const double g = dm * Bz / r + k * Bphi;            // g_B, :611-612
    const double wA = fma(k, a.p.bA[node], mB);         // the determinant's node entry (make_entry)
    const double wA2 = wA * wA;
    const double wc2 = wA2 * a.p.qc[node];
    const double tA = Om2 - wA2, tc = Om2 - wc2;
    const double T = f * Bphi + rho * vphi * Om;        // :642-643
    const double Q = -tA * rho * (vphi * vphi) / r + 2.0 * Om2 * (Bphi * Bphi) / r + 2.0 * Om * Bphi * vphi * f / r;  // :637-638
    const double xr = xi_r / r;
    const double num = g * P - 2.0 * Bz * T * xr;
    xi_z = (f * a.p.q[node] * (Om2 * P - Q * xi_r) / (Om2 * rho * tc) - (2.0 * Om * vphi * Bphi + f * (vphi * vphi)) * xr -
            Bphi * num / (Bz * rho * tA)) /
           (Bphi * Bphi / Bz + Bz);                     // :780
    xi_phi = (num / (rho * tA) + Bphi * xi_z) / Bz;     // :786
    v_r = -Om * xi_r;                                   // :767
    v_phi = -(Om * xi_phi) - a.p.s_phi[node] * r * xi_r;   // :804
    v_z = -(Om * xi_z) - a.p.s_z[node] * xi_r;          // :818
  } else {
    const int je = a.n_ext - 1 - (j - a.N);             // lx[::-1]: from the boundary out to the far field
    const size_t o = i * (size_t)a.n_ext + je;
    P = a.ev[o]; xi_r = a.ef[o];
    r = a.ex[o];
    const double w2 = w * w, k2 = k * k;
    xi_phi = (dm * P / r) / (a.rho_e * (w2 - k2 * a.vAe2));                                   // :787
    const double wfac = (a.flags & ES_FIELD_REFERENCE) ? w2 : 1.0;
    xi_z = k * a.ce2 * wfac * P / (a.rho_e * (w2 - k2 * a.cTe2) * (a.ce2 + a.vAe2));          // :781
    v_r = -w * xi_r;                                    // :766
    v_phi = -w * xi_phi;                                // :803
    v_z = -w * xi_z;                                    // :817
  }
  a.radius[t] = r;
  double* A = a.amp + i * (size_t)ES_AMP_COUNT * n_r + j;
  A[ES_AMP_XI_R * n_r] = xi_r;
  A[ES_AMP_XI_PHI * n_r] = xi_phi;
  A[ES_AMP_XI_Z * n_r] = xi_z;
  A[ES_AMP_P_T * n_r] = P;
  A[ES_AMP_V_R * n_r] = v_r;
  A[ES_AMP_V_PHI * n_r] = v_phi;
  A[ES_AMP_V_Z * n_r] = v_z;
}

// ---- amplitudes -> frames -------------------------------------------------------------------------------------------
// Trigonometric tables of one call, doubles in the context's scratch: [0, n_theta) cos(m theta), then sin(m theta),
// cos(theta), sin(theta), then cos(k z_l - w t_tau) at [4 n_theta + tau * n_z + l].
__global__ __launch_bounds__(256) void field_tables_kernel(const double* __restrict__ theta, int n_theta,
                                                          const double* __restrict__ z, int n_z,
                                                          const double* __restrict__ tt, int n_t, double dm, double k,
                                                          double w, double* __restrict__ tab) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n_zt = (size_t)n_z * n_t;
  if (i < (size_t)n_theta) {
    const double th = theta[i];
    tab[i] = cos(dm * th);
    tab[(size_t)n_theta + i] = sin(dm * th);
    tab[2 * (size_t)n_theta + i] = cos(th);
    tab[3 * (size_t)n_theta + i] = sin(th);
  }
  if (i < n_zt) {
    const size_t tau = i / n_z, l = i - tau * n_z;
    tab[4 * (size_t)n_theta + i] = cos(k * z[l] - w * tt[tau]);
  }
}

__device__ __forceinline__ float to_f32(double v, bool swap) { return __uint_as_float(f32_bits(v, swap)); }

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

// (r cos(theta), r sin(theta), z) at every mesh point, one float per lane: [z][theta][r][3]
template <bool SWAP>
__global__ __launch_bounds__(256) void field_points_kernel(const double* __restrict__ radius, int n_r, int n_theta,
                                                          const double* __restrict__ z, size_t total,
                                                          const double* __restrict__ tab, float* __restrict__ pts) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t p = i / 3;
  const int c = (int)(i - p * 3);
  const size_t rowi = p / (size_t)n_r;
  const int ir = (int)(p - rowi * (size_t)n_r);
  const size_t l = rowi / (size_t)n_theta;
  const int j = (int)(rowi - l * (size_t)n_theta);
  double v;
  if (c == 0) v = radius[ir] * tab[2 * (size_t)n_theta + j];
  else if (c == 1) v = radius[ir] * tab[3 * (size_t)n_theta + j];
  else v = z[l];
  pts[i] = to_f32(v, SWAP);
}

}  // namespace

extern "C" int es_cyl_polarisation(es_context* ctx, const double* d_k, const double* d_w, int n, int n_nodes,
                                   const double* d_int_value, const double* d_int_flux, int n_ext,
                                   const double* d_ext_x, const double* d_ext_value, const double* d_ext_flux,
                                   const es_field_profiles* pr, int m, double rho_e, double vA_e, double c_e,
                                   double cT_e, int flags, double* d_radius, double* d_amp) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, n >= 0 && n_nodes >= 0 && n_ext >= 0, "negative size");
  ES_REQUIRE(ctx, m >= 0, "m");
  ES_REQUIRE(ctx, (flags & ~ES_FIELD_REFERENCE) == 0, "flags");
  const size_t n_r = (size_t)n_nodes + (size_t)n_ext;
  if (n == 0 || n_r == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w && d_radius && d_amp, "null pointer");
  if (n_nodes > 0) {
    ES_REQUIRE(ctx, d_int_value && d_int_flux, "null interior arrays");
    ES_REQUIRE(ctx, pr != nullptr, "null profiles");
    ES_REQUIRE(ctx, pr->r && pr->rho && pr->Bz && pr->Bphi && pr->vz && pr->vphi && pr->bA && pr->qc && pr->q &&
                        pr->s_phi && pr->s_z, "null profile array");
  }
  ES_REQUIRE(ctx, n_ext == 0 || (d_ext_x && d_ext_value && d_ext_flux), "null exterior arrays");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PolArgs a;
  a.k = d_k; a.w = d_w; a.iv = d_int_value; a.ifl = d_int_flux; a.ex = d_ext_x; a.ev = d_ext_value; a.ef = d_ext_flux;
  if (pr) a.p = *pr; else memset(&a.p, 0, sizeof(a.p));
  a.n = n; a.N = n_nodes; a.n_ext = n_ext; a.m = m; a.flags = flags;
  a.rho_e = rho_e; a.vAe2 = vA_e * vA_e; a.ce2 = c_e * c_e; a.cTe2 = cT_e * cT_e;
  a.radius = d_radius; a.amp = d_amp;
  const size_t tot = (size_t)n * n_r;
  ES_REQUIRE(ctx, (tot + 255) / 256 <= 0x7fffffffull, "too many points");
  hipLaunchKernelGGL(polarisation_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, a);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_cyl_field_synthesis(es_context* ctx, const double* d_radius, const double* d_amp, int n_r, int m,
                                      double k, double w, const double* d_theta, int n_theta, const double* d_z,
                                      int n_z, const double* d_t, int n_t, uint32_t var_mask, double v_scale, int flags,
                                      float* d_points, float* d_out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, n_r >= 0 && n_theta >= 0 && n_z >= 0 && n_t >= 0, "negative size");
  ES_REQUIRE(ctx, m >= 0, "m");
  ES_REQUIRE(ctx, var_mask != 0, "empty variable mask");
  ES_REQUIRE(ctx, (var_mask >> ES_VAR_COUNT) == 0, "unknown variable bit");
  ES_REQUIRE(ctx, (flags & ~(ES_FIELD_Z_REFERENCE_ANGLE | ES_FIELD_BIG_ENDIAN)) == 0, "flags");
  ES_REQUIRE(ctx, (size_t)n_z * (size_t)n_theta * (size_t)(n_t > 0 ? n_t : 1) < 0x7fffffffull, "mesh too large");
  if (n_r == 0 || n_theta == 0 || n_z == 0) return ES_SUCCESS;
  if (n_t == 0 && !d_points) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_radius && d_amp && d_theta && d_z, "null pointer");
  ES_REQUIRE(ctx, n_t == 0 || (d_t && d_out), "null pointer");
  ES_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_points) & 3u) == 0,
             "float32 outputs need 4-byte alignment");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t n_zt = (size_t)n_z * n_t;
  const size_t ntab = 4 * (size_t)n_theta + n_zt;
  int rc = es_ensure_scratch(ctx, ntab * sizeof(double));
  if (rc) return rc;
  double* tab = static_cast<double*>(ctx->d_scratch);
  const size_t nmax = (size_t)n_theta > n_zt ? (size_t)n_theta : n_zt;
  hipLaunchKernelGGL(field_tables_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, ctx->stream, d_theta,
                     n_theta, d_z, n_z, d_t, n_t, (double)m, k, w, tab);
  ES_HIP_CHECK(ctx, hipGetLastError());
  const bool swap = (flags & ES_FIELD_BIG_ENDIAN) != 0;
  if (d_points) {
    const size_t total = (size_t)n_z * n_theta * n_r * 3;
    ES_REQUIRE(ctx, (total + 255) / 256 <= 0x7fffffffull, "mesh too large");
    const dim3 g((unsigned)((total + 255) / 256));
    if (swap)
      hipLaunchKernelGGL(field_points_kernel<true>, g, dim3(256), 0, ctx->stream, d_radius, n_r, n_theta, d_z, total, tab,
                         d_points);
    else
      hipLaunchKernelGGL(field_points_kernel<false>, g, dim3(256), 0, ctx->stream, d_radius, n_r, n_theta, d_z, total, tab,
                         d_points);
    ES_HIP_CHECK(ctx, hipGetLastError());
  }
  if (n_t == 0) return ES_SUCCESS;
  const int n_sel = __builtin_popcount(var_mask);
  // workgroups over (column chunk, (z, t) pair, chunk of theta rows): enough waves for every CU to stream (about 16 per CU)
  const unsigned gx = (unsigned)((n_r + 255) / 256);
  const unsigned gy = (unsigned)(n_zt < 65535 ? n_zt : 65535);
  const size_t want = 4096;
  size_t parts = (want + (size_t)gx * gy - 1) / ((size_t)gx * gy);
  if (parts > (size_t)n_theta) parts = (size_t)n_theta;
  if (parts < 1) parts = 1;
  const int theta_chunk = (int)(((size_t)n_theta + parts - 1) / parts);
  const unsigned gz = (unsigned)((n_theta + theta_chunk - 1) / theta_chunk);
  ES_REQUIRE(ctx, gz <= 65535, "n_theta too large");
  const int zref = (flags & ES_FIELD_Z_REFERENCE_ANGLE) ? 1 : 0;
  if (swap)
    hipLaunchKernelGGL(field_synthesis_kernel<true>, dim3(gx, gy, gz), dim3(64), 0, ctx->stream, d_amp, n_r, n_theta, n_z,
                       n_t, tab, var_mask, n_sel, v_scale, zref, theta_chunk, d_out);
  else
    hipLaunchKernelGGL(field_synthesis_kernel<false>, dim3(gx, gy, gz), dim3(64), 0, ctx->stream, d_amp, n_r, n_theta, n_z,
                       n_t, tab, var_mask, n_sel, v_scale, zref, theta_chunk, d_out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
