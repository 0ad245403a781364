// What the two polar field translation units of the cylinder share (es_fields.hip: section 7, a real mode;
// es_cyl_complex_fields.hip: section 16, an unstable mode at complex frequency): the amplitude formulas, ONE text over the
// scalar S of omega, P and xi_r (double, or esb::cz with its arrays as interleaved (re, im) pairs), the angular tables and the
// mesh points.  Everything is in the unnamed namespace and force-inlined or a kernel of its own, so each unit compiles as if
// the text stood in its own file.
#pragma once
#include "es_bessel_complex.hpp"
#include "es_field_shared.hpp"

namespace {

// ---- (P, xi_r) -> seven amplitudes ----------------------------------------------------------------------------------
struct PolArgs {
  const double* k; const double* w;                    // w: omega, or Re omega with w_im
  const double* w_im;                                  // complex scalar only
  const double* iv; const double* ifl;                 // interior value / flux, n x N, node 0 = boundary
  const double* ex; const double* ev; const double* ef; // exterior x / value / flux, n x n_ext, far field -> boundary
  es_field_profiles p;
  int n, N, n_ext, m, flags;
  double rho_e, vAe2, ce2, cTe2;
  double* radius; double* amp;
};

// how an array of the scalar S lies in memory
__device__ __forceinline__ void field_load(const double* a, size_t o, double& v) { v = a[o]; }
__device__ __forceinline__ void field_load(const double* a, size_t o, esb::cz& v) { v = esb::cz(a[2 * o], a[2 * o + 1]); }
__device__ __forceinline__ void field_store(double* a, size_t o, double v) { a[o] = v; }
__device__ __forceinline__ void field_store(double* a, size_t o, esb::cz v) { a[2 * o] = v.re; a[2 * o + 1] = v.im; }
__device__ __forceinline__ void field_omega(const PolArgs& a, size_t i, double& w) { w = a.w[i]; }
__device__ __forceinline__ void field_omega(const PolArgs& a, size_t i, esb::cz& w) { w = esb::cz(a.w[i], a.w_im[i]); }

// one lane per (mode, radial point); the amplitudes of S = esb::cz are the analytic continuation in omega of those of
// S = double: the same expressions, no factor of i between the channels
template <class S>
__device__ __forceinline__ void polarisation_point(const PolArgs& a) {
  const size_t n_r = (size_t)a.N + (size_t)a.n_ext;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)a.n * n_r) return;
  const size_t i = t / n_r;
  const int j = (int)(t - i * n_r);
  const double k = a.k[i], dm = (double)a.m;
  S w;
  field_omega(a, i, w);
  double r;
  S xi_r, xi_phi, xi_z, P, v_r, v_phi, v_z;
  if (j < a.N) {
    const int node = a.N - 1 - j;                       // ix[::-1]: from the axis node out to the boundary
    const size_t o = i * (size_t)a.N + node;
    field_load(a.iv, o, P); field_load(a.ifl, o, xi_r);
    r = a.p.r[node];
    const double rho = a.p.rho[node], Bz = a.p.Bz[node], Bphi = a.p.Bphi[node], vz = a.p.vz[node],
                 vphi = a.p.vphi[node];
    const S Om = w - dm * vphi / r - k * vz;            // shift_freq, Export_vtk.py:617-618
    const S Om2 = Om * Om;
    const double mB = dm * Bphi / r;
    const double f = mB + k * Bz;                       // f_B, :606-607
    const double g = dm * Bz / r + k * Bphi;            // g_B, :611-612
    const double wA = fma(k, a.p.bA[node], mB);         // the determinant's node entry (make_entry)
    const double wA2 = wA * wA;
    const double wc2 = wA2 * a.p.qc[node];
    const S tA = Om2 - wA2, tc = Om2 - wc2;
    const S T = f * Bphi + rho * vphi * Om;             // :642-643
    const S Q = -tA * rho * (vphi * vphi) / r + 2.0 * Om2 * (Bphi * Bphi) / r + 2.0 * Om * Bphi * vphi * f / r;  // :637-638
    const S xr = xi_r / r;
    const S num = g * P - 2.0 * Bz * T * xr;
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
    field_load(a.ev, o, P); field_load(a.ef, o, xi_r);
    r = a.ex[o];
    const S w2 = w * w;
    const double k2 = k * k;
    xi_phi = (dm * P / r) / (a.rho_e * (w2 - k2 * a.vAe2));                                   // :787
    const S wfac = (a.flags & ES_FIELD_REFERENCE) ? w2 : S(1.0);
    xi_z = k * a.ce2 * wfac * P / (a.rho_e * (w2 - k2 * a.cTe2) * (a.ce2 + a.vAe2));          // :781
    v_r = -w * xi_r;                                    // :766
    v_phi = -w * xi_phi;                                // :803
    v_z = -w * xi_z;                                    // :817
  }
  a.radius[t] = r;
  const size_t A = i * (size_t)ES_AMP_COUNT * n_r + j;
  field_store(a.amp, A + ES_AMP_XI_R * n_r, xi_r);
  field_store(a.amp, A + ES_AMP_XI_PHI * n_r, xi_phi);
  field_store(a.amp, A + ES_AMP_XI_Z * n_r, xi_z);
  field_store(a.amp, A + ES_AMP_P_T * n_r, P);
  field_store(a.amp, A + ES_AMP_V_R * n_r, v_r);
  field_store(a.amp, A + ES_AMP_V_PHI * n_r, v_phi);
  field_store(a.amp, A + ES_AMP_V_Z * n_r, v_z);
}

// argument checks and the argument block the two polarisation calls have in common (w_im stays null); *none: nothing to do
inline int polarisation_args(es_context* ctx, const double* d_k, const double* d_w, int n, int n_nodes,
                             const double* d_int_value, const double* d_int_flux, int n_ext, const double* d_ext_x,
                             const double* d_ext_value, const double* d_ext_flux, const es_field_profiles* pr, int m,
                             double rho_e, double vA_e, double c_e, double cT_e, int flags, double* d_radius, double* d_amp,
                             PolArgs& a, unsigned& blocks, bool& none) {
  none = true;
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
  a.k = d_k; a.w = d_w; a.w_im = nullptr; a.iv = d_int_value; a.ifl = d_int_flux; a.ex = d_ext_x; a.ev = d_ext_value;
  a.ef = d_ext_flux;
  if (pr) a.p = *pr; else memset(&a.p, 0, sizeof(a.p));
  a.n = n; a.N = n_nodes; a.n_ext = n_ext; a.m = m; a.flags = flags;
  a.rho_e = rho_e; a.vAe2 = vA_e * vA_e; a.ce2 = c_e * c_e; a.cTe2 = cT_e * cT_e;
  a.radius = d_radius; a.amp = d_amp;
  const size_t tot = (size_t)n * n_r;
  ES_REQUIRE(ctx, (tot + 255) / 256 <= 0x7fffffffull, "too many points");
  blocks = (unsigned)((tot + 255) / 256);
  none = false;
  return ES_SUCCESS;
}

// ---- amplitudes -> frames -------------------------------------------------------------------------------------------
// argument checks the two synthesis calls have in common; *none: nothing to write
inline int synthesis_args(es_context* ctx, const double* d_radius, const double* d_amp, int n_r, int m, const double* d_theta,
                          int n_theta, const double* d_z, int n_z, const double* d_t, int n_t, uint32_t var_mask, int flags,
                          const float* d_points, const float* d_out, bool& none) {
  none = true;
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
  none = false;
  return ES_SUCCESS;
}

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

// the mesh points of one call from the angular tables at `tab`, enqueued on the context's stream
inline int field_points(es_context* ctx, const double* d_radius, int n_r, int n_theta, const double* d_z, int n_z,
                        const double* tab, bool swap, float* d_points) {
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
  return ES_SUCCESS;
}

// Launch shape of a synthesis kernel: workgroups over (column chunk, (z, t) pair, chunk of theta rows), enough waves for every
// CU to stream (about 16 per CU).
struct SynthesisGrid { dim3 grid; int theta_chunk; };
inline int synthesis_grid(es_context* ctx, int n_r, int n_theta, size_t n_zt, SynthesisGrid& G) {
  const unsigned gx = (unsigned)((n_r + 255) / 256);
  const unsigned gy = (unsigned)(n_zt < 65535 ? n_zt : 65535);
  const size_t want = 4096;
  size_t parts = (want + (size_t)gx * gy - 1) / ((size_t)gx * gy);
  if (parts > (size_t)n_theta) parts = (size_t)n_theta;
  if (parts < 1) parts = 1;
  G.theta_chunk = (int)(((size_t)n_theta + parts - 1) / parts);
  const unsigned gz = (unsigned)((n_theta + G.theta_chunk - 1) / G.theta_chunk);
  ES_REQUIRE(ctx, gz <= 65535, "n_theta too large");
  G.grid = dim3(gx, gy, gz);
  return ES_SUCCESS;
}

}  // namespace
