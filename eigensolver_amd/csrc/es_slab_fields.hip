// Perturbation fields of a slab mode, real or unstable (include/eigensolver_amd.h section 9): stages three and four for
// the slab families.  The reference stops at the two curves (Vx, P_T) of a root (Slab/Non uniform flow/COMPLEX ANALYSIS/
// complex_imag_flow_analysis.py:1050-1072); here they become displacement, velocity, total pressure and vorticity
// amplitudes and then float32 frames on an (x, z, t) mesh.  Everything is Re[A(x) e^{i (k z - w t)}] with a complex A and
// a complex w: a real mode is the same arithmetic with zero imaginary parts.
//   es_slab_polarisation      (V, Pf) -> xi_x, xi_z, P_T, v_x, v_z on the table left exterior | interior | mirrored right
//                             exterior, one lane per (mode, table point); a second launch differentiates v_z per region
//                             (np.gradient's three-point formulas) for vort_y
//   es_slab_field_synthesis   the table of one mode -> frames [t][variable][z][x]; the x stage (search, interpolation)
//                             once per workgroup, then bound by store bandwidth
#include "es_bessel_complex.hpp"
#include "es_field_shared.hpp"

// workgroups (of one wave) es_slab_field_synthesis asks for; a build flag so that tools can time other values
#ifndef ES_SLAB_SYNTH_WAVES
#define ES_SLAB_SYNTH_WAVES 4096
#endif

namespace {

using esb::cz;
__device__ __forceinline__ cz times_i(cz a) { return cz(-a.im, a.re); }
__device__ __forceinline__ cz times_minus_i(cz a) { return cz(a.im, -a.re); }

// ---- (V, Pf) -> five amplitudes -----------------------------------------------------------------------------------------
struct SlabPolArgs {
  const double* k; const double* w_re; const double* w_im;
  const double* iv; const double* ifl;                 // interior value / flux, n x N (x 2), node 0 = x = -1
  const double* ex; const double* ev; const double* ef; // exterior x / value / flux, n x n_ext (x 2), -R -> -1
  es_slab_field_profiles p;
  int n, N, n_ext, cplx, flags;
  double rho_e, vAe2, ce2, U_e, sigma;
  double* x; double* amp;
};

__global__ __launch_bounds__(256) void slab_field_polarisation_kernel(SlabPolArgs a) {
  const size_t n_tab = (size_t)a.N + 2 * (size_t)a.n_ext;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)a.n * n_tab) return;
  const size_t i = t / n_tab;
  const int j = (int)(t - i * n_tab);
  const double k = a.k[i];
  const cz w(a.w_re[i], a.w_im ? a.w_im[i] : 0.0);
  auto get = [&](const double* p, size_t o) { return a.cplx ? cz(p[2 * o], p[2 * o + 1]) : cz(p[o], 0.0); };
  double x, rho, c2, vA2, U, dU;
  cz V, Pf;
  const bool interior = j >= a.n_ext && j < a.n_ext + a.N;
  if (interior) {
    const int node = j - a.n_ext;
    const size_t o = i * (size_t)a.N + node;
    V = get(a.iv, o); Pf = get(a.ifl, o);
    x = (node == a.N - 1) ? 1.0 : -1.0 + (double)node * (2.0 / (double)(a.N - 1));   // numpy.linspace(-1, 1, N)
    rho = a.p.rho[node]; c2 = a.p.c2[node]; vA2 = a.p.vA2[node]; U = a.p.U[node]; dU = a.p.dU[node];
  } else {
    const bool left = j < a.n_ext;
    const int je = left ? j : a.n_ext - 1 - (j - a.n_ext - a.N);
    const size_t o = i * (size_t)a.n_ext + je;
    V = get(a.ev, o); Pf = get(a.ef, o);
    x = a.ex[o];
    if (!left) {                                       // mirror image: Vx(+x) = sigma Vx(-x), P_T(+x) = -sigma P_T(-x)
      x = -x;
      V = a.sigma * V;
      Pf = (-a.sigma) * Pf;
    }
    rho = a.rho_e; c2 = a.ce2; vA2 = a.vAe2; U = a.U_e; dU = 0.0;
  }
  const double S = c2 + vA2, q = c2 / S, cT2 = c2 * vA2 / S, k2 = k * k;
  const cz Om = w - k * U;
  const cz Om2 = Om * Om;
  const cz tT = Om2 - k2 * cT2;
  if (interior && (a.flags & ES_SLAB_FIELD_SHEAR_PT)) {
    const cz F = (rho * S) * (tT / (Om2 - k2 * c2));
    Pf = Pf + ((F / Om) * ((k * dU) * (V / Om)));
  }
  const cz VoO = V / Om;
  const cz xi_x = times_i(VoO);
  const cz xi_z = ((k * q) * Pf) / (rho * tT);
  const cz v_z = times_minus_i(Om * xi_z + dU * VoO);
  a.x[t] = x;
  double* A = a.amp + (i * (size_t)ES_SAMP_COUNT * n_tab + j) * 2;
  auto put = [&](int c, cz v) { A[(size_t)c * n_tab * 2] = v.re; A[(size_t)c * n_tab * 2 + 1] = v.im; };
  put(ES_SAMP_XI_X, xi_x);
  put(ES_SAMP_XI_Z, xi_z);
  put(ES_SAMP_P_T, times_minus_i(Pf));
  put(ES_SAMP_V_X, V);
  put(ES_SAMP_V_Z, v_z);
}

// vort_y = i k v_x - d(v_z)/dx.  d/dx is np.gradient(a, x, edge_order=2) of each of the three regions on its own
// (gradient_stencil).
__global__ __launch_bounds__(256) void slab_field_vorticity_kernel(const double* __restrict__ xs,
                                                                   double* __restrict__ amp,
                                                                   const double* __restrict__ kk, int n, int N,
                                                                   int n_ext) {
  const size_t n_tab = (size_t)N + 2 * (size_t)n_ext;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * n_tab) return;
  const size_t i = t / n_tab;
  const int j = (int)(t - i * n_tab);
  const int base = (j < n_ext) ? 0 : (j < n_ext + N ? n_ext : n_ext + N);
  const int len = (base == n_ext) ? N : n_ext;         // >= 3 (checked by the host)
  const Stencil3 g = gradient_stencil(xs + i * n_tab + base, j - base, len);
  const int p = g.p;
  double* A = amp + i * (size_t)ES_SAMP_COUNT * n_tab * 2;
  const double* vz = A + ((size_t)ES_SAMP_V_Z * n_tab + base) * 2;
  const double d_re = (g.c0 * vz[2 * p] + g.c1 * vz[2 * p + 2]) + g.c2 * vz[2 * p + 4];
  const double d_im = (g.c0 * vz[2 * p + 1] + g.c1 * vz[2 * p + 3]) + g.c2 * vz[2 * p + 5];
  const double* vx = A + ((size_t)ES_SAMP_V_X * n_tab + j) * 2;
  const double k = kk[i];
  double* o = A + ((size_t)ES_SAMP_VORT_Y * n_tab + j) * 2;
  o[0] = -(k * vx[1]) - d_re;
  o[1] = k * vx[0] - d_im;
}

// ---- table -> frames on the (x, z, t) mesh --------------------------------------------------------------------------------
struct SlabSynArgs {
  const double* xtab; const double* amp;               // [n_tab], [6 x n_tab x 2]
  const double* x;
  int N, n_ext, n_x, n_z, n_sel;
  size_t n_zt;                                         // rows of a variable over all frames: n_z n_t
  int iters;                                           // bisection steps that bring any region down to one interval
  int rows_per_block;                                  // (frame, z) rows a workgroup walks
  uint32_t mask, fill_bits;                            // fill as it is stored (already byte-swapped if requested)
  double v_scale;
};

// One wave per workgroup: it owns 256 x columns, four per lane, finds once their region, bracket and the interpolated
// (A_re, A_im) of every selected variable, keeps them in registers and walks its share of the (frame, z) rows -- runs of
// rows of one frame, variable outer and z inner, so that a wave's consecutive stores stay in one variable's block.  The
// (z, t) table and the output are __restrict__ kernel arguments so that E C and E S arrive by scalar loads (section 8's
// kernel has the reasoning).  Nothing is read back.
//   WIDE  (every row starts on a 16-byte boundary: n_x a multiple of 4 and d_out aligned) the lane owns four consecutive
//         columns: one 16-byte store per lane;
//   else  the lane owns the columns lane, lane + 64, lane + 128, lane + 192 of the chunk: four 4-byte stores, each
//         wave-instruction 256 contiguous bytes whatever the alignment.
template <bool SWAP, bool WIDE>
__global__ __launch_bounds__(64) void slab_field_synthesis_kernel(SlabSynArgs a, const double* __restrict__ tab,
                                                                 uint32_t* __restrict__ out) {
  const size_t c0 = (size_t)blockIdx.x * 256;
  const int N = a.N, n_ext = a.n_ext;
  const size_t n_tab = (size_t)N + 2 * (size_t)n_ext;
  const double* __restrict__ xt = a.xtab;
  const double x_lo = xt[0], x_hi = xt[n_tab - 1];
  const double x_m = xt[n_ext], x_p = xt[n_ext + N - 1];   // -1 and +1 as tabulated: ties on them are interior
  const uint32_t mask = a.mask;

  size_t col[4];
  double xv[4];
  int lo[4], hi[4];
  unsigned live = 0, valid = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    col[e] = c0 + (WIDE ? (size_t)threadIdx.x * 4 + e : (size_t)threadIdx.x + 64 * e);
    const bool in_mesh = col[e] < (size_t)a.n_x;
    const double x = a.x[in_mesh ? col[e] : 0];
    const bool in = x >= x_m && x <= x_p;
    const bool le = n_ext > 0 && x >= x_lo && x < x_m;
    const bool ri = n_ext > 0 && x > x_p && x <= x_hi;
    const bool ok = in_mesh && (in || le || ri);       // a NaN coordinate fails every comparison
    const int base = in ? n_ext : (le ? 0 : n_ext + N);
    xv[e] = x;
    lo[e] = ok ? base : 0;
    hi[e] = ok ? base + (in ? N : n_ext) - 1 : 0;
    live |= (in_mesh ? 1u : 0u) << e;
    valid |= (ok ? 1u : 0u) << e;
  }
  if (!live) return;
  bracket4(xt, xv, lo, hi, a.iters);                   // largest j of the region with xtab[j] <= x, at most the last but one
  double Are[ES_SVAR_COUNT][4], Aim[ES_SVAR_COUNT][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int v = 0; v < ES_SVAR_COUNT; ++v) { Are[v][e] = 0.0; Aim[v][e] = 0.0; }
    if (!((valid >> e) & 1u)) continue;
    const int j = lo[e];
    const Lerp lerp(xv[e], xt[j], xt[j + 1]);
#pragma unroll
    for (int v = 0; v < ES_SVAR_COUNT; ++v) {
      if (!((mask >> v) & 1u)) continue;
      const double* __restrict__ p = a.amp + ((size_t)v * n_tab + j) * 2;   // ES_SVAR_* and ES_SAMP_* share their order
      const double s = (v == ES_SVAR_V_X || v == ES_SVAR_V_Z || v == ES_SVAR_VORT_Y) ? a.v_scale : 1.0;
      Are[v][e] = lerp(p[0], p[2]) * s;
      Aim[v][e] = lerp(p[1], p[3]) * s;
    }
  }

  const size_t r0 = (size_t)blockIdx.y * (size_t)a.rows_per_block;
  const size_t r1 = (r0 + (size_t)a.rows_per_block < a.n_zt) ? r0 + (size_t)a.rows_per_block : a.n_zt;
  size_t zt = r0;
  while (zt < r1) {
    const size_t tau = zt / (size_t)a.n_z;
    const size_t l0 = zt - tau * (size_t)a.n_z;
    const size_t l1 = (l0 + (r1 - zt) < (size_t)a.n_z) ? l0 + (r1 - zt) : (size_t)a.n_z;
    int slot = 0;
#pragma unroll
    for (int v = 0; v < ES_SVAR_COUNT; ++v) {
      if (!((mask >> v) & 1u)) continue;
      const size_t plane = (tau * (size_t)a.n_sel + slot) * (size_t)a.n_z;
      ++slot;
      for (size_t l = l0; l < l1; ++l) {
        const size_t row = tau * (size_t)a.n_z + l;
        const double EC = tab[row], ES = tab[a.n_zt + row];
        uint32_t b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = f32_bits(Are[v][e] * EC - Aim[v][e] * ES, SWAP);
        fill_invalid(b, valid, a.fill_bits);
        store4<WIDE>(out + (plane + l) * (size_t)a.n_x, col, b, live);
      }
    }
    zt += l1 - l0;
  }
}

}  // namespace

extern "C" int es_slab_polarisation(es_context* ctx, const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                                    int n_nodes, const double* d_int_value, const double* d_int_flux, int n_ext,
                                    const double* d_ext_x, const double* d_ext_value, const double* d_ext_flux,
                                    int complex_input, const es_slab_field_profiles* pr, double rho_e, double vA_e,
                                    double c_e, double U_e, int parity, int flags, double* d_x, double* d_amp) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, n >= 0 && n_nodes >= 0 && n_ext >= 0, "negative size");
  ES_REQUIRE(ctx, n_nodes >= 3, "the interior needs at least 3 points for its derivative");
  ES_REQUIRE(ctx, n_ext == 0 || n_ext >= 3, "an exterior needs at least 3 points for its derivative, or 0 to leave it out");
  ES_REQUIRE(ctx, complex_input == 0 || complex_input == 1, "complex_input");
  ES_REQUIRE(ctx, parity == ES_SLAB_MODE_SAUSAGE || parity == ES_SLAB_MODE_KINK, "parity");
  ES_REQUIRE(ctx, (flags & ~ES_SLAB_FIELD_SHEAR_PT) == 0, "flags");
  const size_t n_tab = (size_t)n_nodes + 2 * (size_t)n_ext;
  ES_REQUIRE(ctx, n_tab < 0x7fffffffull, "too many table points");
  if (n == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_k && d_w_re && d_x && d_amp, "null pointer");
  ES_REQUIRE(ctx, d_int_value && d_int_flux, "null interior arrays");
  ES_REQUIRE(ctx, pr != nullptr, "null profiles");
  ES_REQUIRE(ctx, pr->rho && pr->c2 && pr->vA2 && pr->U && pr->dU, "null profile array");
  ES_REQUIRE(ctx, n_ext == 0 || (d_ext_x && d_ext_value && d_ext_flux), "null exterior arrays");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  SlabPolArgs a;
  a.k = d_k; a.w_re = d_w_re; a.w_im = d_w_im; a.iv = d_int_value; a.ifl = d_int_flux;
  a.ex = d_ext_x; a.ev = d_ext_value; a.ef = d_ext_flux;
  a.p = *pr;
  a.n = n; a.N = n_nodes; a.n_ext = n_ext; a.cplx = complex_input; a.flags = flags;
  a.rho_e = rho_e; a.vAe2 = vA_e * vA_e; a.ce2 = c_e * c_e; a.U_e = U_e;
  a.sigma = (parity == ES_SLAB_MODE_SAUSAGE) ? -1.0 : 1.0;
  a.x = d_x; a.amp = d_amp;
  const size_t tot = (size_t)n * n_tab;
  ES_REQUIRE(ctx, (tot + 255) / 256 <= 0x7fffffffull, "too many points");
  const dim3 grid((unsigned)((tot + 255) / 256));
  hipLaunchKernelGGL(slab_field_polarisation_kernel, grid, dim3(256), 0, ctx->stream, a);
  ES_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(slab_field_vorticity_kernel, grid, dim3(256), 0, ctx->stream, d_x, d_amp, d_k, n, n_nodes, n_ext);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}

extern "C" int es_slab_field_synthesis(es_context* ctx, const double* d_xtab, const double* d_amp, int n_nodes, int n_ext,
                                       double k, double w_re, double w_im, const double* d_x, int n_x, const double* d_z,
                                       int n_z, const double* d_t, int n_t, uint32_t var_mask, double v_scale, float fill,
                                       int flags, float* d_out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, n_nodes >= 0 && n_ext >= 0 && n_x >= 0 && n_z >= 0 && n_t >= 0, "negative size");
  ES_REQUIRE(ctx, var_mask != 0, "empty variable mask");
  ES_REQUIRE(ctx, (var_mask >> ES_SVAR_COUNT) == 0, "unknown variable bit");
  ES_REQUIRE(ctx, (flags & ~ES_FIELD_BIG_ENDIAN) == 0, "flags");
  ES_REQUIRE(ctx, n_nodes >= 3, "the interior needs at least 3 points");
  ES_REQUIRE(ctx, n_ext == 0 || n_ext >= 3, "an exterior needs at least 3 points, or 0 to leave it out");
  const size_t n_tab = (size_t)n_nodes + 2 * (size_t)n_ext;
  ES_REQUIRE(ctx, n_tab < 0x7fffffffull, "table size");
  ES_REQUIRE(ctx, (size_t)n_z * (size_t)n_t < 0x7fffffffull, "mesh too large");
  ES_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(d_out) & 3u) == 0, "float32 output needs 4-byte alignment");
  if (n_x == 0 || n_z == 0 || n_t == 0) return ES_SUCCESS;
  ES_REQUIRE(ctx, d_xtab && d_amp && d_x && d_z && d_t && d_out, "null pointer");
  ES_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t n_zt = (size_t)n_z * n_t;
  double* tab;
  const int rc = zt_tables<true>(ctx, d_z, n_z, d_t, n_t, k, w_re, w_im, &tab);
  if (rc) return rc;
  const bool swap = (flags & ES_FIELD_BIG_ENDIAN) != 0;
  SlabSynArgs a;
  a.xtab = d_xtab; a.amp = d_amp; a.x = d_x;
  a.N = n_nodes; a.n_ext = n_ext; a.n_x = n_x; a.n_z = n_z; a.n_zt = n_zt;
  a.n_sel = __builtin_popcount(var_mask);
  a.iters = bisection_iters(n_nodes > n_ext ? n_nodes : n_ext);
  a.fill_bits = fill_bits_of(fill, swap);
  a.mask = var_mask; a.v_scale = v_scale;
  // workgroups over (chunk of 256 columns, group of rows): about 16 waves per CU, and no more, because each workgroup
  // repeats the x stage of its columns
  const size_t gx = ((size_t)n_x + 255) / 256;
  size_t gy = (ES_SLAB_SYNTH_WAVES + gx - 1) / gx;
  if (gy > n_zt) gy = n_zt;
  if (gy > 65535) gy = 65535;
  a.rows_per_block = (int)((n_zt + gy - 1) / gy);
  gy = (n_zt + (size_t)a.rows_per_block - 1) / (size_t)a.rows_per_block;
  const bool wide = (n_x % 4 == 0) && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(64);
  uint32_t* out = reinterpret_cast<uint32_t*>(d_out);
  auto kernel = ES_SWAP_WIDE_KERNEL(slab_field_synthesis_kernel, swap, wide);
  hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, a, tab, out);
  ES_HIP_CHECK(ctx, hipGetLastError());
  return ES_SUCCESS;
}
