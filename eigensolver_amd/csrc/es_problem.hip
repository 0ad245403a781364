// The problem handle of the shooting path: es_problem_create / es_problem_destroy and the argument checks every entry
// point shares.  Host code only.
#include <vector>
#include <cstdlib>
#include <cmath>

#include "es_shoot_host.hpp"

int check_problem(es_context* ctx, const es_problem* prob) {
  ES_REQUIRE(ctx, prob != nullptr, "null problem");
  return ES_SUCCESS;
}

int check_root_table(es_context* ctx, const es_root_table* table) {
  ES_REQUIRE(ctx, table->capacity == 0 || (table->d_k && table->d_w && table->d_w_lo && table->d_w_hi &&
                                           table->d_resid && table->d_row && table->d_flag),
             "null root table arrays");
  return ES_SUCCESS;
}

// ---- problem creation: pack the k-independent base fields (host, fp64) and upload them -----------------------
extern "C" int es_problem_create(es_context* ctx, const es_shoot_desc* d, const es_profiles* pr, es_problem** out) {
  if (!ctx) return ES_ERR_INVALID_ARG;
  ES_REQUIRE(ctx, d && pr && out, "null pointer");
  *out = nullptr;
  ES_REQUIRE(ctx, d->n_nodes >= 2 && d->n_nodes <= (1 << 24), "n_nodes out of range");
  ES_REQUIRE(ctx, d->geometry >= 0 && d->geometry <= 3, "geometry");
  ES_REQUIRE(ctx, d->x_boundary == -1.0 || d->x_boundary == 1.0, "x_boundary must be -1 or +1");
  const int N = d->n_nodes, npts = 2 * N - 1;
  int nb = 0;
  switch (d->geometry) {
    case ES_GEOM_CYLINDER: nb = FamTraits<FAM_CYL0>::NB; break;
    case ES_GEOM_CYLINDER_TWIST: nb = FamTraits<FAM_CYLT>::NB; break;
    case ES_GEOM_SLAB_DENSITY: nb = FamTraits<FAM_SLABD>::NB; break;
    default: nb = FamTraits<FAM_SLABF>::NB; break;
  }
  std::vector<double> base((size_t)nb * npts);
  auto B = [&](int f, int i) -> double& { return base[(size_t)f * npts + i]; };
  if (d->geometry == ES_GEOM_CYLINDER || d->geometry == ES_GEOM_CYLINDER_TWIST) {
    ES_REQUIRE(ctx, pr->r && pr->rho && pr->c2 && pr->Bz, "cylinder profiles r, rho, c2, Bz required");
    ES_REQUIRE(ctx, d->axis_bc >= 0 && d->axis_bc <= 2, "axis_bc");
    ES_REQUIRE(ctx, d->c1_power == 1 || d->c1_power == 2, "c1_power");
    ES_REQUIRE(ctx, d->m >= 0 && d->m_ext >= 0 && d->m_ext <= 64, "m");
    for (int i = 0; i < npts; ++i) {
      const double r = pr->r[i], rho = pr->rho[i], c2 = pr->c2[i], Bz = pr->Bz[i];
      const double Bphi = pr->Bphi ? pr->Bphi[i] : 0.0;
      const double vz = pr->vz ? pr->vz[i] : 0.0;
      const double vphi = pr->vphi ? pr->vphi[i] : 0.0;
      const double sr = sqrt(rho);
      const double bA = Bz / sr;                    // (k B_z)/sqrt(rho) per unit k, CF:581
      const double vA = (Bz + Bphi) / sr;           // vA_i as written, CF:173-174
      const double S = c2 + vA * vA;
      const double q = c2 / S;
      if (d->geometry == ES_GEOM_CYLINDER) {
        ES_REQUIRE(ctx, Bphi == 0.0 && vphi == 0.0, "ES_GEOM_CYLINDER needs Bphi = vphi = 0 (use CYLINDER_TWIST)");
        B(C0_VZ, i) = vz;
        B(C0_BA, i) = bA;
        B(C0_Q, i) = q;
        B(C0_A1, i) = rho / r;
        B(C0_B1, i) = r / (rho * S);
        B(C0_E1, i) = 1.0 / (r * rho);
        B(C0_E2, i) = r / rho;
      } else {
        // the k-independent parts of the node entries, in the operation order make_entry used per lane and node
        const double dm = (double)d->m, dm2 = dm * dm;
        const double invr = 1.0 / r, invr2 = invr * invr;
        const double bphr = Bphi / r, vphr = vphi / r;
        const double Bphi_n = bphr * r, vphi_n = vphr * r;   // as the device formed them from the stored B_phi/r, v_phi/r
        B(CT_MB, i) = dm * bphr;
        B(CT_BZ, i) = Bz;
        B(CT_BA, i) = bA;
        B(CT_MV, i) = dm * vphr;
        B(CT_VZ, i) = vz;
        B(CT_Q, i) = q;
        B(CT_E3, i) = rho * S;
        B(CT_RHO, i) = rho;
        B(CT_E5, i) = rho * vphi_n * vphi_n * invr;
        B(CT_E6, i) = 2.0 * Bphi_n * Bphi_n * invr;
        B(CT_C7, i) = 2.0 * Bphi_n * vphi_n;
        B(CT_INVR, i) = invr;
        B(CT_BPHI, i) = Bphi_n;
        B(CT_E9, i) = rho * vphi_n;
        B(CT_E10, i) = 2.0 * dm * S * invr2;
        B(CT_S, i) = S;
        B(CT_M2R2, i) = dm2 * invr2;
        B(CT_RDC3, i) = pr->rdC3 ? pr->rdC3[i] : 0.0;
        B(CT_E13, i) = 4.0 * S * invr2;
        B(CT_R, i) = r;
      }
    }
  } else if (d->geometry == ES_GEOM_SLAB_DENSITY) {
    ES_REQUIRE(ctx, pr->rho && pr->c2 && pr->vA2, "slab density profiles rho, c2, vA2 required");
    for (int i = 0; i < npts; ++i) {
      B(SD_RHO, i) = pr->rho[i];
      B(SD_C2, i) = pr->c2[i];
      B(SD_VA2, i) = pr->vA2[i];
    }
  } else {
    ES_REQUIRE(ctx, pr->U, "slab flow profile U required");
    for (int i = 0; i < npts; ++i) {
      B(SF_U, i) = pr->U[i];
      B(SF_DU, i) = pr->dU ? pr->dU[i] : 0.0;
      B(SF_DDU, i) = pr->ddU ? pr->ddU[i] : 0.0;
    }
  }
  es_problem* p = new es_problem();
  p->desc = *d;
  ShootDev& S = p->dev;
  memset(&S, 0, sizeof(S));
  S.family = d->geometry;
  S.n_nodes = N;
  S.npts = npts;
  S.xb = d->x_boundary;
  S.h = (d->x_end - d->x_boundary) / (double)(N - 1);
  S.rho_e = d->rho_e;
  S.vAe2 = d->vA_e * d->vA_e;
  S.ce2 = d->c_e * d->c_e;
  S.cTe2 = d->cT_e * d->cT_e;
  S.Se = S.vAe2 + S.ce2;
  S.U_e = d->U_e;
  S.R_factor = d->L_factor * 2.0 * 3.14159265358979323846;
  S.ic0 = d->ic_value;
  S.ic1 = d->ic_slope;
  S.m = d->m; S.m_ext = d->m_ext; S.axis_bc = d->axis_bc; S.c1_power = d->c1_power;
  S.bc_const = S.bc_const_raw = d->bc_const;
  if (d->geometry == FAM_CYL0 && d->bc_const != 0.0) {
    // the fp64 marches of this family deliver z times adjoint_scale (a factor 3 per step, an exact power of two back per
    // LDS chunk): a non-zero target of the axis condition carries the same factor
    double c = 1.0;
    const int nsteps = N - 1;
    for (int ch = (nsteps + es_shoot_shared::CH - 1) / es_shoot_shared::CH - 1; ch >= 0; --ch) {
      const int c0 = ch * es_shoot_shared::CH;
      const int nst = (nsteps - c0 < es_shoot_shared::CH) ? (nsteps - c0) : es_shoot_shared::CH;
      for (int i = 0; i < nst; ++i) c *= 3.0;
      c = ldexp(c, adjoint_rescale_exp(nsteps - c0 - nst, nsteps - c0));
    }
    S.bc_const = d->bc_const * c;
  }
  S.slab_sign = (d->slab_mode == ES_SLAB_MODE_SAUSAGE) ? -1.0 : 1.0;
  S.c2_i = d->c_i * d->c_i;
  S.vA2_i = d->vA_i * d->vA_i;
  S.S_i = S.c2_i + S.vA2_i;
  S.cT2_i = (S.S_i > 0.0) ? S.c2_i * S.vA2_i / S.S_i : 0.0;
  S.rho_i = d->rho_i;
  S.accept_norm = d->accept_norm;
  {
    // units of the fp32 screening march: V = 2^ev from the larger exterior speed, R = 4^er from the exterior density, by
    // their binary exponents alone -- inputs rescaled by powers of two shift ev and er by exactly as much, and the march
    // sees the same numbers.  The velocity scale stays 1 where the coefficients are not homogeneous in it (the reference's
    // formulas): the flow slab with shear (D(x) of SF-G:423, G = S t^2 + k^4 cT^2 c^2) and the twisted cylinder with
    // c1_power = 1 (C1 = Q Om - (2 m S / r^2) t2 T).
    auto half_exp = [](double x) { return (x > 0.0 && std::isfinite(x)) ? (int)std::floor(0.5 * (double)ilogb(x)) : 0; };
    bool homogeneous = true;
    if (d->geometry == ES_GEOM_SLAB_FLOW)
      for (int i = 0; i < npts; ++i) homogeneous = homogeneous && B(SF_DU, i) == 0.0 && B(SF_DDU, i) == 0.0;
    if (d->geometry == ES_GEOM_CYLINDER_TWIST && d->c1_power != 2) homogeneous = false;
    p->f32_ev = homogeneous ? half_exp(fmax(S.vAe2, S.ce2)) : 0;      // vAe2, ce2: speeds squared
    p->f32_er = half_exp(S.rho_e);
  }
  if (d->geometry == ES_GEOM_CYLINDER || d->geometry == ES_GEOM_SLAB_FLOW || d->geometry == ES_GEOM_SLAB_DENSITY) {
    // continuum bands in phase speed (band_crossed): node j is inside band t iff centre_j - a_j < W < centre_j + a_j
    //   cylinder:     centre = v_z, a = |bA| (Alfven), |bA| sqrt(q) (cusp)
    //   flow slab:    centre = U,   a = c_i, cT_i, vA_i (uniform) and the half line W < U_j (sign of Om)
    //   density slab: centre = 0,   a = c_j, cT_j, vA_j
    const bool cyl = (d->geometry == ES_GEOM_CYLINDER), flow = (d->geometry == ES_GEOM_SLAB_FLOW);
    S.use_bands = 1;
    S.n_bands = cyl ? 2 : (flow ? 4 : 3);
    const double slab_a[3] = {sqrt(S.c2_i), sqrt(S.cT2_i), sqrt(S.vA2_i)};
    for (int t = 0; t < S.n_bands; ++t) {
      double lo_min = INFINITY, lo_max = -INFINITY, hi_min = INFINITY, hi_max = -INFINITY, lo_prev = 0.0, hi_prev = 0.0;
      const bool half_line = (flow && t == 3);
      bool never = !cyl;                                   // slab term whose speed is zero at every node
      for (int i = 0; i < npts; ++i) {
        double centre, a;
        if (cyl) {
          centre = B(C0_VZ, i);
          a = fabs(B(C0_BA, i)) * (t == 0 ? 1.0 : sqrt(B(C0_Q, i)));
        } else if (flow) {
          centre = B(SF_U, i);
          a = half_line ? 0.0 : slab_a[t];
        } else {
          const double c2 = B(SD_C2, i), vA2 = B(SD_VA2, i);
          centre = 0.0;
          a = sqrt(t == 0 ? c2 : (t == 1 ? c2 * vA2 / (c2 + vA2) : vA2));
        }
        if (a > 0.0 || half_line) never = false;
        const double lo = half_line ? -INFINITY : centre - a, hi = centre + a;
        if (!std::isfinite(hi) || (cyl && !(a > 0.0))) S.use_bands = 0;              // empty / undefined interval
        if (i > 0 && !half_line && a > 0.0 && !(lo < hi_prev && lo_prev < hi)) S.use_bands = 0;   // disjoint neighbours
        lo_min = fmin(lo_min, lo); lo_max = fmax(lo_max, lo);
        hi_min = fmin(hi_min, hi); hi_max = fmax(hi_max, hi);
        lo_prev = lo; hi_prev = hi;
      }
      S.band[t][0] = lo_min; S.band[t][1] = lo_max; S.band[t][2] = hi_min; S.band[t][3] = hi_max;
      // a speed of zero (e.g. cT = 0 without field): the term never changes sign -> a band that nothing satisfies
      if (never) { S.band[t][0] = INFINITY; S.band[t][3] = -INFINITY; }
    }
    if (getenv("ES_FORCE_SIGN_TRACKING")) S.use_bands = 0;
  }
  if (hipSetDevice(ctx->device) != hipSuccess ||
      hipMalloc(&p->d_base, base.size() * sizeof(double)) != hipSuccess) {
    ctx->last_error = "hipMalloc(base table) failed";
    delete p;
    return ES_ERR_HIP;
  }
  if (hipMemcpyAsync(p->d_base, base.data(), base.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    ctx->last_error = "upload of base table failed";
    (void)hipFree(p->d_base);
    delete p;
    return ES_ERR_HIP;
  }
  S.base = p->d_base;
  *out = p;
  return ES_SUCCESS;
}

extern "C" int es_problem_destroy(es_context* ctx, es_problem* prob) {
  if (!prob) return ES_SUCCESS;
  if (ctx) (void)hipSetDevice(ctx->device);
  if (prob->d_base) (void)hipFree(prob->d_base);
  delete prob;
  return ES_SUCCESS;
}
