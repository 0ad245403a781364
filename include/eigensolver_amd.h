/* eigensolver_amd.h -- C ABI of the MI355X (gfx950) dispersion-relation hot path.
 *
 * The reference (samuelskirvin/EIGENSOLVER) has no FFI: its operator boundary is the per-geometry worker
 *     sausage(wavenumber, sausage_ws, sausage_ks, freq) / kink(wavenumber, kink_ws, kink_ks, freq)
 * (e.g. Cylinder/Non-uniform flow/Coronal/solvers/Cylinder_method_flow_testing.py:554, :855) plus the analytic
 * scan at module level of Slab/Non uniform flow/Solver/flow_multiprocessor.py:107-303.  Everything those
 * functions capture from module globals is passed here as explicit POD structs / arrays.
 *
 * Conventions
 *  - every function returns an int status (ES_SUCCESS == 0); no exceptions cross the boundary;
 *  - pointers named d_* are DEVICE pointers (HBM), h_* are host pointers; all floating point is IEEE fp64;
 *  - all work is enqueued on the hipStream_t given at context creation (passed as void*); functions that
 *    return counts through host pointers synchronise that stream, the pure *_async entry points do not;
 *  - the library is GPU-only: there is no CPU fallback behind any entry point.
 */
#ifndef EIGENSOLVER_AMD_H
#define EIGENSOLVER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ES_ABI_VERSION 1

/* ---- status codes of the library calls -------------------------------------------------------------- */
enum {
  ES_SUCCESS = 0,
  ES_ERR_INVALID_ARG = 1,
  ES_ERR_HIP = 2,          /* a HIP runtime call failed: see es_last_error()           */
  ES_ERR_CAPACITY = 3,     /* caller-provided output buffer too small (count is still returned) */
  ES_ERR_NO_DEVICE = 4,
  ES_ERR_UNSUPPORTED = 5,
  ES_ERR_EVAL_CAP = 6,     /* es_worker_run: a task exceeded its evaluation bound; its root list is incomplete   */
  ES_ERR_SCREENING = 7     /* es_shoot_find_roots_mixed: an fp32-screened bracket was not confirmed in fp64      */
};

/* ---- per-point status written next to D(k, omega) ------------------------------------------------------
 * The reference silently skips m_e < 0 ("leaky", e.g. Cylinder_method_flow_testing.py:760) and lets inf/nan
 * propagate; here every lane reports why it has no usable determinant. */
enum {
  ES_PT_OK = 0,
  ES_PT_LEAKY = 1,        /* m_e < 0: reference skips the point                                  */
  ES_PT_NONFINITE = 2,    /* evaluated by the reference but the result is inf/nan (singular speed) */
  ES_PT_CONTINUUM = 3     /* Omega^2 crosses omega_A^2(r) or omega_c^2(r) inside the domain        */
};

typedef struct es_context es_context;   /* opaque: device, stream, scratch workspace */
typedef struct es_problem es_problem;   /* opaque: one worker configuration + its profile tables in HBM */

/* ---- context ------------------------------------------------------------------------------------------ */
int es_abi_version(void);
const char* es_status_string(int status);
/* device: HIP device ordinal; stream: hipStream_t (NULL = default stream of that device). */
int es_context_create(int device, void* stream, es_context** out);
int es_context_destroy(es_context* ctx);
const char* es_last_error(const es_context* ctx);
int es_context_synchronize(es_context* ctx);
/* Measurement aid (bench.py `roofline`): with the timer on, every launch of a grid-march kernel (the fp64 kernel of
 * es_shoot_eval_grid[_ex], the fp32 screening kernel of es_shoot_find_roots_mixed) is bracketed by HIP events on the
 * context's stream.  es_context_grid_time synchronises the stream, returns the summed elapsed time and the number of
 * launches since the last call and forgets them.  The reference has no counterpart (it times whole runs with
 * time.time(), e.g. Density_cylinder.py:1129). */
int es_context_grid_timer(es_context* ctx, int enable);
int es_context_grid_time(es_context* ctx, double* h_total_ms, int* h_launches);
/* sizeof() of the ABI structs as this library was compiled, for binding self-checks:
 * which = 0 es_slab_analytic_params, 1 es_shoot_desc, 2 es_profiles, 3 es_root_table, 4 es_worker_spec,
 * 5 es_cyl_uniform_params, 6 es_complex_root_table, 7 es_field_profiles; -1 for an unknown index. */
int es_abi_sizeof(int which);

/* ========================================================================================================
 * (1) Analytic slab dispersion relations with steady flow and their sign-change scan.
 *     Replaces flow_multiprocessor.py:107-127 (m0, me, n0, disp_rel_*) and :166-272 (scan loops),
 *     :284-303 (one-sided pole filter).
 * ====================================================================================================== */
typedef struct es_slab_analytic_params {
  double vA_i, c_i, vA_e, c_e;   /* flow_multiprocessor.py:63-66                                   */
  double mach_i, mach_e;         /* :97-98  (U_i, U_e, not divided by vA_i)                         */
  double R1;                     /* :79     rho_e / rho_i                                           */
  double cT_i, cT_e;             /* :85-89  the *normalised* tube speeds exactly as the script computes them */
} es_slab_analytic_params;

enum { ES_SLAB_SAUSAGE = 0, ES_SLAB_KINK = 1, ES_SLAB_SAUSAGE_BODY = 2, ES_SLAB_KINK_BODY = 3 };

/* D[iK * nW + iW] = disp_rel_<mode>(W[iW], K[iK]).  One grid point per lane. */
int es_slab_analytic_eval(es_context* ctx, const es_slab_analytic_params* p, int mode,
                          const double* d_K, int nK, const double* d_W, int nW, double* d_D);

/* Scan loops :166-272: for every K (outer) and V in W (inner): f(V,K) * f(V+step,K) < 0  ->  root (K, (V+V+step)/2).
 * Roots are written in the reference's loop order.  *h_count receives the number found (may exceed capacity,
 * then ES_ERR_CAPACITY is returned and only `capacity` roots are written). */
int es_slab_analytic_scan(es_context* ctx, const es_slab_analytic_params* p, int mode,
                          const double* d_K, int nK, const double* d_W, int nW, double step,
                          double* d_rootK, double* d_rootW, int capacity, int* h_count);

/* Pole filter :284-303: keep[i] = disp_rel_<mode>(rootW[i], rootK[i]) < thresh (one-sided, as written). */
int es_slab_analytic_filter(es_context* ctx, const es_slab_analytic_params* p, int mode,
                            const double* d_rootK, const double* d_rootW, int n, double thresh,
                            uint8_t* d_keep);


/* ========================================================================================================
 * (2) Shooting evaluation of the boundary determinant D(k, omega) for non-uniform interiors.
 *     Replaces, per (k, omega), the body of the reference workers (coefficients -> exterior ODE -> interior
 *     shoot -> mismatch), e.g. Cylinder_method_flow_testing.py:694-804 (kink) / :991-1111 (sausage),
 *     multiprocessor_Inhomogeneous_method.py:421-501, flow_multiprocessor_coronal.py:400-480,
 *     Twisted_photospheric_nonlinear_flow_kink_fast.py:601-712.
 *     D is the reference's mismatch (xi_e - xi_i for cylinders, P_e - P_i for slabs) divided by the exterior
 *     amplitude |P_e(boundary)| resp. |Vx_e(boundary)|, sign of the reference's amplitude kept.
 * ====================================================================================================== */
enum { ES_GEOM_CYLINDER = 0, ES_GEOM_CYLINDER_TWIST = 1, ES_GEOM_SLAB_DENSITY = 2, ES_GEOM_SLAB_FLOW = 3 };
enum { ES_AXIS_KINK = 0, ES_AXIS_SAUSAGE = 1, ES_AXIS_ROTATION_KINK = 2 };
enum { ES_SLAB_MODE_SAUSAGE = 0, ES_SLAB_MODE_KINK = 1 };
enum { ES_W_ABSOLUTE = 0,      /* omega = w[iw]                       (one frequency vector for all k)     */
       ES_W_PHASE_SPEED = 1,   /* omega = k * w[iw]                   (the reference's bands speeds*k)      */
       ES_W_PER_ROW = 2 };     /* omega = w[ik * nw + iw]             (one frequency array per task)        */

/* Everything a reference worker captures from module globals.
 *
 * Units.  The speeds, densities and fields of es_shoot_desc, es_profiles and es_cyl_uniform_params are dimensional and are used
 * as given: nothing normalises them (lengths are in units of the half-width / radius: x_boundary = -1 or +1).  The results
 * follow scaling laws: with every speed times V and every density times R (B_z, B_phi times V sqrt(R); rdC3 and bc_const times
 * V^2 R; omega times V; k unchanged), D, outer and inner of a cylinder come out times 1 / (V^2 R) and those of a slab times V R,
 * d/d omega takes one V off, roots and group speeds come out times V, rel, resid, statuses, flags, node and iteration counts
 * do not change -- bit for bit when V and sqrt(R) are powers of two (DESIGN.md section 4e has the table;
 * tests/test_unit_scaling_*.py).  Tested range: V in [2^-20, 2^20] and R in [4^-20, 4^20] around the reference's
 * normalisation (speeds, densities and omega of order 1), the fp32 screening of es_shoot_find_roots_mixed included, which
 * marches in units it derives from vA_e, c_e and rho_e.
 * Exception: the flow slab with shear (ES_GEOM_SLAB_FLOW with dU != 0, and section 6 on such a profile) is not homogeneous in
 * the velocity scale -- the reference's D(x), flow_multiprocessor_coronal.py:423, adds Omega^2 - k^2 cT^2 to a term without
 * dimension of speed -- and must be given in the reference's normalised speeds; it follows the density scale.
 * Beyond V = 2^+-40 the shared reciprocal of the flow slab's denominators leaves the fp64 range: measured on the CPU port of
 * these kernels, finite wrong D with ES_PT_OK at V = 2^40 (uniform-flow slab), ES_PT_NONFINITE everywhere at V = 2^-40. */
typedef struct es_shoot_desc {
  int32_t geometry;        /* ES_GEOM_*                                                                   */
  int32_t n_nodes;         /* interior nodes N: the reference's `ix` grid (linspace(x_b, x_end, N)); the
                              propagator takes one RK4 step per interval                                    */
  double x_boundary;       /* first node: -1 (CD-C, CF, slabs) or +1 (CD-P, CR-*)                          */
  double x_end;            /* last node: -/+ r_axis for cylinders (0.001 / 0.01), +1 for slabs             */
  /* exterior medium */
  double rho_e, vA_e, c_e, cT_e, U_e;
  double L_factor;         /* far field at |x| = L_factor * 2 pi / k   (3 or 7)                             */
  double ic_value, ic_slope; /* reference's P0 / V0 = [1e-8, 1e-8] or [1e-8, 1e-15]                          */
  /* cylinder */
  int32_t m;               /* azimuthal order used in the interior coefficient set                          */
  int32_t m_ext;           /* order hard-coded in the reference's exterior ODE (1 kink, 0 sausage)          */
  int32_t axis_bc;         /* ES_AXIS_*                                                                     */
  int32_t c1_power;        /* C1 = Q*Omega (1: CD-C:590) or Q*Omega^2 (2: CF:598, CR-KF:493)                */
  double bc_const;         /* kink: B_phi(x_b)^2 ; rotation: B_phi(1)^2 - rho(1) v_phi(1)^2                 */
  /* slab */
  int32_t slab_mode;       /* ES_SLAB_MODE_*                                                                */
  int32_t accept_norm;     /* 0: rel = 100|d|/max(|outer|,|inner|) (all workers) ; 1: 100|d|/|outer| (CR-KS:722)   */
  double c_i, vA_i, rho_i; /* uniform interior speeds of the flow slab (SF-U / SF-G)                        */
} es_shoot_desc;

/* Profile samples on the 2N-1 points x_j = x_boundary + j*(x_end - x_boundary)/(2N-2)  (nodes and midpoints),
 * host pointers, each of length 2N-1; unused ones may be NULL:
 *   cylinder : r (the x_j themselves), rho, c2 (= c_i^2), Bz, Bphi, vz, vphi, rdC3 (= r d/dr[(Bphi/r)^2 - rho (vphi/r)^2])
 *   slab dens: rho, c2, vA2
 *   slab flow: U, dU, ddU                                                                                   */
typedef struct es_profiles {
  const double* r; const double* rho; const double* c2; const double* vA2;
  const double* Bz; const double* Bphi; const double* vz; const double* vphi; const double* rdC3;
  const double* U; const double* dU; const double* ddU;
} es_profiles;

int es_problem_create(es_context* ctx, const es_shoot_desc* desc, const es_profiles* h_profiles, es_problem** out);
int es_problem_destroy(es_context* ctx, es_problem* prob);

/* D[ik*nw + iw], status[ik*nw + iw] (ES_PT_*), optional rel[ik*nw + iw] = 100*|d|/max(|outer|,|inner|)
 * (the reference's acceptance measure, e.g. Cylinder_method_flow_testing.py:817).  One grid point per lane,
 * radial-profile coefficients staged in LDS per k-row. */
int es_shoot_eval_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                       const double* d_w, int nw, int w_mode,
                       double* d_D, double* d_rel /* may be NULL */, uint8_t* d_status);

/* es_shoot_eval_grid with options.  flags = 0 is es_shoot_eval_grid.
 * ES_EVAL_SKIP_CONTINUUM: points whose status is ES_PT_CONTINUUM get D = rel = NaN instead of the value a march
 * through the singular layer gives (the reference integrates through it with LSODA and returns integrator noise,
 * which the grid search never brackets -- es_shoot_find_roots requires both ends ES_PT_OK).  Where the flag can be
 * decided before the march (families with connected continuum bands in phase speed) such points
 * are not marched at all; with ES_W_PHASE_SPEED whole omega-columns inside a band are removed from the launch
 * (ordered compaction of the live columns on the device, no host synchronisation).  D and rel are identical to
 * flags = 0 at every point whose status is not ES_PT_CONTINUUM; statuses are identical except that a continuum point
 * whose march would have overflowed (ES_PT_NONFINITE with flags = 0) is reported ES_PT_CONTINUUM. */
enum { ES_EVAL_SKIP_CONTINUUM = 1 };
int es_shoot_eval_grid_ex(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                          const double* d_w, int nw, int w_mode, int flags,
                          double* d_D, double* d_rel /* may be NULL */, uint8_t* d_status);

/* Measurement aid: the launch shape es_shoot_eval_grid selects for rows of nw frequencies of this problem -- points per
 * lane, waves per SIMD of the register cap, per-node sign tracking on / off -- i.e. the instantiation
 * shoot_grid_kernel<family, pts, 256, track, wpe> that bench.py prices against profiles/isa_loop_counts.json.  A NEGATIVE
 * *h_pts = -p names the shape with two k-rows per workgroup, shoot_grid_kernel_r2<family, p, track, wpe> (rows of at most
 * 512 frequencies of the untwisted cylinder and the slabs, at least two rows). */
int es_shoot_grid_shape(es_context* ctx, const es_problem* prob, int nw, int* h_pts, int* h_wpe, int* h_track);

/* The same determinant at n arbitrary (k, omega) pairs (one pair per lane, no shared k). */
int es_shoot_eval_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                         double* d_D, double* d_rel /* may be NULL */, uint8_t* d_status);

/* Root table of the grid search (structure of arrays, caller allocated, `capacity` entries each). */
typedef struct es_root_table {
  double* d_k;        /* wavenumber of the row                                       */
  double* d_w;        /* refined omega                                               */
  double* d_w_lo;     /* bracket [w_lo, w_hi] from the grid                          */
  double* d_w_hi;
  double* d_resid;    /* rel = 100 |d| / max(|outer|, |inner|) at the refined omega  */
  int32_t* d_row;     /* row index ik                                                */
  uint8_t* d_flag;    /* 1 = accepted root (resid < tol), 0 = sign change at a pole / continuum edge */
  int32_t capacity;
} es_root_table;

/* Grid search: brackets = sign changes of D between omega-neighbours of the same row with both ends ES_PT_OK
 * (wavefront shuffle + ballot, ordered compaction: rows outer, omega inner); each bracket is narrowed at least
 * as far as `n_bisect` bisection steps would (the reference's 3-point linspace refinement, e.g. :823-829, run to
 * convergence; executed as rounds of 17-section with 16 lanes per bracket -- a fixed rule, so that the table of a grid
 * does not depend on how the grid is tiled over calls or GPUs -- as many as shrink the bracket by 2^n_bisect, always keeping the sign change nearest to the lower end), then polished in fp64 by two regula-falsi steps (the secant through the
 * bracket ends: the Newton-type refinement of the north star, without a derivative of D) and classified with the
 * reference's acceptance rule rel < tol_percent at the last secant point, which is the root reported;
 * [w_lo, w_hi] is the final bracket around it.
 * d_D / d_status must hold the output of es_shoot_eval_grid for the same inputs. */
int es_shoot_find_roots(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                        const double* d_w, int nw, int w_mode, const double* d_D, const uint8_t* d_status,
                        int n_bisect, double tol_percent, es_root_table* table, int* h_count);

/* es_shoot_find_roots without any host synchronisation (pipelined callers, k-tiles of a multi-GPU run: a 512-row tile
 * is 3 ms of GPU work, a read-back in the middle of it is a tenth of that).  The bracket count is written to the
 * caller's device word d_count (it may exceed table->capacity: then only `capacity` brackets were written and refined --
 * the caller checks when it reads the count, as es_shoot_find_roots does for it).  The refinement launches are sized for
 * table->capacity and take the count from device memory, so size the table for the data (about twice the expected
 * count), not for the worst case.  Same table, bit for bit, as es_shoot_find_roots. */
int es_shoot_find_roots_async(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                              const double* d_w, int nw, int w_mode, const double* d_D, const uint8_t* d_status,
                              int n_bisect, double tol_percent, es_root_table* table, int32_t* d_count);

/* Mixed-precision grid search (BASELINE.json configs[4]: "fp32 bracket + fp64 refine"; the reference itself is fp64
 * throughout), for the cylinder families and (round 3) for the slab families whose continuum flag comes from phase-speed bands
 * (every profile of the reference; a slab profile whose node intervals do not overlap needs per-node sign tracking, which
 * exists in fp64 only: ES_ERR_UNSUPPORTED).  What is GUARANTEED: every bracket
 * it reports is an fp64 bracket (both ends re-evaluated in fp64, ES_ERR_SCREENING otherwise) and is refined exactly as
 * es_shoot_find_roots refines it.  What is EMPIRICAL: that no fp64 bracket is missed -- a sign change between two points
 * fp32 judged "sure" (|D| > 5e-2 of the scale, every watched coefficient term more than 1e-3 away from zero) would go
 * unnoticed; the thresholds are supported by measurement, not by an error bound (largest fp32 error among vouched-for points
 * 4.5e-3 of the scale over 3 800 random problems, tools/fuzz_mixed.py; every point of configs[4] in
 * tests/test_full_size_parity_gpu.py and tools/full_size_parity.py): in all of them the bracket set is identical and the root
 * table bit-identical to es_shoot_eval_grid + es_shoot_find_roots.  To check this half on your own equilibrium, run
 * es_shoot_audit_screening (below) on the screened grid and the fp64 grid of the same points.
 *   1. the (k, omega) grid is marched in fp32 (exterior and boundary algebra in fp64); points at which fp32 cannot vouch
 *      for the sign of D or for the status (|D| < 5e-2 of max(|outer|, |inner|), a pole of D nearby, a coefficient within
 *      1e-3 of a singular point at some node, non-finite result) are marked and re-evaluated in fp64;
 *   2. brackets are detected on the merged array, BOTH ends of every bracket are re-evaluated in fp64 (the determinant
 *      signs at bracket endpoints are fp64 signs) -- a bracket these values do not confirm makes the call return
 *      ES_ERR_SCREENING;
 *   3. refinement and classification in fp64 exactly as es_shoot_find_roots.
 * d_D / d_status (nk x nw, caller allocated) receive the screening result: fp64 values at the re-evaluated points, fp32-
 * accurate values elsewhere (not defined at ES_PT_CONTINUUM points of the band families).
 * h_stats (optional, 3 ints): fp64 re-evaluations of unsure grid points, of bracket ends, unconfirmed brackets. */
int es_shoot_find_roots_mixed(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                              const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent,
                              double* d_D, uint8_t* d_status, es_root_table* table, int* h_count, int* h_stats);

/* The two halves of es_shoot_find_roots_mixed as separate calls (same result when called one after the other on the same
 * arrays): es_shoot_screen_grid enqueues step 1, the fp32 screening march (nothing read back); es_shoot_find_roots_screened
 * runs steps 2 - 5 on the screened d_D / d_status.  A caller that runs several problems on several streams can then order
 * the throughput-bound screening launches one after the other and let the latency-bound remainder of one problem run under
 * the screening of the next (bench.py --workload config4). */
int es_shoot_screen_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk, const double* d_w, int nw,
                         int w_mode, double* d_D, uint8_t* d_status);
int es_shoot_find_roots_screened(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                 const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent,
                                 double* d_D, uint8_t* d_status, es_root_table* table, int* h_count, int* h_stats);

/* es_shoot_find_roots_screened / es_shoot_find_roots_mixed without any host synchronisation: what the synchronous calls
 * return through h_count / h_stats and their status goes to the caller's count words instead.
 * d_counts: int32_t[4] in DEVICE memory, written on the context's stream:
 *   [0] bracket count (may exceed table->capacity, exactly as the d_count of es_shoot_find_roots_async, so that
 *       es_root_table_pack_async(ctx, table, d_counts, ...) works unchanged)
 *   [1] fp64 re-evaluations of unsure grid points                                       (h_stats[0] of the synchronous call)
 *   [2] fp64 re-evaluations of bracket ends = 2 min([0], capacity)                      (h_stats[1])
 *   [3] brackets whose fp64 ends do not confirm them                                    (h_stats[2]; the synchronous call
 *       returns ES_ERR_SCREENING)
 * For the same inputs d_D, d_status and the root table are those of es_shoot_screen_grid + es_shoot_find_roots_screened, bit
 * for bit (the first `capacity` records when [0] > capacity): the synchronous and the asynchronous calls are one pipeline
 * of the same kernels, which all take a count as (d_n, n_max) -- the launch is sized for n_max, the count is min(*d_n, n_max)
 * read on the device, or n_max when d_n is null.  The synchronous call keeps the four words in the context, reads each
 * count back after its scan and launches the next stages for exactly that many (d_n null); here every launch is sized for
 * the grid (nk * nw) or for the table capacity and takes its count from d_counts.  Size the table for the data (about twice
 * the expected count), as for es_shoot_find_roots_async; a capacity above 2^30 is an argument error in all four calls (the
 * bracket-end count is an int32).  Nothing is copied to the host and nothing is synchronised, except that a call which grows the
 * context's scratch (the first one at a larger grid or table capacity) frees and allocates device memory, and hipFree /
 * hipMalloc synchronise.  Scratch of the context: 33 bytes per point for max(nk * nw, 2 capacity) points, plus the
 * bracket-scan scratch of 1/8 + 1/64 bytes per grid cell.
 * Argument errors and ES_ERR_UNSUPPORTED (a slab with per-node sign tracking) are returned at once, as by the synchronous
 * calls, and nothing is enqueued; ES_ERR_CAPACITY and ES_ERR_SCREENING are never returned (the caller reads [0] and [3]).
 * nk * nw == 0 zeroes all four words.  es_shoot_find_roots_mixed_async = es_shoot_screen_grid + the screened call. */
int es_shoot_find_roots_screened_async(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                       const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent,
                                       double* d_D, uint8_t* d_status, es_root_table* table, int32_t* d_counts);
int es_shoot_find_roots_mixed_async(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                                    const double* d_w, int nw, int w_mode, int n_bisect, double tol_percent,
                                    double* d_D, uint8_t* d_status, es_root_table* table, int32_t* d_counts);

/* Audit of the fp32 screening against the fp64 grid, on the device: the check of the EMPIRICAL half of the contract of
 * es_shoot_find_roots_mixed (no fp64 bracket is missed), on the caller's own data.  A pure function of its arrays -- it
 * needs no es_problem and marches nothing; it reads 26 bytes per cell (18 without d_rel64) once.
 *   d_D_scr / d_status_scr: the screened grid, either what es_shoot_screen_grid wrote (unsure points carry the bit
 *     ES_PT_SCREEN_UNSURE in their status) or what es_shoot_find_roots_screened / _mixed left behind (merged: no bit set, so
 *     every point counts as vouched for).  d_D64 / d_status64 / d_rel64: es_shoot_eval_grid (flags = 0) of the same grid.
 * Definitions, with cell c = row * nw + j:
 *   unsure(c)  = status_scr[c] & ES_PT_SCREEN_UNSURE;  vouched(c) = !unsure(c).
 *   merged grid: Dm = unsure ? D64 : D_scr, stm = unsure ? status64 : status_scr -- what the search brackets on (its fp64
 *     re-evaluation of an unsure point gives the value of es_shoot_eval_grid bit for bit).
 *   B(D, st)(c) = j < nw - 1 && st[c] == ES_PT_OK && st[c + 1] == ES_PT_OK && D[c] * D[c + 1] < 0: the bracket predicate of
 *     es_shoot_find_roots (NaN products compare false, the last column is never a bracket, a bracket never spans a row).
 *   kind bits of a cell:  ES_AUDIT_MISSED  B(D64, st64) && !B(Dm, stm)          ES_AUDIT_FALSE  B(Dm, stm) && !B(D64, st64)
 *                         ES_AUDIT_STATUS  vouched && stm != status64
 *                         ES_AUDIT_SIGN    vouched, both statuses ES_PT_OK, signbit(D_scr) != signbit(D64)
 *   compared points: vouched, both statuses ES_PT_OK, D_scr != D64, neither NaN.  Over them
 *     sign margin = fabs(D64) / fabs(D_scr - D64): the factor by which the fp32 error at the point would have to grow to
 *       flip the sign (scale-free; below 1 the sign is wrong);
 *     err = fabs(D_scr - D64) / (fabs(D64) * 100.0 / rel64), where d_rel64 is given, D64 != 0 and rel64 is finite and
 *       positive: the fp32 error in units of max(|outer|, |inner|), the scale the screening threshold 5e-2 is measured in.
 *     A statistic that is itself NaN (inf / inf) is skipped.
 * d_counts (10 words): [0] flagged cells (any kind bit; may exceed capacity), [1] missed, [2] false, [3] status, [4] sign,
 *   [5] points vouched for with both statuses ES_PT_OK, [6] unsure points, [7] fp64 brackets, [8] cell of the minimum
 *   margin (-1: no compared point), [9] cell of the maximum err (-1: none, or d_rel64 == NULL).
 * d_worst (2 doubles): [0] minimum margin (+inf if none), [1] maximum err (0 if none).  Ties go to the smallest cell; counts
 *   are integer sums and the extrema are compared, never accumulated, so the result is reproducible bit for bit.
 * Table: the first min([0], capacity) flagged cells in ascending cell order, d_cell[pos] = c, d_kind[pos] = its kind bits;
 *   entries beyond that are left alone.
 * Asynchronous on the context's stream, nothing is read back; a call that grows the context's scratch (the first one at a
 * larger grid) frees and allocates device memory, which synchronises.  nk * nw == 0: counts 0, cells -1, worst (+inf, 0),
 * ES_SUCCESS (the four grid pointers may then be NULL).  ES_ERR_INVALID_ARG, with nothing enqueued: a null context, nk, nw
 * or capacity negative, nk * nw >= 2^31, a required pointer null, d_cell or d_kind null with capacity > 0. */
enum { ES_PT_SCREEN_UNSURE = 0x80 };   /* status bit es_shoot_screen_grid leaves on points fp32 does not vouch for */
enum { ES_AUDIT_MISSED = 1, ES_AUDIT_FALSE = 2, ES_AUDIT_STATUS = 4, ES_AUDIT_SIGN = 8 };   /* kind bits of a cell */

int es_shoot_audit_screening(es_context* ctx, int nk, int nw,
        const double* d_D_scr, const uint8_t* d_status_scr,      /* nk x nw: the screened grid                 */
        const double* d_D64,  const uint8_t* d_status64,         /* nk x nw: es_shoot_eval_grid, flags = 0      */
        const double* d_rel64 /* may be NULL */,
        int capacity, int64_t* d_cell, uint8_t* d_kind,          /* `capacity` entries each; NULL iff capacity == 0 */
        int64_t* d_counts /* 10 words */, double* d_worst /* 2 doubles */);

/* Refinement rule of the context, read by all six searches above at their refinement step (signatures unchanged).
 *   ES_REFINE_SECTION (default): the rule described at es_shoot_find_roots, R = ceil(n_bisect ln 2 / ln 17) rounds of
 *     17-section and two regula-falsi steps: 16 R + 2 marches per bracket.
 *   ES_REFINE_HYBRID: fixed per bracket like the section rule (nothing in it depends on the bracket count of the call, so a
 *     tiled grid still gives the one-call table).  With S = 1 (kHybridSections):
 *       R <= S: the section rule itself, same launches, same table bit for bit.
 *       otherwise 1. S rounds of 17-section, by the same kernels;
 *                 2. one lane per bracket, at most 8 evaluations of a bracketing secant iteration with Illinois scaling (an
 *                    end retained twice in a row has its D halved); an iterate not strictly inside the bracket is replaced by
 *                    the mid-point; a NaN evaluation ends the phase for the bracket.  Converged: D == 0, or |step| <= 1e-12
 *                    |omega|, or bracket width <= 1e-12 |omega| (independent of n_bisect).  The bracket is KEPT iff converged,
 *                    ES_PT_OK and rel < tol_percent at that iterate: d_w is the iterate that met the test, d_resid its rel,
 *                    [d_w_lo, d_w_hi] the final sign-change bracket (ends inclusive), d_flag = 1;
 *                 3. every bracket not kept is gathered, in order, with the state step 1 left, into a scratch root table, the
 *                    remaining R - S rounds and the two regula-falsi steps run on that table by the same kernels, and the
 *                    rows are scattered back.
 *     What is GUARANTEED: every row with d_flag = 0 and every row that took step 3 is the ES_REFINE_SECTION row, bit for
 *     bit; d_row, d_k and the count are those of the section rule; d_flag is >= the section rule's.  What is EMPIRICAL: that
 *     a root kept by step 2 is the sign change nearest the lower end of the bracket, i.e. the root the section rule
 *     converges to (a bracketing secant iteration may settle on another sign change of the bracket); on the fourteen
 *     test problems every kept root is within 1e-12 relative of the section rule's converged root (n_bisect = 44) and no
 *     kept bracket is one the converged section table rejects (tests/test_refine_hybrid_host.py, tests/refine_hybrid_model.py).
 *     With ES_REFINE_SECTIONS in the environment set to 5 or 9 the searches return ES_ERR_UNSUPPORTED under this rule.
 *     The asynchronous searches stay free of read-backs: every launch is sized for the table capacity and the number of
 *     brackets in step 3 is a device word; the context holds 93 more bytes per table entry of capacity (grown, with
 *     a quarter of head room, as the scratch of es_shoot_find_roots_screened_async is: the first call at a larger capacity
 *     frees and allocates device memory, which synchronises).
 * es_context_set_refine_rule: an unknown rule returns ES_ERR_INVALID_ARG and changes nothing.
 * es_context_refine_stats synchronises the stream, returns four counts summed over the searches since the last call and
 * zeroes them (as es_context_grid_time): h[0] brackets refined by steps 1 - 3 of the hybrid rule, h[1] kept by step 2,
 * h[2] sent to step 3 (h[1] + h[2] = h[0]), h[3] evaluations of step 2.  Marches per bracket =
 * 16 S + h[3] / h[0] + (16 (R - S) + 2) h[2] / h[0]. */
enum { ES_REFINE_SECTION = 0, ES_REFINE_HYBRID = 1 };
int es_context_set_refine_rule(es_context* ctx, int rule);
int es_context_get_refine_rule(const es_context* ctx, int* h_rule);
int es_context_refine_stats(es_context* ctx, int64_t h[4]);

/* Send buffer of the multi-GPU exchange (one all-gather of fixed-capacity buffers per step):
 * d_out is (cap + 1) x 6 doubles, row 0 = (count, valid, 0, ...) with valid = min(count, cap, table->capacity) the number
 * of records that follow, rows 1 .. valid = (k, omega, m, resid, flag, global row) of the first records of `table`, the
 * rest zero.  count > valid: the buffer does not hold every record (the receiver's merge raises).  es_root_table_pack
 * rejects a table shorter than min(count, cap); the _async form, which cannot read the count, reports it through
 * `valid`.  d_rows_global[local row] maps the rows of a k-tile to
 * the rows of the whole grid (NULL: identity).  Replaces the reference's positional pairing of two Queues
 * (Density_cylinder.py:1155-1168).  Asynchronous on the context's stream. */
int es_root_table_pack(es_context* ctx, const es_root_table* table, int count, double m,
                       const int64_t* d_rows_global, int cap, double* d_out);
/* The same with the count in device memory (the d_count of es_shoot_find_roots_async). */
int es_root_table_pack_async(es_context* ctx, const es_root_table* table, const int32_t* d_count, double m,
                             const int64_t* d_rows_global, int cap, double* d_out);

/* ========================================================================================================
 * (3) The reference worker itself: kink(wavenumber, kink_ws, kink_ks, freq) / sausage(...) for a batch of
 *     (wavenumber, freq[]) tasks -- main loop over freq, acceptance test, sign-change detection against the
 *     previously evaluated point, recursive 3-point refinement locate_*() with all of the reference's
 *     bookkeeping (e.g. Cylinder_method_flow_testing.py:554-839; quirks listed in DESIGN.md "worker semantics").
 * ====================================================================================================== */
typedef struct es_worker_spec {
  double tol_percent;              /* xi_tol / p_tol / P_tol                                               */
  int32_t min_len;                 /* refinement needs len(ws) > min_len: 1 slabs (SF-U:518), 2 cylinders (CD-C:680) */
  int32_t itt_cap;                 /* `if itt_num > cap: break`  (100 ... 500)                              */
  int32_t reset_loop_ws_each_iter; /* slab sausage workers clear loop_ws at every main iteration (SF-U:536) */
  int32_t break_on_accept;         /* CR kink workers: `break` after the first accepted grid point (CR-KF:722) */
  int32_t stale_ext_const;         /* CR sausage workers: locate_sausage() uses the enclosing loop's xi_e_const, i.e. the
                                      value at the grid frequency that opened the bracket (CR-SF:558 vs :617)            */
  int32_t main_double_append;      /* CR sausage workers append freq[j] to all_ws twice per main-loop evaluation (CR-SF:684 and
                                      :726): len(all_ws) > 2 holds after two evaluations and the refinement interval
                                      linspace(all_ws[-2], all_ws[-1], 3) is the degenerate [w, w, w]                     */
} es_worker_spec;

/* Task t: wavenumber d_k[t], frequencies d_freq[t*nfreq .. t*nfreq+nfreq).  Roots of task t are written to
 * d_roots[t*max_roots ...] in the order the reference appends them; d_nroots[t] is their number (may exceed
 * max_roots, then ES_ERR_CAPACITY is returned).  Every task is bounded by 3 (itt_cap + 2)(nfreq + 1) evaluations (the
 * reference bounds the recursion by itt_cap only); a task that reaches the bound stops, is marked by a NEGATIVE
 * d_nevals[t] and makes the call return ES_ERR_EVAL_CAP -- its root list is incomplete, never silently truncated.
 * d_nevals[t] (optional) counts the determinant evaluations the
 * reference worker performs for the task (the library itself evaluates fewer points -- it does not re-evaluate the
 * end points of a refinement interval -- and, with several lanes per task, some it never uses). */
int es_worker_run(es_context* ctx, const es_problem* prob, const es_worker_spec* spec,
                  const double* d_k, int ntasks, const double* d_freq, int nfreq,
                  double* d_roots, int32_t* d_nroots, int max_roots, int32_t* d_nevals /* may be NULL */);

/* ========================================================================================================
 * (4) Uniform cylinder in closed form (the limit the reference uses as its benchmark case, profile width 1e5,
 *     e.g. Cylinder_method_flow_testing.py:126): the interior ODE is then Bessel's equation, so the same
 *     determinant follows from I_m/K_m (m_i > 0) or J_m/Y_m (m_i < 0, body modes) of sqrt(|m_i|) r with the
 *     K_m/Y_m admixture fixed by the reference's axis condition at r_axis, matched to the exterior K_m/I_m
 *     solution.  No ODE is integrated.  Same normalisation, status codes and rel as es_shoot_eval_grid.
 * ====================================================================================================== */
typedef struct es_cyl_uniform_params {
  double c_i, vA_i, rho_i, U_i;          /* uniform interior: sound speed, Alfven speed, density, axial flow */
  double rho_e, vA_e, c_e, cT_e;         /* exterior                                                        */
  double r_boundary;                     /* -1 or +1 (sign convention of the reference file)                */
  double r_axis;                         /* |r| of the inner end of the reference's ix grid (0.001 / 0.01)   */
  double L_factor, ic_value, ic_slope;   /* far field of the exterior solve                                  */
  int32_t m, m_ext, axis_bc;             /* ES_AXIS_KINK (P(r_ax) = 0) or ES_AXIS_SAUSAGE (P'(r_ax) = 0)      */
  int32_t reserved;
} es_cyl_uniform_params;

int es_cyl_uniform_eval(es_context* ctx, const es_cyl_uniform_params* p, const double* d_k, int nk,
                        const double* d_w, int nw, int w_mode,
                        double* d_D, double* d_rel /* may be NULL */, uint8_t* d_status);

/* Root search of the closed form over (order, k, omega): the grid is evaluated and searched in ONE pass, without a D array
 * unless the caller asks for it.
 *   Orders: m = m_first + io, 0 <= io < n_orders, 0 <= m_first and m_first + n_orders - 1 <= 64.  The determinant of order m
 *     is that of es_cyl_uniform_eval with p->m = p->m_ext = m (p->m and p->m_ext themselves are ignored); every other field
 *     of p, axis_bc included, is used as given: sausage m = 0 and kink m >= 1 are two calls.
 *   Brackets: D[j] D[j+1] < 0 between omega-neighbours of the same (order, row) with both ends ES_PT_OK, the rule of
 *     es_shoot_find_roots; a bracket never spans a row or an order.  Each wave evaluates 63 cells plus the upper end of the
 *     last one, so the neighbour of every cell comes from the next lane and no point is evaluated twice inside a wave.
 *   Table: order outer, row next, omega inner.  d_row is the k-row index ik, d_order[pos] the order m (d_order has
 *     `capacity` entries and may be NULL only if n_orders <= 1); the other columns mean what they do in es_shoot_find_roots.
 *   Refinement: the ES_REFINE_SECTION rule described at es_shoot_find_roots -- R = ceil(n_bisect ln 2 / ln 17) rounds of
 *     17-section (samples lo + (hi - lo)(j + 1)/17, the new bracket chosen by the first sample whose sign differs from
 *     D(lo), NaN products compare false, a NaN D(lo) is never taken over), two regula-falsi steps, the last secant point is
 *     the root and d_flag = (status == ES_PT_OK && rel < tol_percent) there.  The rule depends neither on the context's
 *     refine rule (ES_REFINE_HYBRID has no meaning here) nor on the bracket count of the call: a grid tiled over calls,
 *     orders or GPUs gives the one-call table, bit for bit.
 *   d_D / d_status (optional, layout [(io * nk + ik) * nw + iw]): exactly what es_cyl_uniform_eval writes for that order.
 *     When both are NULL the call writes nothing of size nk * nw except the bracket masks of the context (1/8 byte per
 *     cell) -- the values at the ends of a bracket are recomputed by the same device function, the same bits.
 *   Count and capacity as in es_shoot_find_roots: *h_count may exceed table->capacity, then ES_ERR_CAPACITY is returned and
 *     the first `capacity` records are written and refined.  n_orders * nk * nw == 0: count 0, ES_SUCCESS.  Argument errors
 *     as es_cyl_uniform_eval.
 * The _async form synchronises nothing and reads nothing back: the count goes to the device word d_count, every launch
 * is sized for the grid or for table->capacity and takes the count from device memory (size the table for the data, as for
 * es_shoot_find_roots_async); ES_ERR_CAPACITY is never returned.  The one exception: a call that grows the bracket-scan
 * scratch of the context (the first one at a larger grid) frees and allocates device memory, which synchronises. */
int es_cyl_uniform_find_roots(es_context* ctx, const es_cyl_uniform_params* p, int m_first, int n_orders,
                              const double* d_k, int nk, const double* d_w, int nw, int w_mode,
                              int n_bisect, double tol_percent,
                              double* d_D /* may be NULL */, uint8_t* d_status /* may be NULL */,
                              es_root_table* table, int32_t* d_order /* capacity entries; may be NULL iff n_orders <= 1 */,
                              int* h_count);
int es_cyl_uniform_find_roots_async(es_context* ctx, const es_cyl_uniform_params* p, int m_first, int n_orders,
                                    const double* d_k, int nk, const double* d_w, int nw, int w_mode,
                                    int n_bisect, double tol_percent,
                                    double* d_D /* may be NULL */, uint8_t* d_status /* may be NULL */,
                                    es_root_table* table, int32_t* d_order, int32_t* d_count);

/* ========================================================================================================
 * (5) Eigenfunctions at given (k, omega) -- the two-region solve the reference's analysis scripts repeat at a
 *     chosen root to plot P_T(r) and xi_r(r) (Cylinder/Non-uniform flow/Coronal/Eigenfunctions/
 *     analysis_cylinder_flow_coronal.py:813-924): interior on the problem's node grid (linspace(x_boundary,
 *     x_end, N)), exterior on linspace(-/+ L*2pi/k, -/+1, n_ext) in closed form.
 *     Cylinders: value = P, flux = xi_r (= xi_e_const P' outside, (C1 P + D P')/C3 inside); slabs: value = Vx,
 *     flux = total pressure P_T.  Both regions are scaled so that the exterior value at the boundary is +-1 (sign
 *     of the reference's amplitude); the reference's plot normalisation (division by max|exterior|) is a host-side
 *     step on these arrays.  Layout: [i * N + j] / [i * n_ext + j] for pair i, node j (node 0 = boundary for the
 *     interior arrays; exterior arrays run from the far field to the boundary).
 *     The pairs need not be roots: the two-region solution is defined at every (k, omega) whose exterior is bound;
 *     flux_ext at the boundary minus flux_int at node 0 is the D of es_shoot_eval_points there (cylinders: up to the
 *     truncation error of the grid -- their interior is integrated from the axis point outwards, the direction in which
 *     the singular solution decays, so for any azimuthal order the arrays are good at the axis node too; the determinant
 *     takes the boundary slope from its own adjoint march).
 *     A pair whose exterior is ES_PT_LEAKY or ES_PT_NONFINITE gets NaN in all four of its value / flux rows; its d_ext_x
 *     row is written as for any other pair, and the rows of the other pairs do not depend on it.  ES_PT_CONTINUUM is
 *     not looked at here: the march steps over the singular point on the fixed grid as the determinant does.
 *     n_ext = 0 skips the exterior (the three exterior pointers may then be NULL), n_ext = 1 is an error; n = 0 is a
 *     successful call that touches nothing.
 * ====================================================================================================== */
int es_shoot_eigenfunction(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                           double* d_int_value, double* d_int_flux,            /* n x N      */
                           int n_ext, double* d_ext_x, double* d_ext_value, double* d_ext_flux /* n x n_ext */);

/* ======================================================================================================
 * (6) Complex frequencies (unstable / Kelvin-Helmholtz modes of the flow slab) -- SURVEY 8f row 3.
 *     Replaces the determinant evaluation and the (Re omega, Im omega) scan of
 *       Slab/Non uniform flow/COMPLEX ANALYSIS/flow_multiprocessor_complex_coronal.py
 *         :348 / :737   sausage / kink(wavenumber, ws, ks, ws_imag, ks_imag, freq)   (6-argument workers)
 *         :369-404      m_e, p_e_const, m0, D, coeff, P_Ti, add_P_Ti with omega = omega_r + i omega_i
 *         :419-456      exterior / interior ODEs, boundary value, total pressures
 *         :1127         driver grid: Re(omega) over a phase-speed band x Im(omega) over [-0.25, 0.25]
 *     in its consistent reading (everything complex; the reference mixes real and imaginary parts, see
 *     DESIGN.md): D_c(k, omega) = p_e V_e'/V_e - P_Ti (Vx' - add Vx) at x = -1, the far-end condition
 *     Vx(+1) = -/+ Vx(-1) imposed by superposition, rel = 100 |D_c| / max(|outer|, |inner|).  Points with
 *     Re(m_e) < 0 are ES_PT_LEAKY (`if m_e.real < 0: pass`, SF-X:405).  Only for ES_GEOM_SLAB_FLOW problems.
 *     variant: ES_CX_SFX = the complex script's formulas (D of SF-X:382, P_T with the U' term of SF-X:401, :455);
 *              ES_CX_SFG = the real script's (D of flow_multiprocessor_coronal.py:421, no U' term): at
 *              Im(omega) = 0 this is es_shoot_eval_* up to the sign normalisation of the exterior amplitude.
 *     Grid layout: [(row * n_im + i_im) * n_re + i_re]; w_mode ES_W_ABSOLUTE: omega = w_re + i w_im;
 *     ES_W_PHASE_SPEED: omega = k (w_re + i w_im).
 *     es_complex_find_roots: a grid cell holds a root if D_c winds once around 0 along its four corners (quadrant
 *     count; cells with a non-finite corner are skipped); each such cell is refined by `n_iter` complex secant
 *     steps from the cell centre; flag = 1 if the final rel < tol_percent and the iterate stayed within two cell
 *     diagonals of the centre.  Ordered by (row, i_im, i_re).
 * ====================================================================================================== */
enum { ES_CX_SFX = 0, ES_CX_SFG = 1 };

int es_complex_eval_grid(es_context* ctx, const es_problem* prob, int variant, const double* d_k, int nk,
                         const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                         double* d_D_re, double* d_D_im, double* d_rel /* may be NULL */, uint8_t* d_status);

int es_complex_eval_points(es_context* ctx, const es_problem* prob, int variant, const double* d_k,
                           const double* d_w_re, const double* d_w_im, int n, double* d_D_re, double* d_D_im,
                           double* d_rel /* may be NULL */, uint8_t* d_status);

typedef struct es_complex_root_table {
  double* d_k;
  double* d_w_re;      /* refined root */
  double* d_w_im;
  double* d_resid;     /* rel (percent) at the refined root */
  int32_t* d_row;
  int32_t* d_flag;     /* 1 accepted, 0 not converged / left the cell neighbourhood (e.g. a pole) */
  int32_t capacity;
} es_complex_root_table;

int es_complex_find_roots(es_context* ctx, const es_problem* prob, int variant, const double* d_k, int nk,
                          const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                          const double* d_D_re, const double* d_D_im, const uint8_t* d_status, int n_iter,
                          double tol_percent, es_complex_root_table* table, int* out_count);

/* Eigenfunctions at given complex (k, omega) -- what the reference's analysis script recomputes at a clicked root
 * (Slab/Non uniform flow/COMPLEX ANALYSIS/complex_imag_flow_analysis.py:998-1013 exterior solve, :1023-1043 interior
 * shoot, :1050-1072 plots of the real and imaginary parts of Vx and P_T over lx U ix), in the consistent reading of this
 * section: everything complex.  Interior on the problem's node grid linspace(-1, +1, N): the adjoint march of D_c gives
 * the boundary slope that meets the far-end condition Vx(+1) = -/+ Vx(-1), a forward RK4 march with the same node /
 * mid-point coefficient sets writes value = Vx and flux = P_T = P_Ti (Vx' - add Vx) at every node (add = 0 for
 * ES_CX_SFG).  Exterior on linspace(-L 2pi/k, -1, n_ext) in closed form, decaying branch: value = Vx_e, flux =
 * p_e Vx_e'.  Both regions are per unit V_e(-1), the normalisation of D_c: the exterior value at the boundary is exactly
 * 1 + 0i, the interior value at node 0 is Omega(-1) / Omega_e, and
 *     exterior flux at the boundary - interior flux at node 0 = D_c
 * of es_complex_eval_points (total pressure is continuous at a root).  The reference's plot normalisation (real and
 * imaginary parts divided by the maxima of the exterior parts, :1009-1043) is a host-side step on these arrays.
 * Complex arrays are interleaved (re, im) pairs of doubles (the layout of a C99 double complex); layout [i * N + j] /
 * [i * n_ext + j] for pair i as in es_shoot_eigenfunction: interior node 0 is the boundary, exterior arrays run from
 * the far field to the boundary.  n_ext is 0 (no exterior) or >= 2.  d_status[i] is the status es_complex_eval_points
 * gives the pair; a pair that is not ES_PT_OK gets NaN in every value and flux entry (its d_ext_x is still written).
 * Asynchronous on the context's stream (with d_status = NULL the first call at a larger n grows the context's scratch,
 * which synchronises).  n == 0 returns ES_SUCCESS and touches nothing. */
int es_complex_eigenfunction(es_context* ctx, const es_problem* prob, int variant,
                             const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                             double* d_int_value, double* d_int_flux,      /* n x N complex      */
                             int n_ext, double* d_ext_x,                   /* n x n_ext real     */
                             double* d_ext_value, double* d_ext_flux,      /* n x n_ext complex  */
                             uint8_t* d_status /* n, may be NULL */);

/* ======================================================================================================
 * (7) Perturbation fields of a cylinder mode, ready for VTK -- the third stage of the reference: its movie / vtk export
 *     scripts turn the eigenfunction (P, xi_r) at a root into xi_phi, xi_z and the velocities and fill an
 *     (r, theta, z, t) mesh in a four-deep Python loop
 *       Cylinder/Non-uniform density/Coronal/Movies/Export_vtk.py            :764-818 amplitudes, :930-950 mesh
 *       Cylinder/Non-uniform flow/Coronal/Movies/Gaussian_flow_export_vtk.py :796-852
 *       Cylinder/Rotational flow/Photospheric/vtk export/v01_p1_kink_export_vtk.py :2179-2238
 *     Cylinders only (the reference has no slab movies), radii POSITIVE as in those scripts.
 *
 *     es_cyl_polarisation: (P, xi_r) -> seven radial amplitudes.  One lane per (mode, radial point), nothing is marched.
 *     The eigenfunction arrays are those es_shoot_eigenfunction writes (interior node 0 = boundary, exterior from the far
 *     field to the boundary).  With
 *       Om = w - m v_phi/r - k v_z        f = m B_phi/r + k B_z        g = m B_z/r + k B_phi
 *       omega_A = m B_phi/r + k bA        omega_A^2, omega_c^2 = omega_A^2 qc   (the determinant's node entries, section 2)
 *       T = f B_phi + rho v_phi Om        Q = -(Om^2 - omega_A^2) rho v_phi^2/r + 2 Om^2 B_phi^2/r + 2 Om B_phi v_phi f/r
 *     interior:
 *       xi_z   = [ f q (Om^2 P - Q xi_r)/(Om^2 rho (Om^2 - omega_c^2)) - (2 Om v_phi B_phi + f v_phi^2) xi_r/r
 *                  - B_phi (g P - 2 B_z T xi_r/r)/(B_z rho (Om^2 - omega_A^2)) ] / (B_phi^2/B_z + B_z)
 *       xi_phi = [ (g P - 2 B_z T xi_r/r)/(rho (Om^2 - omega_A^2)) + B_phi xi_z ] / B_z
 *       v_r = -Om xi_r      v_phi = -Om xi_phi - s_phi r xi_r      v_z = -Om xi_z - s_z xi_r
 *     exterior:
 *       xi_phi = (m P/r)/(rho_e (w^2 - k^2 vA_e^2))     xi_z = k c_e^2 [w^2] P/(rho_e (w^2 - k^2 cT_e^2)(c_e^2 + vA_e^2))
 *       v = -w xi
 *     The interface is neutral about four oddities of the reference, which the caller chooses through the profile arrays
 *     and the flags word:
 *       1. q is the CONSTANT c_i0^2/(c_i0^2 + vA_i0^2) in the scripts, not the local ratio c^2/(c^2 + vA^2);
 *       2. s_z is d(v_z/r)/dr there (Export_vtk.py:812-813), not dv_z/dr;
 *       3. the exterior xi_z carries a factor w^2 the interior expression does not: ES_FIELD_REFERENCE switches it on;
 *       4. the z-components get the angular factor -sin(m theta) (:940): ES_FIELD_Z_REFERENCE_ANGLE of the synthesis.
 *     Output ordering is the reference's spatial = concatenate(ix[::-1], lx[::-1]): n_r = N + n_ext points per mode,
 *     interior from the axis node out to the boundary, then exterior from the boundary out to the far field (the boundary
 *     radius appears twice).  d_radius[i * n_r + j], d_amp[(i * 7 + c) * n_r + j], channels c in the order
 *     xi_r, xi_phi, xi_z, P_T, v_r, v_phi, v_z (ES_AMP_*).
 *     A mode whose eigenfunction rows are NaN (it was not ES_PT_OK) gets NaN in all its amplitudes; its radius row is
 *     written and the other modes do not depend on it.  Nodes where Om^2 - omega_A^2 or Om^2 - omega_c^2 vanish give inf /
 *     NaN at that node only: no guard, as in the reference.  n == 0 is a successful call that touches nothing; n_ext = 0
 *     skips the exterior.  Asynchronous on the context's stream.
 * ====================================================================================================== */
/* Device arrays at the N interior nodes (node 0 = boundary), all required. */
typedef struct es_field_profiles {
  const double* r;                         /* node radii, > 0                                                       */
  const double* rho; const double* Bz; const double* Bphi; const double* vz; const double* vphi;
  const double* bA;                        /* omega_A = m B_phi/r + k bA       (B_z / sqrt(rho))                     */
  const double* qc;                        /* omega_c^2 = omega_A^2 qc         (local c^2/(c^2 + vA^2))              */
  const double* q;                         /* factor of the first term of xi_z (oddity 1)                           */
  const double* s_phi;                     /* d(v_phi/r)/dr                                                         */
  const double* s_z;                       /* dv_z/dr, or d(v_z/r)/dr (oddity 2)                                    */
} es_field_profiles;

enum { ES_AMP_XI_R = 0, ES_AMP_XI_PHI, ES_AMP_XI_Z, ES_AMP_P_T, ES_AMP_V_R, ES_AMP_V_PHI, ES_AMP_V_Z, ES_AMP_COUNT };
enum { ES_FIELD_REFERENCE = 1,             /* es_cyl_polarisation: exterior xi_z with the factor w^2 (oddity 3)      */
       ES_FIELD_Z_REFERENCE_ANGLE = 2,     /* es_cyl_field_synthesis: xi_z, v_z with -sin(m theta) (oddity 4)        */
       ES_FIELD_BIG_ENDIAN = 4 };          /* es_cyl_field_synthesis: every float32 written is byte-swapped          */

int es_cyl_polarisation(es_context* ctx, const double* d_k, const double* d_w, int n,
                        int n_nodes, const double* d_int_value, const double* d_int_flux,           /* n x N      */
                        int n_ext, const double* d_ext_x, const double* d_ext_value, const double* d_ext_flux,
                        const es_field_profiles* profiles, int m, double rho_e, double vA_e, double c_e, double cT_e,
                        int flags, double* d_radius /* n x n_r */, double* d_amp /* n x 7 x n_r */);

/* es_cyl_field_synthesis: amplitudes of ONE mode -> frames on the (r, theta, z, t) mesh (Export_vtk.py:930-950), float32.
 *   d_radius [n_r], d_amp [7 x n_r] as es_cyl_polarisation writes them for one mode; d_theta [n_theta], d_z [n_z],
 *   d_t [n_t].  var_mask selects the variables by bit (ES_VAR_*; the first ten are the reference's varlist order), n_sel
 *   of them, stored in ascending bit order.  With C = cos(k z - w t):
 *     xi_r, P_T, v_r      A(r) cos(m theta) C
 *     xi_phi, v_phi       A(r) (-sin(m theta)) C
 *     xi_x = xi_r cos(theta) - xi_phi sin(theta),  xi_y = xi_r sin(theta) + xi_phi cos(theta);  v_x, v_y likewise
 *     xi_z, v_z           A(r) cos(m theta) C (linear theory), or A(r) (-sin(m theta)) C with ES_FIELD_Z_REFERENCE_ANGLE
 *   v_scale multiplies v_r, v_phi, v_z, v_x and v_y (the rotational script's reading; 1 = physical; the 25 and 400 of the
 *   other scripts are plot scales).  The density perturbation of the scripts is not offered.
 *   d_out [n_t][n_sel][n_z][n_theta][n_r] float32, the radial index fastest: VTK's point order, what
 *   postprocess.write_vtk produces from arrays of shape (n_r, n_theta, n_z).
 *   d_points [n_z][n_theta][n_r][3] = (r cos(theta), r sin(theta), z) float32; NULL skips it.
 *   ES_FIELD_BIG_ENDIAN: every float32 written, points included, is byte-swapped: the buffer is the payload of a
 *   legacy-VTK BINARY file as it stands.
 *   Everything is computed in fp64 and rounded once to fp32.  d_out needs 4-byte alignment only: rows that start on a
 *   16-byte boundary are written with 16-byte stores, the others with 4-byte stores.  Indices are size_t (the
 *   reference's own mesh exceeds 2^31 bytes); n_z * n_theta * n_t and n_r must each be below 2^31.
 *   n_t, n_z, n_theta or n_r == 0: nothing to write, ES_SUCCESS.  An empty or unknown mask is an argument error.
 *   Asynchronous on the context's stream, no host read-back (the first call with larger theta / z / t tables grows the
 *   context's scratch, which synchronises). */
enum { ES_VAR_XI_R = 0, ES_VAR_XI_PHI, ES_VAR_P_T, ES_VAR_V_R, ES_VAR_V_PHI, ES_VAR_XI_X, ES_VAR_XI_Y, ES_VAR_V_X,
       ES_VAR_V_Y, ES_VAR_V_Z, ES_VAR_XI_Z, ES_VAR_COUNT };
int es_cyl_field_synthesis(es_context* ctx, const double* d_radius, const double* d_amp, int n_r,
                           int m, double k, double w,
                           const double* d_theta, int n_theta, const double* d_z, int n_z, const double* d_t, int n_t,
                           uint32_t var_mask, double v_scale, int flags,
                           float* d_points /* may be NULL */, float* d_out);

/* ======================================================================================================
 * (8) Cartesian sampling of a cylinder mode, with its vorticity -- the fourth stage of the reference: its movie and
 *     2-D visualisation scripts flatten the polar mesh of stage three, resample it onto a Cartesian one with
 *     scipy.interpolate.griddata and difference the result with np.gradient
 *       Cylinder/Non-uniform flow/Coronal/Movies/Vorticity_gaussian_flow.py :1190-1262   (and 23 more scripts)
 *     Here r and the angle factors are computed at the Cartesian point itself, only the radial amplitudes are
 *     interpolated, separately on each side of the interface, and curl v is a closed expression.
 *     Two things of the scripts are NOT offered: np.gradient along the (r, theta, z) index axes with unit spacing read as
 *     d/dx, d/dy, d/dz (:1227-1233), and a triangulation across r = boundary, where v_phi and v_z jump.
 *
 *     Convention: the synthesis's linear-theory one (section 7 without ES_FIELD_Z_REFERENCE_ANGLE), C = cos(k z - w t),
 *     S = sin(k z - w t):
 *       v_r = a_r cos(m theta) C        v_phi = a_phi (-sin(m theta)) C        v_z = a_z cos(m theta) C
 *     with a_r, a_phi, a_z the channels ES_AMP_V_R, ES_AMP_V_PHI, ES_AMP_V_Z.  curl v in cylindrical components:
 *       w_r   = sin(m theta) (Wr_C C + Wr_S S)      Wr_C   = -m a_z / r                 Wr_S   = -k a_phi
 *       w_phi = cos(m theta) (Wphi_C C + Wphi_S S)  Wphi_C = -a_z'                      Wphi_S = -k a_r
 *       w_z   = sin(m theta) Wz_C C                 Wz_C   = (m a_r - a_phi - r a_phi') / r
 *     The -sin(m theta) reading of the z-components (ES_FIELD_Z_REFERENCE_ANGLE) has another curl and is not offered:
 *     the flag is an argument error in this section.
 *
 *     es_cyl_vorticity_amplitudes: d_radius [n x n_r], d_amp [n x 7 x n_r] exactly as es_cyl_polarisation writes them,
 *     n_r = n_nodes + n_ext (interior from the axis node out to the boundary, then exterior from the boundary outwards,
 *     the boundary radius twice), d_k [n]  ->  d_vort [(i * 5 + c) * n_r + j], channels c = ES_VORT_*.
 *     One lane per (mode, radial point).  The radial derivatives are DEFINED as np.gradient(a, r, edge_order=2) of each
 *     region on its own, indices [0, n_nodes) and [n_nodes, n_r): with hs, hd the spacings below and above a node,
 *       inside a region   (hs^2 f+ + (hd^2 - hs^2) f0 - hd^2 f-) / (hs hd (hs + hd))
 *       at a region end   the second-order one-sided three-point formula,
 *     both for non-uniform radii.  Nothing is differenced across the interface: the tangential velocity jumps there and
 *     the vortex sheet is not a field value.  A region that is present needs >= 3 points (argument error otherwise);
 *     n_nodes = 0 or n_ext = 0 leaves that region out.  NaN / inf amplitudes reach the nodes whose stencil touches them
 *     and no others.  n == 0 is a successful call that touches nothing.  Asynchronous on the context's stream.
 * ====================================================================================================== */
enum { ES_VORT_R_C = 0, ES_VORT_R_S, ES_VORT_PHI_C, ES_VORT_PHI_S, ES_VORT_Z_C, ES_VORT_COUNT };

int es_cyl_vorticity_amplitudes(es_context* ctx, const double* d_radius /* n x n_r */,
                                const double* d_amp /* n x 7 x n_r */, int n, int n_nodes, int n_ext, int m,
                                const double* d_k /* n */, double* d_vort /* n x 5 x n_r */);

/* es_cyl_cartesian_synthesis: amplitudes of ONE mode -> frames on the (x, y, z, t) mesh, float32.
 *   d_radius [n_r], d_amp [7 x n_r], d_vort [5 x n_r] of one mode (d_vort may be NULL if no vorticity bit is set);
 *   d_x [n_x], d_y [n_y], d_z [n_z], d_t [n_t].  var_mask selects by bit (ES_CVAR_*), n_sel variables stored in ascending
 *   bit order.  At a mesh point r = hypot(x, y), (cos theta, sin theta) = (x / r, y / r), cos(m theta) and sin(m theta)
 *   from those two by angle addition.  With A(r) the interpolated amplitude:
 *     P_T, xi_z, v_z      A cos(m theta) C
 *     xi_x = xi_r cos(theta) - xi_phi sin(theta),  xi_y = xi_r sin(theta) + xi_phi cos(theta)   with
 *                         xi_r = A cos(m theta) C, xi_phi = A (-sin(m theta)) C as in section 7;  v_x, v_y likewise
 *     vort_x = w_r cos(theta) - w_phi sin(theta),  vort_y = w_r sin(theta) + w_phi cos(theta),  vort_z = w_z
 *   v_scale multiplies the velocities and the vorticity.
 *   Region, decided by the tabulated radii:
 *     radius[0] <= r <= radius[n_nodes-1]            interior (a point exactly on the boundary radius is interior)
 *     radius[n_nodes-1] < r <= radius[n_r-1]         exterior
 *     anything else -- the hole inside the axis node, beyond the far field, r = 0, NaN coordinates -- gets `fill` in every
 *     selected variable, as bits (a NaN keeps its payload), byte-swapped if requested.
 *   Inside a region the bracketing nodes of the ascending radii are found by bisection (no spacing is assumed) and every
 *   amplitude is A_j + (A_j+1 - A_j) (r - r_j) / (r_j+1 - r_j); exactly on the last node of a region that node's value.
 *   A region that is present needs >= 3 points; at least one must be present.
 *   d_out [n_t][n_sel][n_z][n_y][n_x] float32, x fastest: the point order of a legacy-VTK RECTILINEAR_GRID.
 *   flags: ES_FIELD_BIG_ENDIAN only.  Everything is computed in fp64 and rounded once.  d_out needs 4-byte alignment only:
 *   the (y, x) points of a z plane are contiguous and are written with 16-byte stores when every plane starts on a
 *   16-byte boundary (n_x n_y a multiple of 4, d_out 16-byte aligned), with 4-byte stores otherwise, the same bits either
 *   way.  Indices are size_t; n_z * n_t must be below 2^31.
 *   n_x, n_y, n_z or n_t == 0: nothing to write, ES_SUCCESS.  An empty or unknown mask, a vorticity bit without d_vort
 *   and a misaligned d_out are argument errors.  Asynchronous on the context's stream, no host read-back (the first call
 *   with larger z / t tables grows the context's scratch, which synchronises). */
enum { ES_CVAR_P_T = 0, ES_CVAR_XI_X, ES_CVAR_XI_Y, ES_CVAR_XI_Z, ES_CVAR_V_X, ES_CVAR_V_Y, ES_CVAR_V_Z, ES_CVAR_VORT_X,
       ES_CVAR_VORT_Y, ES_CVAR_VORT_Z, ES_CVAR_COUNT };
int es_cyl_cartesian_synthesis(es_context* ctx, const double* d_radius, const double* d_amp /* 7 x n_r */,
                               const double* d_vort /* 5 x n_r, may be NULL if no vorticity bit is set */,
                               int n_nodes, int n_ext, int m, double k, double w,
                               const double* d_x, int n_x, const double* d_y, int n_y, const double* d_z, int n_z,
                               const double* d_t, int n_t, uint32_t var_mask, double v_scale, float fill, int flags,
                               float* d_out);

/* The launch shape es_cyl_cartesian_synthesis uses for a mesh (no device work; for tools and tests, as es_shoot_grid_shape):
 * a z plane is cut into `pieces` of 256 points; a frame's n_z planes into z_parts pieces of z_chunk planes (the last one
 * shorter when z_chunk does not divide n_z); the n_t * z_parts (frame, z piece) items go to `groups` workgroups per piece,
 * items_per_group each (the last group shorter when it does not divide them).  All sizes must be positive. */
int es_cyl_cartesian_split(int n_x, int n_y, int n_z, int n_t, int* pieces, int* z_chunk, int* z_parts,
                           int* items_per_group, int* groups);

/* ======================================================================================================
 * (9) Perturbation fields of a slab mode, real or unstable -- stages three and four for the slab families, which the
 *     reference leaves at the two curves (Vx, P_T) (complex_imag_flow_analysis.py:1050-1072).  Equilibrium B0(x) z,
 *     rho(x), U(x) z on |x| <= 1, uniform outside, nothing depends on y; every perturbation is
 *     Re[A(x) e^{i (k z - w t)}] with w = w_re + i w_im and a COMPLEX amplitude A(x).
 *
 *     es_slab_polarisation: (V, Pf) = (value, flux) of es_shoot_eigenfunction (complex_input = 0: real arrays, d_w_im may
 *     be NULL) or of es_complex_eigenfunction (complex_input = 1: interleaved (re, im) pairs) -> six complex amplitudes.
 *     With Om = w - k U, S = c^2 + vA^2, q = c^2/S, cT^2 = c^2 vA^2/S (the reference's P_T is i times the physical
 *     total-pressure amplitude):
 *       v_x    = V                          xi_x = i V / Om                      P_T = -i Pf
 *       xi_z   = k q Pf / (rho (Om^2 - k^2 cT^2))
 *       v_z    = -i (Om xi_z + U' V / Om)
 *       vort_y = i k v_x - d(v_z)/dx        (d_z v_x - d_x v_z)
 *     The exterior uses rho_e, c_e, vA_e, U_e and U' = 0.  ES_SLAB_FIELD_SHEAR_PT first adds (F/Om)(k U'/Om) V to the
 *     interior Pf, F = rho S (Om^2 - k^2 cT^2)/(Om^2 - k^2 c^2): the flux of linear theory, where SF-G's determinant has
 *     (F/Om) Vx' alone.  (The ES_CX_SFX flux carries that term already: do not set the flag for it.)
 *     Table of a mode: n_tab = 2 n_ext + N abscissae, ascending -- left exterior [-R, -1] as d_ext_x gives it, interior
 *     x_j = -1 + j (2/(N-1)) with x_{N-1} = +1 (numpy.linspace), right exterior [1, R], the mirror image of the left one
 *     under the far-end condition Vx(+1) = sigma Vx(-1), sigma = -1 (ES_SLAB_MODE_SAUSAGE) / +1 (ES_SLAB_MODE_KINK):
 *     v_x, xi_x, vort_y take the factor sigma, P_T, xi_z, v_z the factor -sigma.  Each boundary abscissa appears twice.
 *     d_x[i * n_tab + j]; d_amp[((i * 6 + c) * n_tab + j) * 2 + {0: re, 1: im}], channels c = ES_SAMP_*.
 *     d(v_z)/dx is np.gradient(a, x, edge_order=2), coefficient form and order of operations as in section 8, of the real
 *     and the imaginary part separately and of each of the three regions on its own -- never across x = -1 or +1, where
 *     v_z jumps -- in a second launch of the same call.  N >= 3; n_ext = 0 leaves both exteriors out, n_ext = 1 or 2 is
 *     an argument error.
 *     A mode whose eigenfunction rows are NaN gets NaN amplitudes (complex NaNs: with real input a part that is
 *     identically zero stays zero; every value synthesised from them is NaN); its d_x row is written and the other modes
 *     do not depend on it.  Nodes where Om, Om^2 - k^2 cT^2 or Om^2 - k^2 c^2 vanish give inf / NaN at the nodes their stencil
 *     touches and nowhere else: no guard, as in section 7.  n == 0 touches nothing.  Asynchronous on the context's stream.
 * ====================================================================================================== */
/* Device arrays at the N interior nodes (node 0 is x = -1), all required. */
typedef struct es_slab_field_profiles {
  const double* rho; const double* c2; const double* vA2; const double* U; const double* dU;
} es_slab_field_profiles;

enum { ES_SAMP_XI_X = 0, ES_SAMP_XI_Z, ES_SAMP_P_T, ES_SAMP_V_X, ES_SAMP_V_Z, ES_SAMP_VORT_Y, ES_SAMP_COUNT };
enum { ES_SLAB_FIELD_SHEAR_PT = 1 };       /* es_slab_polarisation: Pf += (F/Om)(k U'/Om) V before anything is formed */

int es_slab_polarisation(es_context* ctx, const double* d_k, const double* d_w_re,
                         const double* d_w_im /* may be NULL: real modes */, int n,
                         int n_nodes, const double* d_int_value, const double* d_int_flux,    /* n x N [x 2]       */
                         int n_ext, const double* d_ext_x /* n x n_ext */,
                         const double* d_ext_value, const double* d_ext_flux,                 /* n x n_ext [x 2]   */
                         int complex_input, const es_slab_field_profiles* profiles,
                         double rho_e, double vA_e, double c_e, double U_e, int parity /* ES_SLAB_MODE_* */, int flags,
                         double* d_x /* n x n_tab */, double* d_amp /* n x 6 x n_tab x 2 */);

/* es_slab_field_synthesis: the table of ONE mode -> frames on the (x, z, t) mesh, float32.
 *   d_xtab [n_tab], d_amp [6 x n_tab x 2] as es_slab_polarisation writes them for one mode, n_tab = 2 n_ext + n_nodes;
 *   d_x [n_x], d_z [n_z], d_t [n_t].  var_mask selects by bit (ES_SVAR_*), n_sel variables stored in ascending bit order.
 *   With E = e^{w_im t}, C = cos(k z - w_re t), S = sin(k z - w_re t) and A the interpolated amplitude the value is
 *     E (A_re C - A_im S)         (formed as A_re (E C) - A_im (E S), fp64, rounded once to float32)
 *   v_scale multiplies v_x, v_z and vort_y.
 *   Region, decided by the tabulated abscissae (-R = xtab[0], -1 = xtab[n_ext], +1 = xtab[n_ext + N - 1], R = last):
 *     -1 <= x <= 1     interior            -R <= x < -1     left exterior            1 < x <= R     right exterior
 *   Inside a region the bracketing points are found by bisection (no spacing is assumed) and the real and the imaginary
 *   part are A_j + (A_j+1 - A_j) (x - x_j) / (x_j+1 - x_j); exactly on the last node of a region that node's value.
 *   Everything else -- points outside [-R, R], NaN coordinates, an exterior that is absent -- gets `fill` in every
 *   selected variable, as bits (a NaN keeps its payload), byte-swapped if requested.
 *   d_out [n_t][n_sel][n_z][n_x] float32, x fastest: with y = [0] the point order of a legacy-VTK RECTILINEAR_GRID.
 *   flags: ES_FIELD_BIG_ENDIAN only.  d_out needs 4-byte alignment only: rows are written with 16-byte stores when every
 *   row starts on a 16-byte boundary (n_x a multiple of 4, d_out 16-byte aligned), with 4-byte stores otherwise, the same
 *   bits either way.  Indices are size_t; n_z * n_t and n_x must each be below 2^31.
 *   n_x, n_z or n_t == 0: nothing to write, ES_SUCCESS.  An empty or unknown mask, n_nodes < 3, n_ext of 1 or 2 and a
 *   misaligned d_out are argument errors.  Asynchronous on the context's stream, no host read-back (the first call with a
 *   larger (z, t) table grows the context's scratch, which synchronises). */
enum { ES_SVAR_XI_X = 0, ES_SVAR_XI_Z, ES_SVAR_P_T, ES_SVAR_V_X, ES_SVAR_V_Z, ES_SVAR_VORT_Y, ES_SVAR_COUNT };
int es_slab_field_synthesis(es_context* ctx, const double* d_xtab, const double* d_amp /* 6 x n_tab x 2 */,
                            int n_nodes, int n_ext, double k, double w_re, double w_im,
                            const double* d_x, int n_x, const double* d_z, int n_z, const double* d_t, int n_t,
                            uint32_t var_mask, double v_scale, float fill, int flags, float* d_out);

/* ======================================================================================================
 * (10) Branch label of a root: the radial node count of its eigenfunction.  The grid search returns a cloud of (k, omega)
 *     and every stage after it (sections 5, 7, 8, 9) takes ONE chosen root; the reference cuts the cloud into branches by
 *     hand, with phase-speed bands and cut-offs picked per data set
 *       Cylinder/Non-uniform flow/Coronal/Eigenfunctions/analysis_cylinder_flow_coronal.py :244-372
 *     (fast_sausage_branch1/2/3, slow_body_kink, ...).  What those cuts stand for is the pair (sign changes of value, sign
 *     changes of flux) over the interior nodes, with whether the mode peaks at the interface (surface-like) or inside
 *     (body): constant along a dispersion branch, different between neighbouring branches.
 *
 *     es_shoot_mode_signature: one (k, omega) pair per lane, the interior algorithm of es_shoot_eigenfunction (cylinders:
 *     two columns from the axis node out to the boundary, then the state marched out again; slabs: adjoint march, then the
 *     forward march) with `value` and `flux` exactly as section 5 defines them -- but nothing is written per node: the rows
 *     are reduced in registers and each pair gets one entry per output.
 *       d_nodes_value / d_nodes_flux [n]: sign changes of the row over the N interior nodes in output order (node 0 =
 *         boundary).  Entries that are exactly zero or NaN are skipped (the kink axis node of an untwisted cylinder is
 *         exactly 0.0: its target is 0); a change is counted whenever the sign of an entry differs from the sign of the last
 *         entry that was kept.
 *       d_peak_value / d_peak_flux [n]: max |entry| over the N nodes in the normalisation of section 5 (exterior value at
 *         the boundary = +-1; NaN entries are skipped, a row without any other entry gives NaN and node -1);
 *         d_peak_node_value / d_peak_node_flux [n]: the smallest node index that attains it.  peak_value = 1 at node 0 for
 *         a cylinder: the pressure perturbation is largest on the interface.
 *       d_status [n]: ES_PT_* of the exterior as es_shoot_eigenfunction sees it (ES_PT_OK, ES_PT_LEAKY, ES_PT_NONFINITE;
 *         ES_PT_CONTINUUM is not looked at, as in section 5).  A pair that is not ES_PT_OK gets -1 in the four integer
 *         outputs and NaN in the two peaks; the other pairs do not depend on it.
 *     Any of the seven output pointers may be NULL: that output is skipped.
 *     d_count (may be NULL): a device word holding the number of valid pairs -- the d_count of es_shoot_find_roots_async or
 *     d_counts[0] of the screened searches, with table->d_k / table->d_w as the pairs.  The launch is sized for n, the
 *     kernel uses min(max(*d_count, 0), n) and entries beyond it are left alone: no read-back between search and labels.
 *     Asynchronous on the context's stream, no host synchronisation.  n == 0 succeeds and touches nothing (the arrays may
 *     then be NULL).  ES_ERR_INVALID_ARG: n < 0, a null problem, d_k or d_w null with n > 0; ES_ERR_UNSUPPORTED: an unknown
 *     family.  Not offered: complex frequencies (section 6), the closed-form uniform cylinder (section 4) and the exterior
 *     -- the closed-form exterior of a bound mode has no node of interest.
 * ====================================================================================================== */
int es_shoot_mode_signature(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                            const int32_t* d_count /* may be NULL */,
                            int32_t* d_nodes_value, int32_t* d_nodes_flux,
                            int32_t* d_peak_node_value, int32_t* d_peak_node_flux,
                            double* d_peak_value, double* d_peak_flux, uint8_t* d_status);

/* ======================================================================================================
 * (11) Dispersion slopes of a root: the exact partial derivatives of the boundary determinant.  With D(k, omega) the
 *     determinant es_shoot_eval_points returns, D_w = dD/d omega and D_k = dD/dk give at a root
 *       the group speed            c_g = d omega / dk = -D_k / D_w,
 *       the Newton correction      d omega = -D / D_w   (the acceptance residual as an error bar in omega),
 *       D_w itself, the weight of the mode in an initial-value problem.
 *     The reference's analysis scripts fit polynomials through hand-cut branches for this (np.polyfit, e.g.
 *       Cylinder/Non-uniform flow/Coronal/Eigenfunctions/analysis_cylinder_flow_coronal.py);
 *     difference quotients of section 2 need a step, and no fixed step is right both at a regular root and at a root beside
 *     a pole of the exterior term.
 *
 *     es_shoot_root_slopes: one (k, omega) pair per lane; the adjoint march, the closed-form exterior and the boundary
 *     algebra of es_shoot_eval_points carried in 3-component jets (value, d/d omega, d/dk) -- a tangent-linear evaluation,
 *     exact to rounding, no step to choose.
 *       d_outer / d_inner [3][n]: row 0 the value, row 1 d/d omega, row 2 d/dk of the two sides of the matching condition
 *         (cylinders: xi_e and xi_i at the boundary; slabs: the total pressure outside and inside).  D = outer - inner is
 *         the D of es_shoot_eval_points (same march; the reciprocals are grouped per RK4 step), D_w and D_k are the
 *         differences of rows 1 and 2.  The rows are n apart, n the argument, whatever d_count holds.
 *       d_status [n]: ES_PT_* of the exterior as in sections 5 and 10 (ES_PT_OK, ES_PT_LEAKY, ES_PT_NONFINITE;
 *         ES_PT_CONTINUUM is not looked at).  A pair whose exterior is not ES_PT_OK, or one of whose six outputs is not
 *         finite, gets NaN in all six; the other pairs do not depend on it.
 *     Any of the three output pointers may be NULL: that output is skipped.
 *     d_count (may be NULL): as in section 10 -- the device count word of an _async search; the kernel uses
 *     min(max(*d_count, 0), n) and leaves entries beyond it alone.
 *     Asynchronous on the context's stream, no host synchronisation.  n == 0 succeeds and touches nothing (the arrays may
 *     then be NULL).  ES_ERR_INVALID_ARG: n < 0, a null problem, d_k or d_w null with n > 0; ES_ERR_UNSUPPORTED: an unknown
 *     family.  Not offered: the closed-form uniform cylinder (section 4).  Complex frequencies (section 6) have their own
 *     call, es_complex_root_slopes of section 12.
 * ====================================================================================================== */
int es_shoot_root_slopes(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                         const int32_t* d_count /* may be NULL */,
                         double* d_outer /* [3][n]: value, d/dw, d/dk */, double* d_inner /* [3][n] */,
                         uint8_t* d_status);

/* ======================================================================================================
 * (12) Slopes and Newton tracing of complex roots of the flow slab (the unstable, Kelvin-Helmholtz modes of section 6).
 *     D_c(k, omega) of es_complex_eval_points is holomorphic in omega; with D_w = dD_c/d omega and D_k = dD_c/dk (k real)
 *       d omega / dk = -D_k / D_w:  the real part is the group speed, the imaginary part the slope of the growth rate,
 *                                   whose zero marks the most unstable wavenumber;
 *       -D_c / D_w              :  the Newton correction, quadratic because D_c is holomorphic (section 6 takes 12 secant
 *                                   steps from a cell centre).
 *     Both calls take `variant` and the problem as section 6 does (ES_GEOM_SLAB_FLOW only) and report what it reports for a
 *     bad variant (ES_ERR_INVALID_ARG) or another geometry (ES_ERR_UNSUPPORTED).  Both are asynchronous on the context's
 *     stream, no host synchronisation; n == 0 succeeds and touches nothing (the arrays may then be NULL).  d_count (may be
 *     NULL): as in section 10 -- the kernels use min(max(*d_count, 0), n) and leave entries beyond it alone.
 *
 *     es_complex_root_slopes: one (k, omega) pair per lane; the coefficient functions, the adjoint RK4 march, the closed-form
 *     exterior and the boundary algebra of es_complex_eval_points carried in jets of three complex components (value,
 *     d/d omega, d/dk) -- exact to rounding, no step to choose (beside a critical layer no difference step is safe,
 *     DESIGN.md section 8g).
 *       d_outer / d_inner [3][n][2]: (re, im) pairs; row 0 the value, row 1 d/d omega, row 2 d/dk of the total pressure
 *         outside and inside.  outer - inner of row 0 is the D_c of es_complex_eval_points (the same operations in the same
 *         order); D_w and D_k are the differences of rows 1 and 2.  The rows are n apart, whatever d_count holds.
 *       d_status [n]: the status es_complex_eval_points gives the pair.  A pair whose status is not ES_PT_OK, or one of
 *         whose six outputs is not finite, gets NaN in all six; the other pairs do not depend on it.
 *     Any of the three output pointers may be NULL: that output is skipped.
 *     ES_ERR_INVALID_ARG: n < 0, a null problem, d_k, d_w_re or d_w_im null with n > 0.
 *
 *     es_complex_newton: one guess per lane, Newton's iteration in omega at fixed k:
 *         w = guess; iters = 0; ok = true
 *         repeat max_iter times:
 *             D, D_w, status at w
 *             if status != ES_PT_OK or D, D_w not finite or D_w == 0:  ok = false; stop
 *             s = -D / D_w;  if |s| > step_cap: s *= step_cap / |s|
 *             w += s; iters += 1
 *             if |s| <= 1e-14 max(1, |w|): stop
 *         at the final w:  resid = 100 |D| / max(|outer|, |inner|),  dwdk = -D_k / D_w,  status
 *         flag = ok && status == ES_PT_OK && resid < tol_percent && |w - guess| <= max_shift
 *       d_w_re, d_w_im, d_resid, d_iters, d_flag [n]; d_dwdk [n][2] (re, im; may be NULL).  w is reported whatever the flag;
 *       resid and dwdk are NaN where the final status is not ES_PT_OK.  max_iter == 0 is the final evaluation alone: the
 *       guess with its resid and slope.  Pass DBL_MAX for no step_cap / max_shift.
 *       At a branch point -- where a conjugate pair of roots meets on the real axis -- D_w = 0: dwdk is then not finite
 *       and the iteration stops with ok = false if it lands there exactly; nothing else is done about it.
 *     ES_ERR_INVALID_ARG: n < 0, max_iter < 0, step_cap, max_shift or tol_percent not positive, a null problem, any array
 *     but d_count and d_dwdk null with n > 0.
 * ====================================================================================================== */
int es_complex_root_slopes(es_context* ctx, const es_problem* prob, int variant,
                           const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                           const int32_t* d_count /* may be NULL */,
                           double* d_outer /* [3][n][2]: value, d/dw, d/dk; (re, im) pairs */,
                           double* d_inner /* [3][n][2] */, uint8_t* d_status);

int es_complex_newton(es_context* ctx, const es_problem* prob, int variant,
                      const double* d_k, const double* d_guess_re, const double* d_guess_im, int n,
                      const int32_t* d_count /* may be NULL */,
                      int max_iter, double step_cap, double max_shift, double tol_percent,
                      double* d_w_re, double* d_w_im, double* d_resid,
                      double* d_dwdk /* [n][2], may be NULL */, int32_t* d_iters, int32_t* d_flag);

/* ======================================================================================================
 * (13) Newton tracing of real roots: the shooting determinant of section 2, all four families.  Section 11 delivers D, D_w and
 *     D_k at a pair; this call iterates with them.  A coarse scan gives every branch with its label (section 10) and its
 *     group speed (section 11); a piecewise-cubic Hermite prediction through those roots is then within ~1e-3 of the curve
 *     at any k in between, and Newton with the exact D_w reaches the root in 3 - 5 steps -- a dispersion curve on thousands
 *     of wavenumbers without marching and bracketing a (k, omega) grid of that many rows.
 *
 *     es_shoot_newton: one guess per lane, Newton's iteration in omega at fixed k:
 *         w = guess; iters = 0; ok = true
 *         repeat max_iter times:
 *             outer, inner with d/dw at (k, w), exterior status       (the march of section 11 in (value, d/d omega) jets)
 *             D = outer - inner, D_w likewise
 *             if status != ES_PT_OK or D, D_w not finite or D_w == 0:  ok = false; stop
 *             s = -D / D_w;  if |s| > step_cap: s = copysign(step_cap, s)
 *             w += s; iters += 1
 *             if |s| <= 1e-14 |w|: stop            (relative alone: the rule does not depend on the unit of omega; section
 *                                                   12's complex rule still has the floor max(1, |w|))
 *         at the final w (the jets of section 11, and the continuum looked at):
 *             scale = |outer| (problems with accept_norm) or max(|outer|, |inner|)        -- the rel of section 2
 *             resid = 100 |D| / scale,  dwdk = -D_k / D_w,  status
 *         flag = ok && status == ES_PT_OK && resid < tol_percent && |w - guess| <= max_shift
 *       d_w, d_resid, d_iters, d_flag [n]; d_dwdk [n] and d_status [n] may be NULL.  w is reported whatever the flag.
 *       d_status is the status es_shoot_eval_points gives the final pair, ES_PT_CONTINUUM included (bands where the problem
 *       has them, sign tracking otherwise, selected as in section 2); resid and dwdk are NaN where it is ES_PT_LEAKY or
 *       ES_PT_NONFINITE.  max_iter == 0 is the final evaluation alone: w = guess with its resid and slope, resid formed
 *       from the outer and inner es_shoot_root_slopes returns for the pair.  Pass DBL_MAX for no step_cap / max_shift.
 *       Beside a pole of the exterior term (DESIGN.md sections 8f, 9) the iteration steps away from the pole: for
 *       f = c / (x - p) the Newton step is x - p.  Where two roots of a row merge D_w = 0: dwdk is then not finite and the
 *       iteration stops with ok = false if it lands there exactly.
 *     The lanes do not depend on each other: a leaky or non-finite guess changes nothing beside it.
 *     d_count (may be NULL): as in sections 10 - 12 -- the kernel uses min(max(*d_count, 0), n) and leaves entries beyond it
 *     alone.  Asynchronous on the context's stream, no host read-back.  n == 0 succeeds and touches nothing (the arrays may
 *     then be NULL).  ES_ERR_INVALID_ARG: n < 0, max_iter < 0, step_cap, max_shift or tol_percent not positive, a null
 *     problem, any array but d_count, d_dwdk and d_status null with n > 0; ES_ERR_UNSUPPORTED: an unknown family.  Not
 *     offered: the closed-form uniform cylinder (section 4), second derivatives, continuation in a parameter other than k.
 * ====================================================================================================== */
int es_shoot_newton(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_guess, int n,
                    const int32_t* d_count /* may be NULL */, int max_iter, double step_cap, double max_shift,
                    double tol_percent, double* d_w, double* d_resid, double* d_dwdk /* may be NULL */,
                    int32_t* d_iters, int32_t* d_flag, uint8_t* d_status /* may be NULL */);

/* ======================================================================================================
 * (14) Complex frequencies on the untwisted cylinder: the determinant of section 2 at omega = omega_r + i omega_i and its
 *     root search -- the unstable (Kelvin-Helmholtz) modes of a cylinder whose axial jet is fast enough, where the root leaves
 *     the real axis and sections 2 and 13 find nothing.  ES_GEOM_CYLINDER problems only (non-uniform density or axial flow,
 *     any m, both axis conditions, both signs of r); every other geometry gets ES_ERR_UNSUPPORTED (the flow slab has
 *     section 6, whose calls in turn keep refusing cylinders; the twisted cylinder has section 17).  Values only (DESIGN.md
 *     section 8i).
 *     What is computed: the interior of section 2 -- the same node grid, the same coefficient formulas, one classical RK4
 *     step per interval, the adjoint row march, the axis condition by superposition -- in complex arithmetic, and the
 *     exterior P_e = a I_m(mu |r|) + b K_m(mu |r|) with mu = principal sqrt(m_e), K and I at complex argument, the
 *     reference's far-field initial values.  The exterior solution is normalised by its own complex boundary value,
 *     P_e(boundary) = 1 (section 2 divides by |P_e| and keeps a sign), so at omega_i = 0
 *         D_c = sign(P_e(boundary)) D of es_shoot_eval_points,    Im D_c = 0.
 *     outer = xi_e, inner = xi_i, D_c = outer - inner, rel = 100 |D_c| / max(|outer|, |inner|) (|outer| alone for problems
 *     with accept_norm).  D_c(k, conj omega) = conj D_c(k, omega).
 *     Status: ES_PT_LEAKY where Re(m_e) < 0 (the rule of section 6, and of section 2 on the real axis; it keeps mu in the
 *     sector |arg mu| <= pi/4); ES_PT_NONFINITE where m_e, xi_e_const or the result is not finite.  ES_PT_CONTINUUM is never
 *     reported: off the real axis the coefficients have no zero on the grid, and on it callers have section 2.  D_c, rel,
 *     outer and inner are NaN unless the status is ES_PT_OK.
 *     Grid layout, w_mode, the cell rule, the secant refinement, the flag, the order of the table, es_complex_root_table and
 *     the capacity convention (ES_ERR_CAPACITY with the full count in *out_count and the first `capacity` records written)
 *     are those of section 6; argument checks likewise, without `variant`.  A call with no points (a zero size) succeeds and
 *     touches nothing.  The eval calls are asynchronous on the context's stream; es_cyl_complex_find_roots synchronises.
 *     es_cyl_complex_eval_points: d_outer, d_inner (each may be NULL) receive the two sides as interleaved (re, im) pairs [n].
 * ====================================================================================================== */
int es_cyl_complex_eval_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                             const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                             double* d_D_re, double* d_D_im, double* d_rel /* may be NULL */, uint8_t* d_status);

int es_cyl_complex_eval_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                               const double* d_w_im, int n, double* d_D_re, double* d_D_im,
                               double* d_rel /* may be NULL */, uint8_t* d_status,
                               double* d_outer /* [n][2], may be NULL */, double* d_inner /* [n][2], may be NULL */);

int es_cyl_complex_find_roots(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                              const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                              const double* d_D_re, const double* d_D_im, const uint8_t* d_status, int n_iter,
                              double tol_percent, es_complex_root_table* table, int* out_count);

/* ======================================================================================================
 * (15) Slopes and Newton tracing of complex roots of the untwisted cylinder (the unstable modes of section 14): what section
 *     12 is to section 6.  D_c(k, omega) of es_cyl_complex_eval_points is holomorphic in omega; with D_w = dD_c/d omega and
 *     D_k = dD_c/dk (k real)
 *       d omega / dk = -D_k / D_w:  the real part is the group speed, the imaginary part the slope of the growth rate,
 *                                   whose zero marks the most unstable wavenumber;
 *       -D_c / D_w              :  the Newton correction, quadratic because D_c is holomorphic (section 14 takes 12 secant
 *                                   steps from a cell centre, plus the grid row that found the cell).
 *     Both calls take the problem as section 14 does: ES_GEOM_CYLINDER only, every other geometry -- the twisted cylinder,
 *     which has sections 17 and 18 for this, and the slabs -- gets ES_ERR_UNSUPPORTED.  Both are asynchronous on the
 *     context's stream with no host read-back; n == 0 succeeds and touches nothing (the arrays may then be NULL).  d_count
 *     (may be NULL): as in sections 10 - 13 -- the kernels use min(max(*d_count, 0), n) and leave entries beyond it alone.
 *
 *     es_cyl_complex_root_slopes: one (k, omega) pair per lane; the node entries, the coefficients, the adjoint RK4 march,
 *     the Bessel exterior and the boundary algebra of section 14 -- the same program text -- carried in jets of three complex
 *     components (value, d/d omega, d/dk); K_n and I_n carry their argument derivative by the recurrence identities.  Exact
 *     to rounding, no step to choose.
 *       d_outer / d_inner [3][n][2]: (re, im) pairs; row 0 the value, row 1 d/d omega, row 2 d/dk of xi_e and xi_i.  Row 0
 *         is the outer and inner of es_cyl_complex_eval_points, the section-14 value; D_w and D_k are the differences of
 *         rows 1 and 2.  The rows are n apart, whatever d_count holds.
 *       d_status [n]: the status section 14 gives the pair; ES_PT_NONFINITE also where a derivative of outer or inner is
 *         not finite.  A pair whose status is not ES_PT_OK gets NaN in all six outputs; the other pairs do not depend on it.
 *     Any of the three output pointers may be NULL: that output is skipped.
 *     ES_ERR_INVALID_ARG: n < 0, a null problem, d_k, d_w_re or d_w_im null with n > 0.
 *
 *     es_cyl_complex_newton: one guess per lane, the iteration of es_complex_newton (section 12) step for step, with
 *         resid = the rel of section 14 at the final w: 100 |D_c| / max(|outer|, |inner|), |outer| alone for problems with
 *         accept_norm.
 *       d_w_re, d_w_im, d_resid, d_iters, d_flag [n]; d_dwdk [n][2] (re, im; may be NULL).  w is reported whatever the flag;
 *       resid and dwdk are NaN where the final status is not ES_PT_OK.  max_iter == 0 is the final evaluation alone: the
 *       guess with its resid and slope.  Pass DBL_MAX for no step_cap / max_shift.
 *       At a branch point -- where a conjugate pair of roots meets on the real axis, the onset of the instability --
 *       D_w = 0: dwdk is then not finite and the iteration stops with ok = false if it lands there exactly; nothing else is
 *       done about it.  On the real axis d omega / dk is real: the group speed of section 11.
 *     ES_ERR_INVALID_ARG: n < 0, max_iter < 0, step_cap, max_shift or tol_percent not positive, a null problem, any array
 *     but d_count and d_dwdk null with n > 0.
 *     Not offered: second derivatives.  (Slopes and Newton tracing on the twisted cylinder: section 18.)
 *     (Eigenfunctions and fields at complex roots: section 16.)
 * ====================================================================================================== */
int es_cyl_complex_root_slopes(es_context* ctx, const es_problem* prob,
                               const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                               const int32_t* d_count /* may be NULL */,
                               double* d_outer /* [3][n][2]: value, d/dw, d/dk; (re, im) pairs */,
                               double* d_inner /* [3][n][2] */, uint8_t* d_status);

int es_cyl_complex_newton(es_context* ctx, const es_problem* prob,
                          const double* d_k, const double* d_guess_re, const double* d_guess_im, int n,
                          const int32_t* d_count /* may be NULL */,
                          int max_iter, double step_cap, double max_shift, double tol_percent,
                          double* d_w_re, double* d_w_im, double* d_resid,
                          double* d_dwdk /* [n][2], may be NULL */, int32_t* d_iters, int32_t* d_flag);

/* ======================================================================================================
 * (16) Eigenfunctions and perturbation fields of complex cylinder roots (the unstable modes of sections 14 and 15): what
 *     sections 5 and 7 are to section 2 -- P(r), xi_r(r), the seven amplitudes and growing float32 frames for VTK.
 *     es_cyl_complex_eigenfunction takes the problem as sections 14 / 15 do: ES_GEOM_CYLINDER only, every other geometry gets
 *     ES_ERR_UNSUPPORTED.  DESIGN.md section 8k.
 *
 *     es_cyl_complex_eigenfunction: the signature of es_complex_eigenfunction (section 6) without `variant`, the layout of
 *     section 5: interior node 0 is the boundary; the exterior runs from the far field to the boundary on
 *     linspace(-/+R, -/+1, n_ext) with the last point exactly -/+1 (both signs of r are accepted).  value = P, flux = xi_r:
 *     inside xi_r = Xi / r, outside xi_r = xi_e_const P_e'.  Complex arrays are interleaved (re, im) pairs.
 *       Interior: the algorithm of section 5 for cylinders in complex arithmetic.  Both RK4 marches run from the axis node
 *       outwards on the node / mid-point coefficient sets of section 14 (one complex division per node): the first carries
 *       the columns e = (1, 0) and d to the boundary -- ES_AXIS_KINK: d = (0, 1), target = bc_const xi_e; ES_AXIS_SAUSAGE:
 *       d = (a12, -a11), target = 0 --, beta follows from P(r_b) = P_b, the second march writes every node from the axis
 *       state target e + beta d.
 *       Exterior: P_e(x) = [b_s K_m(mu |x|) + E2x a_s I_m(mu |x|)] e^{-(mu |x| - mu)} / Pv with the scaled Bessel functions,
 *       a_s, b_s and Pv of section 14, mu the principal square root; where Re(xR - xb) >= 40 the I part is dropped at every
 *       point, as section 14 drops it at the boundary.
 *       Normalisation: that of section 14, P_e(boundary) = 1 + 0i.  So the exterior value at the boundary is exactly 1, the
 *       interior value at node 0 is 1 to rounding (beta imposes it), the exterior flux at the boundary is the `outer` of
 *       es_cyl_complex_eval_points, and
 *           exterior flux at the boundary - interior flux at node 0 = D_c.
 *       The adjoint RK4 row march of the determinant is J (outward RK4 march) J^-1 for the trace-free coefficient matrix,
 *       so the two agree exactly where the axis target is zero: ES_AXIS_SAUSAGE, and ES_AXIS_KINK with bc_const = 0, which
 *       is every untwisted reference problem.  There this holds to rounding (2e-15 of max(|outer|, |inner|) measured), not
 *       only to truncation as in section 5.  With a non-zero target the two differ by (det S - 1) target / p2, S the
 *       discrete outward transfer matrix, whose determinant RK4 keeps at 1 to truncation only (section 19).
 *       d_status[i] (may be NULL) is the status section 14 gives the pair: ES_PT_OK, ES_PT_LEAKY or ES_PT_NONFINITE.  A pair
 *       that is not ES_PT_OK gets NaN in every value and flux entry; its d_ext_x row is still written and the other pairs do
 *       not depend on it.  n_ext is 0 or >= 2; n == 0 succeeds and touches nothing.  Asynchronous on the context's stream
 *       (with d_status = NULL the first call at a larger n grows the context's scratch, which synchronises).  Argument errors
 *       as in section 6.
 *
 *     es_cyl_complex_polarisation: the interior and exterior formulas of es_cyl_polarisation (section 7) -- one program text
 *     -- evaluated with complex omega (d_w_re, d_w_im [n]), P and xi_r (the arrays of es_cyl_complex_eigenfunction).  The same
 *     es_field_profiles, ES_FIELD_REFERENCE and output order: n_r = N + n_ext, axis node -> boundary, then boundary -> far
 *     field, the boundary radius twice; radii must be positive.  d_radius [n x n_r] real; d_amp is complex,
 *     d_amp[((i * 7 + c) * n_r + j) * 2 + {re, im}], channels ES_AMP_*.  NaN eigenfunction rows give complex-NaN amplitudes;
 *     nodes where Om^2 - omega_A^2 or Om^2 - omega_c^2 vanish are not guarded, as in section 7.
 *       Phase convention: the convention between the channels is section 7's, which is the reference's -- the amplitudes are
 *       the analytic continuation of section 7 in omega, no factor of i is introduced between xi_r and xi_phi, xi_z.
 *
 *     es_cyl_complex_field_synthesis: the complex amplitude table of ONE mode (d_amp [7 x n_r x 2]) -> float32 frames
 *     d_out [n_t][n_sel][n_z][n_theta][n_r]; arguments as es_cyl_field_synthesis with w_re, w_im.  With
 *       EC = e^{w_im t} cos(k z - w_re t),    ES = e^{w_im t} sin(k z - w_re t)
 *     every variable of section 7 with angular factor Theta(theta) has the value A_re (Theta EC) - A_im (Theta ES) -- the real
 *     part of A Theta e^{i (k z - w t)} --, xi_x, xi_y, v_x, v_y are the section-7 rotations of those; fp64 throughout, rounded
 *     once.  At w_im = 0 and A_im = 0 this is section 7's expression, grouping included: the same bits.  d_points, var_mask,
 *     v_scale, ES_FIELD_Z_REFERENCE_ANGLE, ES_FIELD_BIG_ENDIAN, the size limits, the alignment rule (16-byte stores where the
 *     row is 16-byte aligned, 4-byte stores otherwise, the same bits either way), the empty-size and mask rules are those of
 *     section 7.
 *     (Eigenfunctions of the twisted cylinder at complex frequency: section 19; es_cyl_complex_polarisation and
 *     es_cyl_complex_field_synthesis take no problem and serve both families.)
 *     (Cartesian sampling and vorticity of these modes, section 8 at complex frequency: section 20.)
 *     Not offered: physically phased amplitudes (the i between the radial and the other components).
 * ====================================================================================================== */
int es_cyl_complex_eigenfunction(es_context* ctx, const es_problem* prob,
                                 const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                                 double* d_int_value, double* d_int_flux,      /* n x N complex      */
                                 int n_ext, double* d_ext_x,                   /* n x n_ext real     */
                                 double* d_ext_value, double* d_ext_flux,      /* n x n_ext complex  */
                                 uint8_t* d_status /* n, may be NULL */);

int es_cyl_complex_polarisation(es_context* ctx, const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                                int n_nodes, const double* d_int_value, const double* d_int_flux,   /* n x N complex     */
                                int n_ext, const double* d_ext_x,                                    /* n x n_ext real    */
                                const double* d_ext_value, const double* d_ext_flux,                 /* n x n_ext complex */
                                const es_field_profiles* profiles, int m, double rho_e, double vA_e, double c_e, double cT_e,
                                int flags, double* d_radius /* n x n_r */, double* d_amp /* n x 7 x n_r complex */);

int es_cyl_complex_field_synthesis(es_context* ctx, const double* d_radius, const double* d_amp /* 7 x n_r complex */,
                                   int n_r, int m, double k, double w_re, double w_im,
                                   const double* d_theta, int n_theta, const double* d_z, int n_z, const double* d_t, int n_t,
                                   uint32_t var_mask, double v_scale, int flags,
                                   float* d_points /* may be NULL */, float* d_out);

/* ======================================================================================================
 * (17) Complex frequencies on the twisted (rotating) cylinder: section 14 for ES_GEOM_CYLINDER_TWIST problems -- the
 *     determinant at omega = omega_r + i omega_i and its root search, the unstable (Kelvin-Helmholtz) modes of a tube with
 *     azimuthal shear.  ES_GEOM_CYLINDER_TWIST problems only (m >= 0 as in section 2, the three axis conditions, both values
 *     of c1_power, both signs of r); every other geometry gets ES_ERR_UNSUPPORTED with the outputs untouched (the untwisted
 *     cylinder has section 14, whose calls in turn keep refusing twisted problems).  Values only.
 *     What is computed: the interior of section 2 for this family -- the 20-field base table, the general coefficient set
 *     with v_phi and B_phi, one classical RK4 step of the full 2x2 system per interval, the adjoint row march, the axis
 *     condition by superposition (ES_AXIS_ROTATION_KINK: P(r_ax) + bc_const xi_e = 0) -- in complex arithmetic, and the
 *     exterior of section 14 as it is: the medium outside is the same.  Normalisation P_e(boundary) = 1, so at omega_i = 0
 *         D_c = sign(P_e(boundary)) D of es_shoot_eval_points,    Im D_c = 0,
 *     and D_c(k, conj omega) = conj D_c(k, omega).  outer, inner, rel, the statuses (ES_PT_LEAKY where Re(m_e) < 0,
 *     ES_PT_NONFINITE where m_e, xi_e_const or the result is not finite, never ES_PT_CONTINUUM; NaN outputs unless ES_PT_OK),
 *     the signatures, the grid layout, w_mode, the cell rule, the secant refinement, the flag, the order of the table, the
 *     capacity convention and the argument checks are those of section 14, word for word.  A call with no points succeeds
 *     and touches nothing.  The eval calls are asynchronous on the context's stream; es_cylt_complex_find_roots synchronises.
 *     Not offered: m < 0.  (Slopes and Newton tracing: section 18; eigenfunctions and fields: section 19.)
 * ====================================================================================================== */
int es_cylt_complex_eval_grid(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                              const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                              double* d_D_re, double* d_D_im, double* d_rel /* may be NULL */, uint8_t* d_status);

int es_cylt_complex_eval_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w_re,
                                const double* d_w_im, int n, double* d_D_re, double* d_D_im,
                                double* d_rel /* may be NULL */, uint8_t* d_status,
                                double* d_outer /* [n][2], may be NULL */, double* d_inner /* [n][2], may be NULL */);

int es_cylt_complex_find_roots(es_context* ctx, const es_problem* prob, const double* d_k, int nk,
                               const double* d_w_re, int n_re, const double* d_w_im, int n_im, int w_mode,
                               const double* d_D_re, const double* d_D_im, const uint8_t* d_status, int n_iter,
                               double tol_percent, es_complex_root_table* table, int* out_count);

/* ======================================================================================================
 * (18) Slopes and Newton tracing of complex roots of the twisted (rotating) cylinder (the unstable modes of section 17):
 *     section 15 for ES_GEOM_CYLINDER_TWIST problems.  ES_GEOM_CYLINDER_TWIST problems only (m >= 0, the three axis
 *     conditions, both values of c1_power, both signs of r); every other geometry gets ES_ERR_UNSUPPORTED with the outputs
 *     untouched (the untwisted cylinder has section 15, whose calls in turn keep refusing twisted problems).
 *     What is computed: the program text of section 17 -- the 20-field base table, the general coefficient set with v_phi and
 *     B_phi, the full-shape RK4 step, the adjoint row march, the axis condition, the Bessel exterior -- carried in jets of
 *     three complex components (value, d/d omega, d/dk) for the slopes and of two (value, d/d omega) for the Newton steps.
 *     Row 0 of d_outer / d_inner is the outer and inner of es_cylt_complex_eval_points.  On the real axis d omega / dk is
 *     real, the group speed of section 11, and the jets at conj omega are the conjugates of those at omega.
 *     The signatures, the output layouts ([3][n][2] outer / inner; w, resid, dwdk, iters, flag), d_count, the statuses, the
 *     NaN rule, the Newton rule (that of es_complex_newton, step for step), the flag, the argument checks and the
 *     asynchrony are those of section 15, word for word.
 *     Not offered: m < 0; second derivatives.  (Eigenfunctions and fields at these roots: section 19.)
 * ====================================================================================================== */
int es_cylt_complex_root_slopes(es_context* ctx, const es_problem* prob,
                                const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                                const int32_t* d_count /* may be NULL */,
                                double* d_outer /* [3][n][2]: value, d/dw, d/dk; (re, im) pairs */,
                                double* d_inner /* [3][n][2] */, uint8_t* d_status);

int es_cylt_complex_newton(es_context* ctx, const es_problem* prob,
                           const double* d_k, const double* d_guess_re, const double* d_guess_im, int n,
                           const int32_t* d_count /* may be NULL */,
                           int max_iter, double step_cap, double max_shift, double tol_percent,
                           double* d_w_re, double* d_w_im, double* d_resid,
                           double* d_dwdk /* [n][2], may be NULL */, int32_t* d_iters, int32_t* d_flag);

/* ======================================================================================================
 * (19) Eigenfunctions and perturbation fields of complex roots of the twisted (rotating) cylinder (the unstable modes of
 *     sections 17 and 18): section 16 for ES_GEOM_CYLINDER_TWIST problems.  ES_GEOM_CYLINDER_TWIST problems only (m >= 0,
 *     the three axis conditions, both values of c1_power, both signs of r); every other geometry gets ES_ERR_UNSUPPORTED
 *     with the outputs untouched (the untwisted cylinder has section 16, whose call in turn keeps refusing twisted
 *     problems).  DESIGN.md section 8n.
 *
 *     es_cylt_complex_eigenfunction: the signature, the layouts, the exterior, the normalisation P_e(boundary) = 1 + 0i,
 *     the NaN rule, the argument checks, the asynchrony and the d_status = NULL scratch rule of
 *     es_cyl_complex_eigenfunction, word for word; d_status[i] is the status section 17 gives the pair.
 *       Interior: the discrete problem of section 5 for this family in complex arithmetic -- the node / mid-point
 *       coefficient sets of section 17 (the 20-field base table, the general coefficient set with v_phi and B_phi, one
 *       complex division per node), one classical RK4 step of the full 2x2 system per interval taken outwards,
 *       y_j = S_j y_{j+1}, the axis condition at node N-1
 *           ES_AXIS_KINK            P =   bc_const xi_e
 *           ES_AXIS_ROTATION_KINK   P = -(bc_const xi_e)
 *           ES_AXIS_SAUSAGE         (P, Xi) along (a12, -a11)     (P' = 0; a11 is not zero in this family)
 *       and P = P_b at node 0; xi_r = Xi / r.  Its solution is the one section 16's two outward marches give in exact
 *       arithmetic, but it is not formed that way: with a non-zero target (every ES_AXIS_ROTATION_KINK problem) a state
 *       marched outwards grows like the regular solution r^m while the answer stays O(1), and P(r_b) = P_b came out of a
 *       cancellation that left up to 1e-6 of rounding in fp64.  Three passes instead: g from d = (0, 1) (sausage:
 *       (a12, -a11)) at the axis outwards, its raw state parked in the caller's own output rows; s from (0, 1) at the
 *       boundary inwards by the exact inverse of the same step, s_{j+1} = S_j^-1 s_j; s once more with every node written as
 *       a s_j + b g_j, b = P_b / P(g_0) and a = target / P(s_{N-1}) (sausage: a = 0).  So d_int_value and d_int_flux are
 *       read as well as written by the call, and the interior value at node 0 is P_b = 1 to one rounding.
 *       Exterior: the medium outside is the same; the exterior arrays are those of section 16.
 *       The exterior value at the boundary is exactly 1, the exterior flux at the boundary is the `outer` of
 *       es_cylt_complex_eval_points.  The identity
 *           exterior flux at the boundary - interior flux at node 0 = D_c
 *       holds to rounding for ES_AXIS_SAUSAGE and wherever the target is zero (bc_const = 0: the zero-twist limit), as in
 *       section 16.  With a non-zero target -- every ES_AXIS_ROTATION_KINK problem of the family -- the adjoint row march
 *       of the determinant and the outward step's solution differ by (det S - 1) target / p2, S the discrete outward transfer
 *       matrix, whose determinant RK4 keeps at 1 only to truncation: the identity then holds to the RK4 truncation of the
 *       grid, 1e-7 to 2e-4 of max(|outer|, |inner|) at N = 130 on the problems measured and smaller on a finer grid (the
 *       table of DESIGN.md section 8n).  The eigenfunction is the outward step's; on the real axis it is that of section 5
 *       wherever that march keeps its digits (3e-13 on the reference problem).
 *
 *     Amplitudes and frames: es_cyl_complex_polarisation and es_cyl_complex_field_synthesis (section 16) on these arrays;
 *     they take no problem.  With the twisted es_field_profiles (v_phi and s_phi not zero) the T, Q, g and s_phi terms of
 *     section 7's formulas take part with complex Om.
 *     (Cartesian sampling and vorticity of these modes: section 20, which takes no problem either.)
 *     Not offered: m < 0; physically phased amplitudes.
 * ====================================================================================================== */
int es_cylt_complex_eigenfunction(es_context* ctx, const es_problem* prob,
                                  const double* d_k, const double* d_w_re, const double* d_w_im, int n,
                                  double* d_int_value, double* d_int_flux,      /* n x N complex      */
                                  int n_ext, double* d_ext_x,                   /* n x n_ext real     */
                                  double* d_ext_value, double* d_ext_flux,      /* n x n_ext complex  */
                                  uint8_t* d_status /* n, may be NULL */);

/* ======================================================================================================
 * (20) Cartesian sampling of an unstable cylinder mode, with its vorticity: section 8 at complex frequency, on the complex
 *     amplitude tables of es_cyl_complex_polarisation (section 16).  Neither call takes a problem, so both serve the
 *     untwisted cylinder (sections 14 - 16) and the twisted one (sections 17 - 19).  DESIGN.md section 8o.
 *
 *     Convention: section 16's.  Every field is Re[A(r) Theta(theta) e^{i (k z - w t)}], w = w_re + i w_im, with the angular
 *     factors of sections 7 / 8; with
 *       EC = e^{w_im t} cos(k z - w_re t),    ES = e^{w_im t} sin(k z - w_re t)
 *     its value is A_re (Theta EC) - A_im (Theta ES).  With d/dz -> i k the curl of
 *       (v_r, v_phi, v_z) = Re[(a_r cos(m theta), a_phi (-sin(m theta)), a_z cos(m theta)) e^{i (k z - w t)}]
 *     has three complex radial amplitudes (the growth factor depends on t alone and does not enter):
 *       w_r   = Re[W_r   sin(m theta) e^{i (k z - w t)}]      W_r   = -m a_z / r + i k a_phi
 *       w_phi = Re[W_phi cos(m theta) e^{i (k z - w t)}]      W_phi = -a_z' + i k a_r
 *       w_z   = Re[W_z   sin(m theta) e^{i (k z - w t)}]      W_z   = (m a_r - a_phi - r a_phi') / r
 *     On a real table this is section 8: Re W = (Wr_C, Wphi_C, Wz_C), Im W = (-Wr_S, -Wphi_S, 0).
 *
 *     es_cyl_complex_vorticity_amplitudes: d_radius [n x n_r] real, d_amp [n x 7 x n_r] complex exactly as
 *     es_cyl_complex_polarisation writes them (interleaved (re, im) pairs), d_k [n]  ->
 *     d_vort[((i * 3 + c) * n_r + j) * 2 + {re, im}], channels c = ES_CVORT_*.  One lane per (mode, radial point).  The radial
 *     derivatives are those of es_cyl_vorticity_amplitudes -- np.gradient(a, r, edge_order=2) of each region on its own, in
 *     its coefficient form -- applied to the real and the imaginary part separately; each part keeps section 8's grouping, so
 *     that on a table with zero imaginary parts the values are section 8's.  A region that is present needs >= 3 points
 *     (argument error otherwise); n_nodes = 0 or n_ext = 0 leaves that region out.  NaN / inf amplitudes, in either part,
 *     reach the nodes whose stencil touches them and no others.  n == 0 is a successful call that touches nothing.
 *     Asynchronous on the context's stream.
 *
 *     es_cyl_complex_cartesian_synthesis: the complex tables of ONE mode, d_amp [7 x n_r x 2] and d_vort [3 x n_r x 2]
 *     (d_vort may be NULL if no vorticity bit is set)  ->  d_out [n_t][n_sel][n_z][n_y][n_x] float32.  Variables and mask:
 *     ES_CVAR_* of section 8.  Everything of es_cyl_cartesian_synthesis carries over: the regions and the tie rule, the
 *     bisection, the linear interpolation (of real and imaginary parts), `fill` as bits, ES_FIELD_BIG_ENDIAN as the only flag
 *     (ES_FIELD_Z_REFERENCE_ANGLE is an argument error), 16-byte stores where every plane starts on a 16-byte boundary and
 *     4-byte stores otherwise with the same bits, 4-byte alignment of d_out, the size limits, the empty sizes, the
 *     argument errors, the asynchrony.  Per point and variable a complex coefficient c is formed, part by part exactly as
 *     section 8 forms its real one (the (A * v_scale) * cos(m theta) grouping and the rotations to x, y included), and the
 *     value is c_re EC - c_im ES, fp64 throughout, rounded once.  At w_im = 0 and with zero imaginary parts this is section
 *     8's expression, grouping included: the same frames.  The launch shape is that of es_cyl_cartesian_split.
 *     Not offered: m < 0; physically phased amplitudes.
 * ====================================================================================================== */
enum { ES_CVORT_R = 0, ES_CVORT_PHI, ES_CVORT_Z, ES_CVORT_COUNT };

int es_cyl_complex_vorticity_amplitudes(es_context* ctx, const double* d_radius /* n x n_r */,
                                        const double* d_amp /* n x 7 x n_r complex */, int n, int n_nodes, int n_ext,
                                        int m, const double* d_k /* n */, double* d_vort /* n x 3 x n_r complex */);

int es_cyl_complex_cartesian_synthesis(es_context* ctx, const double* d_radius, const double* d_amp /* 7 x n_r complex */,
                                       const double* d_vort /* 3 x n_r complex, may be NULL if no vorticity bit is set */,
                                       int n_nodes, int n_ext, int m, double k, double w_re, double w_im,
                                       const double* d_x, int n_x, const double* d_y, int n_y, const double* d_z, int n_z,
                                       const double* d_t, int n_t, uint32_t var_mask, double v_scale, float fill,
                                       int flags, float* d_out);

/* ======================================================================================================
 * (21) Dispersion curvature: the second partial derivatives of the boundary determinant and the extrema of the group speed.
 *     With D, D_w, D_k of section 11 and D_ww, D_wk, D_kk, along the branch through a root
 *       the curvature              q = d2 omega / dk2 = d c_g / dk = -(D_kk + 2 D_wk c_g + D_ww c_g^2) / D_w,
 *                                  the group-velocity dispersion of a packet at k; it changes sign at an extremum of c_g
 *                                  (the Airy phase of an impulsively generated wave train),
 *       the Halley correction      d omega = -2 D D_w / (2 D_w^2 - D D_ww).
 *
 *     es_shoot_root_curvature: section 11's evaluation carried in six-component second-order jets -- exact to rounding, no
 *     step to choose.  Everything of es_shoot_root_slopes holds: one pair per lane, d_count, entries beyond the count left
 *     alone, any output pointer may be NULL, the asynchrony, n == 0, the argument errors.
 *       d_outer / d_inner [6][n]: rows 0-2 as section 11 (the same arithmetic), row 3 d2/d omega2, row 4 d2/d omega dk,
 *         row 5 d2/dk2 of the two sides.  The rows are n apart.
 *       d_status [n]: as section 11.  A pair whose exterior is not ES_PT_OK, or one of whose twelve outputs is not finite,
 *         gets NaN in all twelve.
 *
 *     es_shoot_cg_extrema: per lane a bracket on ONE branch, (k_lo, w_lo) and (k_hi, w_hi) with k_lo < k_hi, both roots or
 *     near-roots (e.g. neighbouring points of a Newton trace); the k at which the curvature changes sign between them.
 *       A point (k, w) is polished by Newton in omega at fixed k -- at most 8 steps, until |step| <= 1e-14 |omega|, failing
 *       on what fails a step of es_shoot_newton (no step cap) -- and evaluated once at second order: c_g, q, the status and
 *       the residual (percent) of es_shoot_eval_points there.
 *       Both ends are treated so.  If q_lo and q_hi do not differ in sign (a zero or a NaN differs from nothing) the end with
 *       the smaller |q| is reported (a finite one before a non-finite one), flag 0, iters 0.  Otherwise regula falsi with the
 *       Illinois modification on q(k): k_new = k_hi - f_hi (k_hi - k_lo) / (f_hi - f_lo) (the midpoint should rounding put it
 *       outside the open bracket), omega from the nearer end's Taylor prediction w + c_g dk + q dk^2 / 2, polished and
 *       evaluated as above; the new point replaces the end whose q has its sign, and where the same end is replaced twice
 *       running the ordinate f of the other end is halved.  Stops at q = 0, at k_hi - k_lo <= 1e-12 |k_new|, after
 *       max_iter iterates, or at an iterate whose polish failed or whose q is not finite.  The last iterate is reported.
 *       Every tolerance is relative: nothing ties the rule to a unit system.
 *       d_k, d_w, d_cg, d_q, d_resid, d_iters (iterates taken), d_flag [n]; d_status [n] (may be NULL).  flag = 1: the sign
 *       changed, every polish succeeded, the reported point is ES_PT_OK and resid < tol_percent.  A reported point without
 *       a value (leaky, non-finite) carries NaN in c_g, q and resid.
 *       ES_ERR_INVALID_ARG: a null problem, n < 0, max_iter < 0, tol_percent <= 0, a required pointer null with n > 0.
 *     Not offered: complex frequencies (sections 12, 15, 18), the closed-form uniform cylinder (section 4), third derivatives.
 * ====================================================================================================== */
int es_shoot_root_curvature(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, int n,
                            const int32_t* d_count /* may be NULL */,
                            double* d_outer /* [6][n]: value, d/dw, d/dk, d2/dw2, d2/dwdk, d2/dk2 */,
                            double* d_inner /* [6][n] */, uint8_t* d_status);

int es_shoot_cg_extrema(es_context* ctx, const es_problem* prob, const double* d_k_lo, const double* d_w_lo,
                        const double* d_k_hi, const double* d_w_hi, int n, const int32_t* d_count /* may be NULL */,
                        int max_iter, double tol_percent, double* d_k, double* d_w, double* d_cg, double* d_q,
                        double* d_resid, int32_t* d_iters, int32_t* d_flag, uint8_t* d_status /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* EIGENSOLVER_AMD_H */
