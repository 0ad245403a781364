// Host functions of the shooting path that cross its translation units (es_shoot.hip, es_refine.hip, es_screen.hip,
// es_roots.hip, es_problem.hip); plain functions, as es_ensure_scratch in es_common.hpp.
#pragma once
#include "es_shoot_shared.hpp"

constexpr uint8_t F32_UNSURE = 0x80;   // status bit: the fp32 screening (es_screen.hip) cannot vouch for sign or status

// a launch bound as the kernels take it: counts are int32, a launch may be sized for more (a grid beyond 2^31 cells)
inline int es_bound(long n_max) { return (int)(n_max < INT32_MAX ? n_max : INT32_MAX); }
inline dim3 es_blocks(long n_max) { return dim3((unsigned)((n_max + 255) / 256)); }

int check_problem(es_context* ctx, const es_problem* prob);                                    // es_problem.hip
int check_root_table(es_context* ctx, const es_root_table* table);
int check_mixed_args(es_context* ctx, const es_problem* prob, int nk, int nw, int w_mode);     // es_screen.hip
// the hybrid rule is defined on 17-section only; checked by every search before it enqueues anything (es_refine.hip)
int check_refine_rule(es_context* ctx);

// fp64 evaluation of es_count(d_n, n_max) points, the launch sized for n_max (d_rel is optional); es_shoot.hip
int dispatch_points(es_context* ctx, const es_problem* prob, const double* d_k, const double* d_w, const int* d_n, long n_max,
                    double* d_D, double* d_rel, uint8_t* d_status);
// refinement by the context's rule (es_refine.hip); d_n, n_max, n_hint: see launch_refine_steps
int dispatch_refine(es_context* ctx, const es_problem* prob, const es_root_table& tab, const int* d_n, int n_max, int n_hint,
                    int n_bisect, double tol);
