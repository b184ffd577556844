/* openpystruct_amd -- C ABI, extension header: a natural-frequency floor in frame design sizing.
 *
 * An addition to include/openpystruct_amd.h, include/openpystruct_amd_frame_loads.h (9p), include/openpystruct_amd_frame_designs.h
 * (9l) and include/openpystruct_amd_frame_groups.h (9n): three entry points of the same shared library, the same conventions --
 * DEVICE pointers owned by the caller, nothing allocated, copied or synchronised inside, work enqueued on `stream` (a hipStream_t
 * passed as void*), return codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration of those headers:
 * OPS_AMD_ABI_VERSION and ops_sizing_params stay what they are.
 *
 *   ops_frame_frequency_floor_f64: the hinge of the m lowest eigenvalues of K(I) phi = lambda M phi against a floor, and its
 *   gradient.  floor = (2 pi f_min)^2, one value (floor_stride 0) or one per design (1).
 *       h_j            = max(0, 1 - lambda[g,j] / floor)                          j < m
 *       penalty[g]     = alpha * sum_j h_j^2
 *       grad_extra[g,e] = sum_j, in mode order, of (-2 alpha h_j / floor) phi_j,e . (K_b,e phi_j,e)
 *   phi [G,p,Nn,3]: M-normalised vectors, the Q the Ritz step of ops_frame_modes_ritz_f64 leaves; lambda [G,p]; M does not depend on
 *   I, so no adjoint solve.  One thread per (design, element) as ops_frame_modes_grad_f64; the m coefficients are formed in
 *   registers from lambda (no cotangent array in memory); penalty[g] is written by the thread of element 0.  A design with
 *   status[g] != 0 gets a NaN row and a NaN penalty; a design with active[g] == 0 (active may be NULL: all active) writes nothing.
 *   Where every h_j is 0 the row is exactly +0.0 and the penalty exactly 0.0.  No atomics, no LDS.
 *   Refused as ops_frame_modes_grad_f64 refuses (G < 0, p outside 1 .. 8, m outside 1 .. p, n_nodes < 2, n_elems < 1, a NULL array:
 *   ERR_INVALID_ARG; G == 0: OK, nothing launched); also alpha not >= 0, a floor_stride that is neither 0 nor 1 and floor NULL:
 *   ERR_INVALID_ARG.
 *
 *   ops_frame_design_step_dyn_f32, ops_frame_group_step_dyn_f32: ops_frame_design_step_f32 and ops_frame_group_step_f32 with two more
 *   arrays, both required (NULL: ERR_INVALID_ARG), neither specific to frequency: grad_extra [G,n_elems] float64, a gradient with
 *   respect to the element inertias, and penalty_extra [G] float64.  After the walk over the cases
 *       g64[e] += grad_extra[g,e]          one float64 addition, before grad_out is written, before the value is rounded to float32
 *                                          and, in the group step, before the per-group sum;
 *       loss    = loss + (float)penalty_extra[g]      added last, in float32 (under "max": after the max, it is not one of the cases).
 *   Adam, the clamp, the early stop and the stores are those of the plain entries; with zeros in both arrays every field is bit-equal
 *   to theirs.  Everything those entries refuse is refused alike.  All decided before any HIP call.  Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_FRAME_FREQUENCY_H
#define OPENPYSTRUCT_AMD_FRAME_FREQUENCY_H

#include <stdint.h>

#include "openpystruct_amd.h"
#include "openpystruct_amd_frame_designs.h"
#include "openpystruct_amd_frame_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

int ops_frame_frequency_floor_f64(int G, int m, int p, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                                  const int32_t* conn, const double* phi, const double* lambda, const int32_t* status,
                                  const double* floor, long floor_stride, double alpha, const uint8_t* active, double* grad_extra,
                                  double* penalty, void* stream);

int ops_frame_design_step_dyn_f32(int G, int C, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                                  const int32_t* conn, float* I, double* I64, const double* disp, const double* V, const double* M,
                                  const double* lambda, const double* loss_extra, const int32_t* status_fwd,
                                  const int32_t* status_adj, const double* weights, int aggregate, float* exp_avg, float* exp_avg_sq,
                                  float* best_loss, int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active, float* last_loss,
                                  float* case_penalty, int32_t* governing, double* grad_out, const ops_sizing_params* hp,
                                  const float* schedule, const double* grad_extra, const double* penalty_extra, void* stream);

int ops_frame_group_step_dyn_f32(int G, int C, int n_nodes, int n_elems, int n_groups, const double* elem_geo, const double* elem_E,
                                 const int32_t* conn, const int32_t* elem_group, const int32_t* group_ptr, const int32_t* group_elems,
                                 float* X, float* I, double* I64, const double* disp, const double* V, const double* M,
                                 const double* lambda, const double* loss_extra, const int32_t* status_fwd, const int32_t* status_adj,
                                 const double* weights, int aggregate, float* exp_avg, float* exp_avg_sq, float* best_loss,
                                 int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active, float* last_loss, float* case_penalty,
                                 int32_t* governing, double* grad_out, const ops_sizing_params* hp, const float* schedule,
                                 const double* grad_extra, const double* penalty_extra, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_FRAME_FREQUENCY_H */
