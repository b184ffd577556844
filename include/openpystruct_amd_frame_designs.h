/* openpystruct_amd -- C ABI, extension header: frame sizing of ONE design under C load cases on one kept factorisation.
 *
 * An addition to include/openpystruct_amd.h, include/openpystruct_amd_frame_sizing.h (9h), include/openpystruct_amd_sizing_multicase.h
 * (9j) and include/openpystruct_amd_frame_cases.h (9k): three entry points of the same shared library, the same conventions --
 * DEVICE pointers owned by the caller, nothing allocated, copied or synchronised inside, work enqueued on `stream` (a hipStream_t
 * passed as void*), return codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration of those headers:
 * OPS_AMD_ABI_VERSION, ops_sizing_params and ops_frame_sizing_objective stay what they are.
 *
 * Layout: G designs of n_elems elements, each under C load cases, design-major: case c of design g is row g*C + c of
 * disp [G,C,Nn,3], V, M [G,C,Ne], rhs, lambda [G,C,Nn,3], loss_extra, status_fwd, status_adj [G,C] -- the outputs of
 * ops_frame_resolve_f64 on the design's kept factor.  The inertias exist ONCE per design: I [G,Ne] float32 and I64 [G,Ne] float64
 * (what ops_frame_factor_solve_f64 factorises); no entry here reads or writes C copies of them.
 *
 * An epoch of the loop (openpystruct_amd/frame_designs.py) is ops_frame_factor_solve_f64 on I64, ops_frame_resolve_f64 (forward),
 * 1. below, ops_frame_resolve_f64 (adjoint: its disp is lambda), 2. below.
 *
 *   1. ops_frame_design_rhs_f64: the adjoint right-hand sides rhs and the hinge values loss_extra of all G*C rows.  It is
 *      ops_frame_sizing_rhs_f64 (same objective, same lane-group mapping, same summation order) with the inertia of row r read from
 *      I64[r / C] and `active` [G] (may be NULL: all) read per design: every row of rhs and loss_extra is bit-equal to
 *      ops_frame_sizing_rhs_f64 on the G*C rows with I repeated per case (and active repeated per row).  A design with
 *      active[g] == 0 gets zeros in its C rhs rows; its loss_extra entries are not written.
 *   2. ops_frame_design_step_f32: ONE launch, per design
 *        the gradient per case, in float64: grad_c[e] = explicit part + (g_f,e - lambda_c,e) . (K_b,e u_c,e), the expression of
 *        ops_frame_sizing_grad_f64 (NaN where status_fwd[g,c] or status_adj[g,c] is non-zero; either may be NULL); the per-case
 *        gradient rows never exist in memory;
 *        the design step of ops_beam_sizing_step_multicase_f32 (9j): float32 penalties P_c on the float32-rounded V, M plus
 *        (float)loss_extra[g,c]; aggregate 0: L = sum I + sum_c w_c P_c, Adam gradient (float)(sum_c w_c grad_c - (sum_c w_c - 1));
 *        aggregate 1: L = sum I + max_c P_c, ties to the lowest index, the gradient of the governing case only (formed once c* is
 *        known); Adam, the schedule table ([max_epochs, 2] of ops_sizing_schedule_f32, may be NULL: pow() in the kernel), the clamp,
 *        one early stop per design.  The new inertias go to I [G,Ne] and, widened, to I64 [G,Ne]; I64 is not refreshed when the
 *        design stops (it keeps what the last solve ran on).
 *      The state I, exp_avg, exp_avg_sq, best_loss, patience_cnt, epochs_run, active, last_loss, case_penalty, governing is
 *      bit-equal to ops_frame_sizing_grad_f64 on the G*C rows (I repeated) followed by ops_beam_sizing_step_multicase_f32, and
 *      I64[g] to that chain's I64_rows[g*C].  Optional (may be NULL): loss_extra, status_fwd, status_adj, weights [C] float64
 *      (NULL: all 1), schedule, case_penalty [G,C] float32, governing [G] int32, grad_out [G,Ne] float64 = the aggregated gradient
 *      before it is rounded to float32.  A design with active[g] == 0 writes nothing.  One 64-lane wavefront per design, no atomics,
 *      no LDS, a fixed summation order: a design's result depends on its own data alone, not on G or on its position.
 *   3. ops_frame_design_max_cases: the largest C served (64).
 *
 * G == 0: OK, nothing launched.  A negative size, C < 1, n_nodes < 2, n_elems < 1, a NULL required pointer, an alpha that is not
 * >= 0 or an alpha > 0 with a limit that is not > 0 (rhs), alpha_sway + alpha_deflection > 0 with loss_extra == NULL (rhs),
 * aggregate outside {0, 1}, weights with aggregate == 1: ERR_INVALID_ARG.  n_elems > 512 (the step's limit, in both entries),
 * C > ops_frame_design_max_cases() or G*C beyond 2^31 - 1: ERR_UNSUPPORTED.  All decided before any HIP call, nothing written.  Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_FRAME_DESIGNS_H
#define OPENPYSTRUCT_AMD_FRAME_DESIGNS_H

#include <stdint.h>

#include "openpystruct_amd.h"
#include "openpystruct_amd_frame_sizing.h"

#ifdef __cplusplus
extern "C" {
#endif

int ops_frame_design_rhs_f64(int G, int C, int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA,
                             const double* elem_E, const int32_t* node_elem_ptr, const int32_t* node_elem_idx,
                             const double* I64, const double* disp, const double* V, const double* M,
                             const ops_sizing_params* hp, const ops_frame_sizing_objective* obj, const uint8_t* active,
                             double* rhs, double* loss_extra, void* stream);
int ops_frame_design_step_f32(int G, int C, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                              const int32_t* conn, float* I, double* I64, const double* disp, const double* V, const double* M,
                              const double* lambda, const double* loss_extra, const int32_t* status_fwd,
                              const int32_t* status_adj, const double* weights, int aggregate, float* exp_avg,
                              float* exp_avg_sq, float* best_loss, int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active,
                              float* last_loss, float* case_penalty, int32_t* governing, double* grad_out,
                              const ops_sizing_params* hp, const float* schedule, void* stream);
int ops_frame_design_max_cases(void);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_FRAME_DESIGNS_H */
