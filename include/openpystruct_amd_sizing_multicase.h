/* openpystruct_amd -- C ABI, extension header: the optimiser step of ONE design under C load cases.
 *
 * An addition to include/openpystruct_amd.h and include/openpystruct_amd_sizing_grad.h: two entry points of the same shared
 * library, the same conventions -- DEVICE pointers owned by the caller, nothing allocated, copied or synchronised inside, work
 * enqueued on `stream` (a hipStream_t passed as void*), return codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration
 * of those headers: OPS_AMD_ABI_VERSION and ops_sizing_params stay what they are.
 *
 * Layout: G designs of Ne elements, each carried by C beam rows (its load cases), design-major: load case c of design g is beam
 * row g*C + c of V, M, grad [G*C, Ne] and loss_extra [G*C] -- the outputs of ops_beam_solve_batched_f64 and
 * ops_beam_sizing_grad_f64 on the G*C rows, whose inertias are I64_rows.
 *
 * Per design, in float32 on the float32-rounded V and M (as ops_beam_sizing_step_grad_f32 forms its loss):
 *   P_c = alpha_moment sum_e M_c,e^2 / (2 E I_e + bend_eps) + alpha_shear sum_e V_c,e^2 / (G (area_coef sqrt(I_e)))
 *         + (float)loss_extra[g*C + c]                                   (loss_extra == NULL: the last term is absent)
 *   aggregate == 0 (weighted sum):  L = sum_e I_e + sum_c w_c P_c,  w = weights [C] float64 on the device (NULL: all 1);
 *                                   Adam gradient (float)(sum_c w_c grad_c[e] - (sum_c w_c - 1)), formed in float64: every row
 *                                   of grad is 1 + dP_c/dI, the weight term 1 is counted once.
 *   aggregate == 1 (worst case):    L = sum_e I_e + max_c P_c, governing case c* = the lowest index that attains the maximum;
 *                                   Adam gradient (float)grad_c*[e].  weights must be NULL.
 * With C == 1, aggregate == 0 and weights == NULL the step is ops_beam_sizing_step_grad_f32 bit for bit (the loss is summed
 * ((sum I + a_M b_0) + a_S s_0) + extra_0, later cases are added as P_c in index order; with weights every case enters as
 * (float)w_c * P_c).  Then Adam, the schedule table ([max_epochs, 2] of ops_sizing_schedule_f32, may be NULL: pow() in the
 * kernel), the clamp and the early stop of that entry point, once per design.
 *
 * Written per design [G, ...]: I, exp_avg, exp_avg_sq [G, Ne] float32, best_loss, last_loss [G] float32, patience_cnt,
 * epochs_run [G] int32, active [G] uint8.  I64_rows [G*C, Ne]: the new inertias widened, the same row C times -- what the next
 * solve and gradient launches read; not refreshed when the design stops.  active_rows [G*C]: cleared for the C rows of a design
 * that stops (the `active` argument of ops_beam_sizing_grad_f64).  Optional (may be NULL): case_penalty [G*C] float32 = P_c,
 * governing [G] int32 = c* (aggregate 1) or the lowest index of the largest w_c P_c (aggregate 0).
 * A design with active[g] == 0 writes nothing.  No atomics, a fixed summation order: a design's result does not depend on G or on
 * its neighbours in the launch.
 *
 * G == 0: OK.  A negative size, C < 1, Ne < 1, a NULL required pointer (everything but loss_extra, weights, schedule,
 * case_penalty, governing), aggregate outside {0, 1}, weights with aggregate == 1: ERR_INVALID_ARG.  Ne > 512 or
 * C > ops_beam_sizing_multicase_max_cases(): ERR_UNSUPPORTED.  All decided before any HIP call, nothing written.
 * Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_SIZING_MULTICASE_H
#define OPENPYSTRUCT_AMD_SIZING_MULTICASE_H

#include <stdint.h>

#include "openpystruct_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int ops_beam_sizing_step_multicase_f32(int G, int C, int Ne, float* I, double* I64_rows, const double* V, const double* M,
                                       const double* grad, const double* loss_extra, const double* weights, int aggregate,
                                       float* exp_avg, float* exp_avg_sq, float* best_loss, int32_t* patience_cnt,
                                       int32_t* epochs_run, uint8_t* active, uint8_t* active_rows, float* last_loss,
                                       float* case_penalty, int32_t* governing, const ops_sizing_params* hp,
                                       const float* schedule, void* stream);
int ops_beam_sizing_multicase_max_cases(void);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_SIZING_MULTICASE_H */
