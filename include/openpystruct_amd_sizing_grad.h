/* openpystruct_amd -- C ABI, extension header: the exact ("total") gradient of the beam sizing objective.
 *
 * An addition to include/openpystruct_amd.h (the reference's sizing loop differentiates the explicit I terms of its loss only and
 * holds M and V fixed): two entry points of the same shared library, the same conventions -- DEVICE pointers owned by
 * the caller, nothing allocated, copied or synchronised inside, work enqueued on `stream` (a hipStream_t passed as void*), return
 * codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration of that header: OPS_AMD_ABI_VERSION and ops_sizing_params
 * stay what they are.
 *
 * The objective, in float64:
 *   L(I) = sum_e I_e + alpha_moment sum_e M_e^2 / (2 E I_e + bend_eps) + alpha_shear sum_e V_e^2 / (G area_coef sqrt(I_e))
 *        + alpha_deflection sum_n (max(0, |v_n| - deflection_limit) / deflection_limit)^2
 * with E, G, alpha_moment, alpha_shear, bend_eps, area_coef of ops_sizing_params and M, V, v functions of I through the solve.
 *
 * The gradient entry point (sizing_grad): grad [B,Ne] = dL/dI, the explicit part plus the adjoint solve, ONE launch; the cotangents
 * are formed in registers from this epoch's forward (v, theta, V, M: the outputs of ops_beam_solve_batched_f64 on the same x, E, I,
 * fix, wy).  x, E, I, fix, wy and their batch strides as in ops_beam_solve_vjp_f64 (stride 0 = one row shared by all beams; I is
 * always per beam).  active (may be NULL: all): rows of cases with active[b] == 0 are not written, a wave of such cases returns at once.
 * loss_extra [B]: the value of the deflection term, summed in a fixed order (no atomics); may be NULL when alpha_deflection == 0.
 * status [B] (may be NULL): 0, or non-zero for a beam whose factorisation met a non-positive pivot -- its grad row and loss_extra
 * are NaN, the other beams are computed as if solved alone.  alpha_deflection > 0 needs deflection_limit > 0 and loss_extra.
 * Ne up to ops_amd_max_elements() (ERR_UNSUPPORTED beyond).
 *
 * The step entry point (sizing_step_grad) is ops_beam_sizing_step_f32 with the Adam gradient read from grad (rounded to float32)
 * instead of the explicit formula, and (float)loss_extra[b] (NULL: nothing) added to the case's loss before the early-stop decision;
 * everything else -- the loss on the float32-rounded V, M, Adam, the schedule table (may be NULL), the clamp, I64 frozen when a case
 * stops, inactive cases untouched, Ne <= 512 -- is that entry point's.  V32, M32: both or neither.
 * B == 0: OK; a negative size, a NULL required pointer or a bad stride: ERR_INVALID_ARG, nothing written.  Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_SIZING_GRAD_H
#define OPENPYSTRUCT_AMD_SIZING_GRAD_H

#include <stdint.h>

#include "openpystruct_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ops_sizing_objective {
  double alpha_deflection;   /* weight of the deflection term; 0: the term is absent */
  double deflection_limit;   /* v_lim > 0, in the units of v; read only when alpha_deflection > 0 */
} ops_sizing_objective;

int ops_beam_sizing_grad_f64(int B, int Ne, const double* x, long x_bstride, const double* E, long E_bstride,
                             const double* I, long I_bstride, const uint8_t* fix, long fix_bstride,
                             const double* wy, long wy_bstride, const double* v, const double* theta,
                             const double* V, const double* M, const ops_sizing_params* hp,
                             const ops_sizing_objective* obj, const uint8_t* active, double* grad,
                             double* loss_extra, int32_t* status, void* stream);
int ops_beam_sizing_step_grad_f32(int B, int Ne, float* I, double* I64, const double* V, const double* M,
                                  const double* grad, const double* loss_extra, float* exp_avg, float* exp_avg_sq,
                                  float* best_loss, int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active,
                                  float* last_loss, float* V32, float* M32, const ops_sizing_params* hp,
                                  const float* schedule, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_SIZING_GRAD_H */
