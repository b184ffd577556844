/* openpystruct_amd -- C ABI, extension header: the exact ("total") gradient of the frame sizing objective.
 *
 * An addition to include/openpystruct_amd.h (the reference's frame loop differentiates the explicit I terms of its loss only and
 * holds M and V fixed): two entry points of the same shared library, the same conventions -- DEVICE pointers owned by
 * the caller, nothing allocated, copied or synchronised inside, work enqueued on `stream` (a hipStream_t passed as void*), return
 * codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration of that header: OPS_AMD_ABI_VERSION and ops_sizing_params
 * stay what they are.
 *
 * The objective, in float64, per frame:
 *   L(I) = sum_e I_e + alpha_moment sum_e M_e^2 / (2 E I_e + bend_eps) + alpha_shear sum_e V_e^2 / (G area_coef sqrt(I_e))
 *        + alpha_sway sum_n h(|ux_n|, sway_limit) + alpha_deflection sum_n h(|uy_n|, deflection_limit),
 *   h(a, lim) = (max(0, a - lim) / lim)^2,
 * with E, G, alpha_moment, alpha_shear, bend_eps, area_coef of ops_sizing_params, M = forces[..., 2], V = forces[..., 1] (global Fy,
 * for columns too) and ux, uy = disp[..., 0], disp[..., 1] over all nodes (constrained DOFs are 0), all functions of I through the
 * solve.  The limits are penalties: nothing here holds a displacement below its limit.
 *
 * dL/dI is three calls on one stream, the solve's VJP of openpystruct_amd_frame_vjp.h with the objective's cotangents
 * (gM = dL/dM, gV = dL/dV, g_disp[n] = (dL/dux_n, dL/duy_n, 0)) formed in registers from this epoch's forward instead of read:
 *   1. ops_frame_sizing_rhs_f64:   rhs [B,Nn,3], the adjoint right-hand side, and loss_extra [B], the value of the two hinge terms
 *                                  per frame, summed in one fixed order (no atomics): its bits depend on the frame's own data and
 *                                  on n_nodes, not on B, on the frame's place in the batch or on the launch;
 *   2. ops_frame_solve_batched_f64_ex with loads = rhs (loads_bstride = n_nodes * 3), an all-zero elem_w and a workspace of the
 *      adjoint's own (see openpystruct_amd_frame_vjp.h): its disp is lambda;
 *   3. ops_frame_sizing_grad_f64:  grad [B,Ne] = explicit part (M, V held fixed) + (g_f,e - lambda_e) . (K_b,e u_e).
 *   elem_geo, elem_EA, elem_E, conn, node_elem_ptr, node_elem_idx: as in openpystruct_amd_frame_vjp.h;
 *   I [B,Ne]; disp [B,Nn,3], V, M [B,Ne]: the forward's outputs on that I; lambda [B,Nn,3]: the adjoint solve's disp.
 *   active [B] (may be NULL: all): a frame with active[b] == 0 gets ZEROS in its rhs rows (the adjoint solve then gives lambda = 0
 *   and reads nothing uninitialised); its loss_extra and its grad row are not written; a wavefront of such frames loads nothing else.
 *   loss_extra may be NULL when alpha_sway == alpha_deflection == 0 (it is written, as 0, when given).  A frame whose forward failed
 *   has NaN in disp: the hinge's comparisons would drop a NaN, so the rhs entry forwards it -- loss_extra is NaN whenever ux or uy
 *   of a node is.  status_fwd / status_adj [B] (either may be NULL): a frame with a non-zero status gets NaN in its grad row.
 * B == 0: OK.  A negative size, n_nodes < 2, n_elems < 1, a NULL required pointer, an alpha that is not >= 0, an alpha > 0 with a
 * limit that is not > 0, alpha_sway + alpha_deflection > 0 with loss_extra == NULL: ERR_INVALID_ARG, nothing written.  One launch
 * each.  Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_FRAME_SIZING_H
#define OPENPYSTRUCT_AMD_FRAME_SIZING_H

#include <stdint.h>

#include "openpystruct_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ops_frame_sizing_objective { double alpha_sway, sway_limit, alpha_deflection, deflection_limit; } ops_frame_sizing_objective;

int ops_frame_sizing_rhs_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA,
                             const double* elem_E, const int32_t* node_elem_ptr, const int32_t* node_elem_idx,
                             const double* I, const double* disp, const double* V, const double* M,
                             const ops_sizing_params* hp, const ops_frame_sizing_objective* obj, const uint8_t* active,
                             double* rhs, double* loss_extra, void* stream);
int ops_frame_sizing_grad_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                              const int32_t* conn, const double* I, const double* disp, const double* V, const double* M,
                              const double* lambda, const ops_sizing_params* hp, const uint8_t* active,
                              const int32_t* status_fwd, const int32_t* status_adj, double* grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_FRAME_SIZING_H */
