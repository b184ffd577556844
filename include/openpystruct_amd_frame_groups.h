/* openpystruct_amd -- C ABI, extension header: frame sizing of one design under C load cases with LINKED design variables -- several
 * elements share one section.
 *
 * An addition to include/openpystruct_amd.h and include/openpystruct_amd_frame_designs.h (9l): one entry point of the same shared
 * library, the same conventions -- DEVICE pointers owned by the caller, nothing allocated, copied or synchronised inside, work
 * enqueued on `stream` (a hipStream_t passed as void*), return codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration
 * of those headers: OPS_AMD_ABI_VERSION and ops_sizing_params stay what they are.
 *
 *   ops_frame_group_step_f32: ops_frame_design_step_f32 (same layout of the G designs and their G*C rows, same arguments with the
 *   same meaning) with the design variables by group.  An epoch of the loop (openpystruct_amd/frame_groups.py) is that of 9l with
 *   this launch in the place of the design step.
 *
 *   Tables, shared by all designs, int32, on the device: elem_group [n_elems], the group of every element, in 0 .. n_groups-1;
 *   group_ptr [n_groups+1] and group_elems [n_elems], the same map in CSR form: group j holds the elements
 *   group_elems[group_ptr[j] .. group_ptr[j+1]), in ascending order, and every group is non-empty.  THE TABLES ARE DEVICE MEMORY: THIS
 *   ENTRY CANNOT VALIDATE THEM.  openpystruct_amd.frame_groups.member_groups builds them from checked labels and is the only
 *   supported source of them; a table that breaks the rules above gives undefined results.
 *
 *   State: X [G,n_groups] float32, the variables; exp_avg, exp_avg_sq [G,n_groups].  I [G,n_elems] float32 and I64 [G,n_elems]
 *   float64 are outputs, the expansion I[e] = X[elem_group[e]] of the new variables; I64 is also an input, exactly as in the design
 *   step (the gradient is formed on what the last factorisation ran on), and is not refreshed when the design stops.  The float32
 *   inertia of element e that the penalties are formed on is X[g, elem_group[e]].
 *
 *   Per design: penalties, loss, governing case and the per-element float64 gradient g[e], aggregated over the cases, are the
 *   expressions of ops_frame_design_step_f32 in its order (csrc/frame_designs_math.hpp, one function for both entries).  Then
 *   gX[j] = g[e_0] + g[e_1] + ... over the elements of group j in group_elems order, in float64, starting from the first element's
 *   value.  (The objective's sum_e I_e stays a sum over elements: its derivative, the size of the group, is part of that sum.)
 *   grad_out [G,n_groups] (may be NULL) = gX before rounding.  Adam, the clamp and the early stop are the design step's, applied
 *   to X with (float)gX[j].  A design with active[g] == 0 writes nothing.  One 64-lane wavefront per design, no atomics, a fixed
 *   summation order: a design's result depends on its own data alone, not on G or on its position.  With the identity table
 *   (n_groups == n_elems, elem_group[e] == e) every field is bit-equal to ops_frame_design_step_f32, and X to I.
 *
 * n_groups < 1, n_groups > n_elems or a NULL table (or X): ERR_INVALID_ARG.  Everything else ops_frame_design_step_f32 refuses is
 * refused alike (G == 0: OK, nothing launched).  All decided before any HIP call, nothing written.  Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_FRAME_GROUPS_H
#define OPENPYSTRUCT_AMD_FRAME_GROUPS_H

#include <stdint.h>

#include "openpystruct_amd.h"
#include "openpystruct_amd_frame_designs.h"

#ifdef __cplusplus
extern "C" {
#endif

int ops_frame_group_step_f32(int G, int C, int n_nodes, int n_elems, int n_groups, const double* elem_geo, const double* elem_E,
                             const int32_t* conn, const int32_t* elem_group, const int32_t* group_ptr, const int32_t* group_elems,
                             float* X, float* I, double* I64, const double* disp, const double* V, const double* M,
                             const double* lambda, const double* loss_extra, const int32_t* status_fwd, const int32_t* status_adj,
                             const double* weights, int aggregate, float* exp_avg, float* exp_avg_sq, float* best_loss,
                             int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active, float* last_loss, float* case_penalty,
                             int32_t* governing, double* grad_out, const ops_sizing_params* hp, const float* schedule, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_FRAME_GROUPS_H */
