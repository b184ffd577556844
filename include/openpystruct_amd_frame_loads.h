/* openpystruct_amd -- C ABI, extension header: per-frame element loads around the batched frame solve.
 *
 * An addition to include/openpystruct_amd.h: three entry points of the same shared library, the same
 * conventions -- DEVICE pointers owned by the caller, nothing allocated, copied or synchronised inside, work enqueued on `stream`
 * (a hipStream_t passed as void*), return codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration of that header:
 * OPS_AMD_ABI_VERSION stays what it is.
 *
 * ops_frame_solve_batched_f64 takes one elem_w [Ne,2] (beamUniform Wy, Wx) for the whole batch.  The solve is linear in the element
 * loads: with pg_e = R_e^T [wx L/2, wy L/2, wy L^2/12, wx L/2, wy L/2, -wy L^2/12] (global, per element), the solve of frame b under
 * (loads_b, w_b) is three calls on one stream:
 *   1. ops_frame_load_rhs_f64:     rhs [B,Nn,3] = loads + sum over each node's element ends of pg_e[3 end .. 3 end + 2], pg_e from the
 *                                  frame's own (wy, wx);
 *   2. ops_frame_solve_batched_f64_ex with loads = rhs (loads_bstride = n_nodes * 3) and an all-zero elem_w.  The assembly plan holds
 *      the consistent loads of elem_w, so a plan built with another elem_w must NOT be reused here: flags = 0, or a workspace of
 *      this path's own;
 *   3. ops_frame_load_forces_f64:  forces[b,e,:] -= pg_e in place, then V = forces[...,1], M = forces[...,2].  Rows of a frame with
 *                                  status[b] != 0 are not touched (they hold the solve's NaNs); status NULL: every frame is corrected.
 * ops_frame_load_vjp_f64 is the gradient with respect to the element loads:
 *   g_w[b,e,0] = (lambda_e - g_f,e) . dpg_e/dwy,  g_w[b,e,1] = (lambda_e - g_f,e) . dpg_e/dwx,
 * lambda the adjoint displacements of include/openpystruct_amd_frame_vjp.h (its step 2; zero on constrained DOFs), g_f = g_forces
 * with gV added to component 1 and gM to component 2 (each NULL = zeros).  A frame with a non-zero status_fwd or status_adj (either may
 * be NULL) gets a NaN row.  dL/dI and dL/dloads of that header do not depend on the element loads.
 *   elem_geo [Ne,3] (L, cos, sin); conn [Ne,2]; node_elem_ptr [Nn+1] / node_elem_idx [2 Ne]: per node, its incident element ends as
 *   2 * element + end (CSR; any degree): the order of each node's sum;
 *   loads [Nn,3] (loads_bstride 0) or [B,Nn,3] (loads_bstride 3 Nn); elem_w [Ne,2] (w_bstride 0) or [B,Ne,2] (w_bstride 2 Ne).
 * No atomics: the results are reproducible and depend neither on B nor on a frame's place in the batch.  B == 0: OK, nothing is
 * launched; a negative size, n_nodes < 2, n_elems < 1, a stride other than the two allowed values or a NULL required pointer:
 * ERR_INVALID_ARG, nothing is written.  One launch each.  Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_FRAME_LOADS_H
#define OPENPYSTRUCT_AMD_FRAME_LOADS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int ops_frame_load_rhs_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const int32_t* node_elem_ptr,
                           const int32_t* node_elem_idx, const double* loads, long loads_bstride, const double* elem_w,
                           long w_bstride, double* rhs, void* stream);
int ops_frame_load_forces_f64(int B, int n_elems, const double* elem_geo, const double* elem_w, long w_bstride,
                              const int32_t* status, double* forces, double* V, double* M, void* stream);
int ops_frame_load_vjp_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const int32_t* conn,
                           const double* lambda, const double* g_forces, const double* gV, const double* gM,
                           const int32_t* status_fwd, const int32_t* status_adj, double* g_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_FRAME_LOADS_H */
