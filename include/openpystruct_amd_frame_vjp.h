/* openpystruct_amd -- C ABI, extension header: the vector-Jacobian product of the batched frame solve.
 *
 * An addition to include/openpystruct_amd.h (the reference differentiates nothing through its solve): two entry
 * points of the same shared library, the same conventions -- DEVICE pointers owned by the caller, nothing allocated, copied or
 * synchronised inside, work enqueued on `stream` (a hipStream_t passed as void*), return codes OPS_AMD_OK / OPS_AMD_ERR_* -- and
 * no change to any declaration of that header: OPS_AMD_ABI_VERSION stays what it is.
 *
 * The stiffness matrix is symmetric, so the adjoint system is the forward system with another right-hand side, and the VJP of
 * ops_frame_solve_batched_f64 is three calls on one stream:
 *   1. ops_frame_adjoint_rhs_f64:    rhs [B,Nn,3] = g_disp + sum over each node's elements of (K_e g_f,e)[that end], where
 *                                    g_f = g_forces with gV added to component 1 and gM to component 2, K_e with the frame's own I_e;
 *   2. ops_frame_solve_batched_f64_ex with loads = rhs (loads_bstride = n_nodes * 3) and an all-zero elem_w: its disp is lambda
 *      (0 on constrained DOFs; values of rhs there are ignored).  The assembly plan holds the consistent loads of elem_w, so a
 *      plan built with the forward's elem_w must NOT be reused here: flags = 0, or a workspace of the adjoint's own;
 *   3. ops_frame_grad_contract_f64:  gI [B,Ne] = (g_f,e - lambda_e) . (K_b,e u_e),  K_e = K_ax,e + I_e K_b,e.
 * dL/dloads = lambda, per frame.  E, A, the geometry and the element loads get no gradient.
 *   elem_geo [Ne,3], elem_EA [Ne], elem_E [Ne]: as in ops_frame_solve_batched_f64;  conn [Ne,2]: the node numbers of each element's ends;
 *   node_elem_ptr [Nn+1] / node_elem_idx [2 Ne]: per node, its incident element ends as 2 * element + end (CSR; any degree);
 *   I [B,Ne]; disp, lambda [B,Nn,3]: the forward's and the adjoint solve's displacements;
 *   cotangents g_disp [B,Nn,3], g_forces [B,Ne,6], gV, gM [B,Ne]: dense, NULL = zeros (bit for bit);
 *   status_fwd / status_adj [B] (either may be NULL): a frame with a non-zero status gets NaN in its gI row (its lambda is NaN already).
 * No atomics: the results are reproducible and do not depend on B.  B == 0: OK; a negative size, n_nodes < 2, n_elems < 1 or a NULL
 * required pointer: ERR_INVALID_ARG.  One launch each.  Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_FRAME_VJP_H
#define OPENPYSTRUCT_AMD_FRAME_VJP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int ops_frame_adjoint_rhs_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA,
                              const double* elem_E, const int32_t* conn, const int32_t* node_elem_ptr,
                              const int32_t* node_elem_idx, const double* I, const double* g_disp,
                              const double* g_forces, const double* gV, const double* gM, double* rhs, void* stream);
int ops_frame_grad_contract_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                                const int32_t* conn, const double* disp, const double* lambda,
                                const double* g_forces, const double* gV, const double* gM,
                                const int32_t* status_fwd, const int32_t* status_adj, double* gI, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_FRAME_VJP_H */
