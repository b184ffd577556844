/* openpystruct_amd -- C ABI, extension header: several load cases per frame on one kept factorisation.
 *
 * An addition to include/openpystruct_amd.h: three entry points of the same shared library, the same
 * conventions -- DEVICE pointers owned by the caller, nothing allocated, copied or synchronised inside, work enqueued on `stream`
 * (a hipStream_t passed as void*), return codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration of that header:
 * OPS_AMD_ABI_VERSION stays what it is.
 *
 * ops_frame_solve_batched_f64 factorises K(I) in every call.  Here the factorisation is kept:
 *   1. ops_frame_factor_solve_f64: ops_frame_solve_batched_f64 (same arguments, same outputs for its own loads and elem_w, equal to
 *      that entry's tolerances -- not bit for bit: it always takes the wave-per-frame kernel, whatever B is) that leaves K = L D L^T
 *      of every frame in `factor`.  status[b] != 0: that frame's factorisation failed.  The factor stays valid until the buffer is
 *      next written; it belongs to (I, the topology arrays) of this call.
 *   2. ops_frame_resolve_f64: K(I_b) x = rhs_{b,c} for C right-hand sides per frame by substitution alone, and forces = K_e u_e with
 *      NO element loads (the form the adjoint and the per-frame element-load paths use: include/openpystruct_amd_frame_vjp.h,
 *      include/openpystruct_amd_frame_loads.h).  One launch.  Outputs are [B,C,...], row b * C + c; status is [B,C].
 *        rhs [B,C,Nn,3] (rhs_bstride = C * n_nodes * 3) or [C,Nn,3] shared by all frames (rhs_bstride = 0); values on constrained
 *        DOFs are ignored;  factor_status [B]: the keeping solve's status -- a frame with a non-zero one gets NaN rows and status 1
 *        in all C cases and its factor is not read;  I [B,Ne], the topology arrays, n_eq, half_bandwidth: those of the keeping solve.
 *      With rhs = the keeping solve's loads, C = 1 and that solve's elem_w all zero the outputs are the keeping solve's bit for bit;
 *      the results of (b, c) depend on that frame's factor and that right-hand side alone -- not on B, C or the position.
 *   ops_frame_factor_workspace_bytes: the size of `factor` for B frames; 0: the shape is not served.
 * Served: half_bandwidth <= 55 and frames whose four waves fit the LDS of a compute unit (the wave-per-frame kernel's own
 * limits); anything else is OPS_AMD_ERR_UNSUPPORTED (ops_frame_solve_batched_f64 serves every shape).
 * B == 0 or C == 0: OK, nothing is launched.  A negative size, n_nodes < 2, n_elems < 1, n_eq < 1, a stride other than the two
 * allowed values, a NULL pointer (status of the keeping solve may be NULL, everything else is required) or a factor_bytes below
 * ops_frame_factor_workspace_bytes: ERR_INVALID_ARG.  Both are decided before any HIP call and nothing is written.
 * Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_FRAME_CASES_H
#define OPENPYSTRUCT_AMD_FRAME_CASES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t ops_frame_factor_workspace_bytes(int B, int n_eq, int half_bandwidth);
int ops_frame_factor_solve_f64(int B, int n_nodes, int n_elems, int n_eq, int half_bandwidth,
                               const double* elem_geo, const double* elem_EA, const double* elem_E,
                               const double* elem_w, const int32_t* elem_eq, const int32_t* node_eq,
                               const double* I, const double* loads, long loads_bstride, double* disp,
                               double* forces, double* V, double* M, int32_t* status, void* factor,
                               size_t factor_bytes, void* stream);
int ops_frame_resolve_f64(int B, int C, int n_nodes, int n_elems, int n_eq, int half_bandwidth,
                          const double* elem_geo, const double* elem_EA, const double* elem_E,
                          const int32_t* elem_eq, const int32_t* node_eq, const double* I,
                          const double* rhs, long rhs_bstride, const int32_t* factor_status,
                          double* disp, double* forces, double* V, double* M, int32_t* status,
                          const void* factor, size_t factor_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_FRAME_CASES_H */
