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
 * ERR_INVALID_ARG, nothing is written.  One launch each.  Never throws, never blocks.
 *
 * Natural frequencies and mode shapes on the kept factorisation: three more entry points on the same node-walk
 * tables, same conventions.  The problem is K(I) phi = lambda M phi on the free DOFs, K the matrix ops_frame_factor_solve_f64
 * (include/openpystruct_amd_frame_cases.h) factorises, M = element mass (mass per unit length elem_mass [Ne]; consistent != 0: the
 * rotated consistent 6 x 6 matrix, 0: lumped, elem_mass L / 2 on the four translations) + nodal masses; M does not depend on I.
 * One iteration of the subspace iteration on p <= 8 vectors is three calls on one stream, R [B,p,Nn,3] = M Q of the iteration before
 * (at the start M X0, X0 zero on constrained DOFs):
 *   1. ops_frame_resolve_f64 with C = p, rhs = R (rhs_bstride = p * n_nodes * 3): disp = X = K^-1 R [B,p,Nn,3], status = row_status;
 *   2. ops_frame_mass_apply_f64:  y[r] = M x[r] for R rows [R,Nn,3], one thread per (row, node): the node's own nodal term, then its
 *      incident element ends in table order.  nodal_mass [Nn,3] (nodal_bstride 0), [B,Nn,3] (nodal_bstride 3 Nn; the frame of row r
 *      is r / rows_per_frame) or NULL (none);
 *   3. ops_frame_modes_ritz_f64:  one wavefront per frame.  Kr = sym(X^T R), Mr = X^T MX, Mr = G G^T, A = G^-1 Kr G^-T, cyclic Jacobi
 *      on A in row-cyclic order until the off-diagonal sum of squares is at most (2^-52 trace)^2, or 16 sweeps; Ritz values
 *      ascending into lambda [B,p]; Z = G^-T V; Q = X Z (M-orthonormal); R <- MX Z.  change [B,p] = |lambda - lambda_prev| / lambda
 *      with lambda_prev what `lambda` held at the call: the caller fills it with +inf before the first iteration, which gives
 *      change = +inf there.  status [B]: 0; 1 when any of the frame's p row_status is non-zero (the keeping solve or a re-solve row
 *      failed); 2 when Mr is not positive definite (p exceeds the number of DOFs that carry mass).  A frame with a non-zero status
 *      gets NaN in Q, lambda and change and keeps its R; no other frame is touched.  The dot products are per-lane strided partial
 *      sums added by a fixed butterfly: no atomics, the same bits for every B and every place in the batch.
 * ops_frame_modes_grad_f64: gI[b,e] = sum over j < m, in mode order, of g_lambda[b,j] phi_j,e . (K_b,e phi_j,e), K_b,e the bending part
 * of the rotated stiffness per unit inertia; phi [B,p,Nn,3] M-normalised, g_lambda [B,m], 1 <= m <= p; a frame with status[b] != 0
 * gets a NaN row.  One thread per (frame, element).
 * R == 0 / B == 0: OK, nothing is launched; a negative size, rows_per_frame < 1, n_nodes < 2, n_elems < 1, p outside 1..8, m outside
 * 1..p, a stride other than the two allowed values or a NULL pointer (nodal_mass alone may be NULL): ERR_INVALID_ARG, decided
 * before any HIP call, nothing is written.
 *
 * Linear buckling load factors on the kept factorisation: three more entry points, same tables, same conventions.
 * The problem is K(I) phi = lambda S phi on the free DOFs, S = -K_g(N) the negated geometric stiffness of the axial forces
 * N_e = ((c f3 + s f4) - (c f0 + s f1)) / 2 (tension positive) of `forces` [B,Ne,6], the global end forces of a reference static
 * solve of the same frames; consistent != 0: N / (30 L) [[36, 3L, -36, 3L], [3L, 4L^2, -3L, -L^2], [-36, -3L, 36, -3L], [3L, -L^2,
 * -3L, 4L^2]] on the local (v1, th1, v2, th2), rotated; 0: N / L [[1, -1], [-1, 1]] on (v1, v2), the linearised P-Delta matrix.  S is
 * indefinite and may be rank deficient, so the iteration is the inverse iteration on K^-1 S, R [B,p,Nn,3] = S Q of the iteration
 * before (at the start S X0, X0 zero on constrained DOFs):
 *   1. ops_frame_resolve_f64 with C = p, rhs = R: disp = X = K^-1 R, status = row_status;
 *   2. ops_frame_geom_apply_f64:  y[r] = S x[r] for R rows [R,Nn,3] (the frame of row r is r / rows_per_frame), one thread per (row,
 *      node), the node's incident element ends in table order;
 *   3. ops_frame_buckling_ritz_f64:  one wavefront per frame.  Kr = sym(X^T R) (= X^T K X), Sr = X^T SX, Kr = G G^T, A = G^-1 Sr G^-T,
 *      cyclic Jacobi in row-cyclic order until the off-diagonal sum of squares is at most (2^-52)^2 times the sum of all squares of
 *      A, or 16 sweeps; Ritz values DESCENDING into mu [B,p]; lambda [B,p] = 1 / mu where mu > 0, else +inf; Z = G^-T V; Q = X Z
 *      (K-orthonormal: Q^T S Q = diag(mu)); R <- SX Z.  change [B,p] = |mu - mu_prev| / |mu| with mu_prev what `mu` held at the call
 *      (the caller fills it with +inf before the first iteration).  status [B]: 0; 1 when any of the frame's p row_status is
 *      non-zero; 2 when Kr is not positive definite: a Cholesky pivot at or below 2^-40 of its diagonal entry (p exceeds the rank
 *      of S, or the start is dependent; in both the pivot is rounding noise of either sign).  A frame with a non-zero
 *      status gets NaN in Q, mu, lambda and change and keeps its R; no other frame is touched.  No atomics, no LDS: the same bits for
 *      every B and every place in the batch.
 * ops_frame_buckling_grad_f64, one thread per (frame, element), the sums over j < m in mode order and over finite lambda alone:
 *   gI_direct[b,e] = sum_j g_lambda[b,j] lambda[b,j] phi_j,e . (K_b,e phi_j,e),
 *   g_forces[b,e,:] = (sum_j g_lambda[b,j] lambda[b,j]^2 phi_j,e . (k_g,unit,e phi_j,e)) (-c/2, -s/2, 0, c/2, s/2, 0),
 * the cotangent of the reference solve's end forces: dlambda/dI = gI_direct + the gI of that solve's vector-Jacobian product
 * (include/openpystruct_amd_frame_cases.h).  phi [B,p,Nn,3] K-normalised, lambda and g_lambda [B,m], 1 <= m <= p, `consistent` the
 * kind of the geometric matrix; a frame with status[b] != 0 gets NaN rows.
 * Refusals as above: R == 0 / B == 0: OK; a negative size, rows_per_frame < 1, n_nodes < 2, n_elems < 1, p outside 1..8, m outside
 * 1..p or a NULL pointer: ERR_INVALID_ARG, decided before any HIP call, nothing is written. */
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
int ops_frame_mass_apply_f64(int R, int rows_per_frame, int n_nodes, int n_elems, const double* elem_geo, const int32_t* conn,
                             const int32_t* node_elem_ptr, const int32_t* node_elem_idx, const double* elem_mass, int consistent,
                             const double* nodal_mass, long nodal_bstride, const double* x, double* y, void* stream);
int ops_frame_modes_ritz_f64(int B, int p, int n_nodes, const double* X, const double* MX, double* R, double* Q,
                             double* lambda, double* change, const int32_t* row_status, int32_t* status, void* stream);
int ops_frame_modes_grad_f64(int B, int m, int p, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                             const int32_t* conn, const double* phi, const double* g_lambda, const int32_t* status, double* gI,
                             void* stream);
int ops_frame_geom_apply_f64(int R, int rows_per_frame, int n_nodes, int n_elems, const double* elem_geo, const int32_t* conn,
                             const int32_t* node_elem_ptr, const int32_t* node_elem_idx, const double* forces, int consistent,
                             const double* x, double* y, void* stream);
int ops_frame_buckling_ritz_f64(int B, int p, int n_nodes, const double* X, const double* SX, double* R, double* Q, double* mu,
                                double* lambda, double* change, const int32_t* row_status, int32_t* status, void* stream);
int ops_frame_buckling_grad_f64(int B, int m, int p, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                                const int32_t* conn, int consistent, const double* phi, const double* lambda,
                                const double* g_lambda, const int32_t* status, double* gI_direct, double* g_forces, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_FRAME_LOADS_H */
