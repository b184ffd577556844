// Arithmetic of the frame solve's vector-Jacobian product, per node and per element: plain C++ that
// compiles for the device (csrc/frame_vjp.hip) and with g++ for the host (tests/test_frame_vjp_host.py builds a
// stand-alone program from this file).  No dependence on the band kernels: the adjoint solve between the two steps is
// one more call of ops_frame_solve_batched_f64_ex.  The node walk (fa_walk, fa_scatter_k), the end-node gather (fa_gather) and
// the contraction (fa_contract) are stated here once: frame_sizing_math.hpp (§9h) and frame_loads.hpp (§9i) are built on them.
//
//   fold      g_f = g_forces, gV added to component 1, gM to component 2
//   rhs       r[n,:] = g_disp[n,:] + sum over the elements e at node n of (K_e g_f,e)[end of e at n]
//   contract  gI[e] = (g_f,e - lambda_e) . (K_b,e u_e),   K_e = K_ax,e + I_e K_b,e
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FA_HD __host__ __device__ inline
#else
#define FA_HD inline
#endif

namespace opsamd {

// y = K_e x for the six global end DOFs (ux1, uy1, rz1, ux2, uy2, rz2) of an ElasticBeam2d of length L and direction
// (c, s): the element end-force expression of csrc/frame_solve.hip (write_results) without element loads -- rotate to local
// axes, basic forces q0 (axial), q1, q2 (end moments), back to global.  EA = 0, EI = E gives K_b,e x.
FA_HD void fa_apply_k(double L, double c, double s, double EA, double EI, const double x[6], double y[6]) {
  const double ul0 = c * x[0] + s * x[1], ul1 = -s * x[0] + c * x[1], ul2 = x[2];
  const double ul3 = c * x[3] + s * x[4], ul4 = -s * x[3] + c * x[4], ul5 = x[5];
  const double rL = 1.0 / L, chord = (ul4 - ul1) * rL, b2 = 2.0 * EI * rL;
  const double q0 = EA * rL * (ul3 - ul0);
  const double q1 = 2.0 * b2 * (ul2 - chord) + b2 * (ul5 - chord);
  const double q2 = b2 * (ul2 - chord) + 2.0 * b2 * (ul5 - chord);
  const double sh = (q1 + q2) * rL;
  y[0] = c * (-q0) - s * sh;
  y[1] = s * (-q0) + c * sh;
  y[2] = q1;
  y[3] = c * q0 + s * sh;
  y[4] = s * q0 - c * sh;
  y[5] = q2;
}

// the folded cotangent of element row `row` (= frame * Ne + element); a NULL cotangent reads as zeros through the same
// additions, so NULL and explicit zeros give the same bits
FA_HD void fa_fold(const double* g_forces, const double* gV, const double* gM, long row, double gf[6]) {
  for (int k = 0; k < 6; ++k) gf[k] = g_forces ? g_forces[row * 6 + k] : 0.0;
  gf[1] += gV ? gV[row] : 0.0;
  gf[2] += gM ? gM[row] : 0.0;
}

// The node walk, stated once: r[0..2] += the three components at node n of every incident element end's six-vector.  The node's
// incident (element, end) pairs are node_elem_idx[node_elem_ptr[n] .. node_elem_ptr[n + 1]) as 2 * element + end, in one fixed
// order -- the sum is reproducible and independent of the batch.  end_vector(e, y) fills the six global end values of element e.
template <class EndVector>
FA_HD void fa_walk(const int32_t* node_elem_ptr, const int32_t* node_elem_idx, int n, double r[3], EndVector end_vector) {
  for (int p = node_elem_ptr[n]; p < node_elem_ptr[n + 1]; ++p) {
    const int e = node_elem_idx[p] >> 1, end = node_elem_idx[p] & 1;
    double y[6];
    end_vector(e, y);
    for (int k = 0; k < 3; ++k) r[k] += y[3 * end + k];
  }
}

// the walk with K_e g_f,e as the end vector; fold(row, gf) fills the folded cotangent of element row `row` (= b * n_elems + e)
template <class Fold>
FA_HD void fa_scatter_k(int n_elems, const double* elem_geo, const double* elem_EA, const double* elem_E,
                        const int32_t* node_elem_ptr, const int32_t* node_elem_idx, const double* I, long b, int n, double r[3],
                        Fold fold) {
  fa_walk(node_elem_ptr, node_elem_idx, n, r, [&](int e, double y[6]) {
    const long row = b * n_elems + e;
    double gf[6];
    fold(row, gf);
    fa_apply_k(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], elem_EA[e], elem_E[e] * I[row], gf, y);
  });
}

// the six end values of element e of frame b from a per-node array x [B,Nn,3]
FA_HD void fa_gather(int n_nodes, const int32_t* conn, const double* x, long b, int e, double out[6]) {
  const long n1 = b * n_nodes + conn[2 * e], n2 = b * n_nodes + conn[2 * e + 1];
  for (int k = 0; k < 3; ++k) {
    out[k] = x[n1 * 3 + k];
    out[3 + k] = x[n2 * 3 + k];
  }
}

// the contraction, stated once: (g_f,e - lambda_e) . (K_b,e u_e) of element e of frame b for a folded cotangent gf
FA_HD double fa_contract(int n_nodes, const double* elem_geo, const double* elem_E, const int32_t* conn, const double* disp,
                         const double* lambda, const double gf[6], long b, int e) {
  double u[6], lam[6], y[6];
  fa_gather(n_nodes, conn, disp, b, e, u);
  fa_gather(n_nodes, conn, lambda, b, e, lam);
  fa_apply_k(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], 0.0, elem_E[e], u, y);
  double acc = 0.0;
  for (int k = 0; k < 6; ++k) acc += (gf[k] - lam[k]) * y[k];
  return acc;
}

// the three adjoint loads of node n of frame b
FA_HD void fa_node_rhs(int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA, const double* elem_E,
                       const int32_t* node_elem_ptr, const int32_t* node_elem_idx, const double* I, const double* g_disp,
                       const double* g_forces, const double* gV, const double* gM, long b, int n, double r[3]) {
  const long node = b * n_nodes + n;
  for (int k = 0; k < 3; ++k) r[k] = g_disp ? g_disp[node * 3 + k] : 0.0;
  fa_scatter_k(n_elems, elem_geo, elem_EA, elem_E, node_elem_ptr, node_elem_idx, I, b, n, r,
               [&](long row, double gf[6]) { fa_fold(g_forces, gV, gM, row, gf); });
}

// gI of element e of frame b from the forward's displacements and the adjoint's (lambda: zero on constrained DOFs, as disp is)
FA_HD double fa_elem_gI(int n_nodes, int n_elems, const double* elem_geo, const double* elem_E, const int32_t* conn,
                        const double* disp, const double* lambda, const double* g_forces, const double* gV,
                        const double* gM, long b, int e) {
  double gf[6];
  fa_fold(g_forces, gV, gM, b * n_elems + e, gf);
  return fa_contract(n_nodes, elem_geo, elem_E, conn, disp, lambda, gf, b, e);
}

}  // namespace opsamd
