// Arithmetic of per-frame element loads around the batched frame solve, per node and per element: plain
// C++ that compiles for the device (csrc/frame_loads.hip) and with g++ for the host (tests/test_frame_loads_host.py builds
// a stand-alone program from this file).  No dependence on the band kernels: the solve is linear in the element loads, so
// the solve under (loads, w) is the solve under loads + scatter(pg) with NO element loads, then forces_e -= pg_e.
//
//   pg_e      R_e^T [wx L/2, wy L/2, wy L^2/12, wx L/2, wy L/2, -wy L^2/12]: the consistent loads of beamUniform(wy, wx),
//             global, the expression of csrc/frame_wave.hpp (frame_plan_kernel)
//   rhs       r[n,:] = loads[n,:] + sum over the elements e at node n of pg_e[3 end .. 3 end + 2]
//   forces    forces_e -= pg_e
//   vjp       g_w[e,0] = (lambda_e - g_f,e) . dpg_e/dwy,  g_w[e,1] = (lambda_e - g_f,e) . dpg_e/dwx
#pragma once
#include <stdint.h>

#include "frame_adjoint.hpp"

namespace opsamd {

// consistent global end loads of beamUniform(wy, wx) on an element of length L and direction (c, s)
FA_HD void fl_pg(double L, double c, double s, double wy, double wx, double pg[6]) {
  const double pl[6] = {wx * L / 2, wy * L / 2, wy * L * L / 12, wx * L / 2, wy * L / 2, -wy * L * L / 12};
  pg[0] = c * pl[0] - s * pl[1];
  pg[1] = s * pl[0] + c * pl[1];
  pg[2] = pl[2];
  pg[3] = c * pl[3] - s * pl[4];
  pg[4] = s * pl[3] + c * pl[4];
  pg[5] = pl[5];
}

// the three loads of node n of frame b: its own nodal load plus the consistent loads of its incident element ends, in the one
// fixed order of fa_walk (frame_adjoint.hpp).  loads_bstride: 0 (one [Nn,3] for the batch) or 3 Nn; w_bstride: 0 (one [Ne,2])
// or 2 Ne
FA_HD void fl_node_rhs(int n_nodes, const double* elem_geo, const int32_t* node_elem_ptr, const int32_t* node_elem_idx,
                       const double* loads, long loads_bstride, const double* elem_w, long w_bstride, long b, int n,
                       double r[3]) {
  const double* ld = loads + b * loads_bstride + 3 * (long)n;
  const double* w = elem_w + b * w_bstride;
  for (int k = 0; k < 3; ++k) r[k] = ld[k];
  fa_walk(node_elem_ptr, node_elem_idx, n, r, [&](int e, double pg[6]) {
    fl_pg(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], w[2 * e], w[2 * e + 1], pg);
  });
}

// f (the six global end forces of element e of frame b, solved without element loads) -= pg_e
FA_HD void fl_elem_forces(const double* elem_geo, const double* elem_w, long w_bstride, long b, int e, double f[6]) {
  const double* w = elem_w + b * w_bstride;
  double pg[6];
  fl_pg(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], w[2 * e], w[2 * e + 1], pg);
  for (int k = 0; k < 6; ++k) f[k] -= pg[k];
}

// (g_wy, g_wx) of element e of frame b from the adjoint displacements (lambda: zero on constrained DOFs) and the folded
// cotangent of the forces; pg is linear in (wy, wx), so its derivatives are pg of the unit loads.  The difference is lambda - g_f,
// the negative of fa_contract's: the sign of a zero sum depends on it, so the contraction is this function's own
FA_HD void fl_elem_gw(int n_nodes, int n_elems, const double* elem_geo, const int32_t* conn, const double* lambda,
                      const double* g_forces, const double* gV, const double* gM, long b, int e, double gw[2]) {
  double gf[6], d[6], dy[6], dx[6];
  fa_gather(n_nodes, conn, lambda, b, e, d);      // (before the fold: fewer live registers on the device)
  fa_fold(g_forces, gV, gM, b * n_elems + e, gf);
  for (int k = 0; k < 6; ++k) d[k] -= gf[k];
  fl_pg(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], 1.0, 0.0, dy);
  fl_pg(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], 0.0, 1.0, dx);
  double ay = 0.0, ax = 0.0;
  for (int k = 0; k < 6; ++k) {
    ay += d[k] * dy[k];
    ax += d[k] * dx[k];
  }
  gw[0] = ay;
  gw[1] = ax;
}

}  // namespace opsamd
