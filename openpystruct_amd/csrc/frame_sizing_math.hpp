// Arithmetic of the exact-gradient frame sizing objective, per node and per element: plain C++ that compiles
// for the device (csrc/frame_sizing_grad.hip) and with g++ for the host (tests/test_frame_sizing_grad_host.py builds a
// stand-alone program from this file).  Nothing is restated: the objective's cotangents and its explicit part are the
// functions of sizing_grad_math.hpp (the beam objective's: sizing_quot, sizing_gM, sizing_gV, sizing_explicit, sizing_defl,
// sizing_gv); the element stiffness, the node walk and the end-node contraction are fa_apply_k, fa_scatter_k and fa_contract
// of frame_adjoint.hpp.
//
//   L(I) = sum_e I_e + aM sum_e M_e^2 / (2 E I_e + bend_eps) + aV sum_e V_e^2 / (G area_coef sqrt(I_e))
//        + aS sum_n h(|ux_n|, s_lim) + aD sum_n h(|uy_n|, d_lim),      h(a, lim) = (max(0, a - lim) / lim)^2
//   rhs   r[n,:] = (gv_s(ux_n), gv_d(uy_n), 0) + sum over the elements e at node n of (K_e g_f,e)[end of e at n],
//         g_f,e = (0, gV_e, gM_e, 0, 0, 0): §9f's fold with g_forces = 0
//   grad  dL/dI_e = sizing_explicit + (g_f,e - lambda_e) . (K_b,e u_e)
// The cotangents are formed from (I, V, M) and disp where they are used and live in registers only.
#pragma once

#include "frame_adjoint.hpp"
#include "sizing_grad_math.hpp"

namespace opsamd {

// the objective's constants: SizingObj once per hinge -- `sway` carries (aS, s_lim) in (aD, vlim) and is applied to ux, `defl`
// carries (aD, d_lim) and is applied to uy; the element constants are the same in both
struct FrameSizingObj { SizingObj sway, defl; };

FA_HD FrameSizingObj frame_sizing_obj(double aM, double aV, double E, double bend_eps, double G, double area_coef, double aS,
                                      double s_lim, double aD, double d_lim) {
  const SizingObj s{aM, aV, 2.0 * E, bend_eps, G * area_coef, aS, aS > 0.0 ? s_lim : 1.0};
  const SizingObj d{aM, aV, 2.0 * E, bend_eps, G * area_coef, aD, aD > 0.0 ? d_lim : 1.0};
  return FrameSizingObj{s, d};
}

// the folded cotangent of element row `row` (= frame * Ne + element) from this epoch's forward
FA_HD void fs_fold(const SizingObj& o, const SizingQuot& q, double gf[6]) {
  gf[0] = 0.0; gf[1] = sizing_gV(o, q); gf[2] = sizing_gM(o, q);
  gf[3] = 0.0; gf[4] = 0.0; gf[5] = 0.0;
}

// The three adjoint loads of node n of frame b (fa_node_rhs with the objective's cotangents in place of arrays: the same walk,
// fa_scatter_k).  Returns the node's share of the two hinge terms.  sizing_defl compares, and a comparison drops a NaN: a NaN
// displacement (a frame whose forward failed) is forwarded to the returned value by hand.
FA_HD double fs_node_rhs(const FrameSizingObj& o, int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA,
                         const double* elem_E, const int32_t* node_elem_ptr, const int32_t* node_elem_idx, const double* I,
                         const double* disp, const double* V, const double* M, long b, int n, double r[3]) {
  const long node = b * n_nodes + n;
  const double ux = disp[node * 3], uy = disp[node * 3 + 1];
  r[0] = sizing_gv(o.sway, ux);
  r[1] = sizing_gv(o.defl, uy);
  r[2] = 0.0;
  fa_scatter_k(n_elems, elem_geo, elem_EA, elem_E, node_elem_ptr, node_elem_idx, I, b, n, r,
               [&](long row, double gf[6]) { fs_fold(o.sway, sizing_quot(o.sway, I[row], V[row], M[row]), gf); });
  const double h = sizing_defl(o.sway, ux) + sizing_defl(o.defl, uy);
  return (ux != ux || uy != uy) ? ux + uy : h;
}

// dL/dI of element e of frame b from the forward's (I, V, M, disp) and the adjoint's displacements lambda: the explicit part plus
// fa_contract of the objective's cotangents
FA_HD double fs_elem_grad(const FrameSizingObj& o, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                          const int32_t* conn, const double* I, const double* V, const double* M, const double* disp,
                          const double* lambda, long b, int e) {
  const long row = b * n_elems + e;
  const double Ie = I[row], Ve = V[row];
  const SizingQuot q = sizing_quot(o.sway, Ie, Ve, M[row]);
  double gf[6];
  fs_fold(o.sway, q, gf);
  return sizing_explicit(o.sway, Ie, Ve, q) + fa_contract(n_nodes, elem_geo, elem_E, conn, disp, lambda, gf, b, e);
}

}  // namespace opsamd

#if defined(__HIPCC__)
// ---- host side of the entries that take the objective (frame_sizing_grad.hip, frame_designs.hip, frame_groups.hip) ----
#include <type_traits>

#include "../../include/openpystruct_amd_frame_sizing.h"

namespace opsamd {

// the objective from the C structs; (0, 0, 0, 0): without its hinges, which reach a gradient through lambda alone
inline FrameSizingObj frame_sizing_obj(const ops_sizing_params* hp, double aS, double s_lim, double aD, double d_lim) {
  return frame_sizing_obj(hp->alpha_moment, hp->alpha_shear, hp->E, hp->bend_eps, hp->G, hp->area_coef, aS, s_lim, aD, d_lim);
}

// what an adjoint right-hand-side entry refuses of its objective: a weight below zero (or NaN), a weighted hinge without a
// positive limit, or without `loss_extra` to take its value
inline int frame_sizing_obj_check(const ops_frame_sizing_objective* obj, const double* loss_extra) {
  if (!(obj->alpha_sway >= 0.0) || !(obj->alpha_deflection >= 0.0)) return OPS_AMD_ERR_INVALID_ARG;
  if (obj->alpha_sway > 0.0 && !(obj->sway_limit > 0.0)) return OPS_AMD_ERR_INVALID_ARG;
  if (obj->alpha_deflection > 0.0 && !(obj->deflection_limit > 0.0)) return OPS_AMD_ERR_INVALID_ARG;
  if (obj->alpha_sway + obj->alpha_deflection > 0.0 && !loss_extra) return OPS_AMD_ERR_INVALID_ARG;
  return OPS_AMD_OK;
}

// f(std::integral_constant<int, W>) with W the lanes per row of the right-hand-side kernels: the smallest of 4 .. 64 that is
// >= min(n_nodes, 64).  frame_rhs_threads: a wavefront per 64 / W rows, as frame_stream_launch's count of one thread per row
inline long frame_rhs_threads(int B, int W) { return (((long)B + 64 / W - 1) / (64 / W)) * 64; }
template <class F>
int frame_rhs_width(int n_nodes, F f) {
  if (n_nodes <= 4) return f(std::integral_constant<int, 4>{});
  if (n_nodes <= 8) return f(std::integral_constant<int, 8>{});
  if (n_nodes <= 16) return f(std::integral_constant<int, 16>{});
  if (n_nodes <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

}  // namespace opsamd
#endif
