// Per-lane arithmetic of the exact-gradient sizing objective (sizing_grad.hip).
//
// The objective, in float64 on the widened float32 inertias:
//   L(I) = sum_e I_e + aM sum_e M_e^2 / (2 E I_e + bend_eps) + aV sum_e V_e^2 / (G area_coef sqrt(I_e))
//        + aD sum_n (max(0, |v_n| - v_lim) / v_lim)^2
// M, V, v depend on I through K(I) u = f, so dL/dI is the explicit part (M, V held fixed) plus the beam solve's VJP
// (beam_adjoint.hpp) with the cotangents gM = dL/dM, gV = dL/dV, gv = dL/dv, gt = 0.  Everything here is a function of one
// element's (I, V, M) or one node's v; per element the two quotients
//   qM = M / (2 E I + bend_eps),   qV = V / (G area_coef sqrt(I))
// carry every division and the square root but one: gM = 2 aM qM, gV = 2 aV qV, and the explicit part is
//   1 - aM 2E qM^2 - aV (V qV / 2) / I       (V^2 / 2 / (G area_coef I^1.5) = V qV / (2 I)).
// Like beam_adjoint.hpp this header has no I/O and no cross-lane traffic; g++ compiles it for tests/csrc/emul_sizing_grad.cpp.
#pragma once

#include "beam_adjoint.hpp"

namespace opsamd {

// the objective's constants as the lanes use them (from ops_sizing_params and ops_sizing_objective)
struct SizingObj {
  double aM, aV, twoE, bend_eps, Gac;   // Gac = G * area_coef
  double aD, vlim;                      // aD == 0: no deflection term (vlim unused)
};

struct SizingQuot { double qV, qM; };

BEAM_HD SizingQuot sizing_quot(const SizingObj& o, double Ie, double V, double M) {
  return SizingQuot{V / (o.Gac * __builtin_sqrt(Ie)), M / (o.twoE * Ie + o.bend_eps)};
}
BEAM_HD double sizing_gV(const SizingObj& o, const SizingQuot& q) { return 2.0 * o.aV * q.qV; }
BEAM_HD double sizing_gM(const SizingObj& o, const SizingQuot& q) { return 2.0 * o.aM * q.qM; }

// dL/dI_e with M, V held fixed
BEAM_HD double sizing_explicit(const SizingObj& o, double Ie, double V, const SizingQuot& q) {
  return 1.0 - o.aM * o.twoE * (q.qM * q.qM) - o.aV * (0.5 * V * q.qV) / Ie;
}

// one node's share of the deflection term and its derivative with respect to v_n
BEAM_HD double sizing_defl(const SizingObj& o, double v) {
  const double ex = __builtin_fabs(v) - o.vlim;
  if (!(o.aD > 0.0) || !(ex > 0.0)) return 0.0;
  const double r = ex / o.vlim;
  return o.aD * (r * r);
}
BEAM_HD double sizing_gv(const SizingObj& o, double v) {
  const double ex = __builtin_fabs(v) - o.vlim;
  if (!(o.aD > 0.0) || !(ex > 0.0)) return 0.0;
  return 2.0 * o.aD * (v < 0.0 ? -ex : ex) / (o.vlim * o.vlim);
}

}  // namespace opsamd
