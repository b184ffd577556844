// Per-lane arithmetic of the beam-solve vector-Jacobian product (beam_vjp.hip).
//
// The forward solves K(I) u = f on the free DOFs (beam_math.hpp).  Its VJP is one more solve with the SAME matrix,
//   K lambda = g_u,   g_u = [gv; gt] + sum_e k_e^T [gV_e, gM_e, 0, 0]^T   (masked to the free DOFs),
// followed by per-element contractions with lambda and the forward's u.  K is symmetric, so the adjoint solve is the
// forward's substructured block Cholesky with another right-hand side: the factorisation statements below are those of
// seg_condense / seg_solve, and the interface system goes through the unchanged make_row / cr_eliminate / cr_back.
// What differs is the load: the forward hard-codes the consistent UDL pair (pw, mw) / (pw, -mw) plus a nodal Fy; the
// adjoint load of an element is a general 4-vector (adj_elem_load), and the nodal part has a rotation component.
//
// Recovery in the forward (seg_solve): with r = k_e u_e,  V_e = r_0 - pw_e,  M_e = r_1 - mw_e.  Hence, with the unit-
// inertia stiffness k^_e = k_e / I_e, r^ = k^_e u_e and lambda_e = [lambda_a; lambda_b] on the element's two nodes:
//   gI_e  = gV r^_0 + gM r^_1 - lambda_e . r^                      (dk_e/dI_e = k^_e; r^_2 = -r^_0)
//   gwy_e = lambda_e . (L/2, L^2/12, L/2, -L^2/12) - gV L/2 - gM L^2/12
//   gFy_n = lambda_v(n)                                              (zero on fixed DOFs: lambda is)
// Like beam_math.hpp this header has no I/O and no cross-lane traffic; g++ compiles it for tests/csrc/emul_beam_vjp.cpp.
#pragma once

#include "beam_math.hpp"

namespace opsamd {

// One element as the adjoint sweeps see it: the forward's unit-inertia tile entries, length, inertia, cotangents.
struct AdjElem { double c2, c6, c12, L, Ie, gV, gM; };

// A real element: the entries exactly as beam_solve.hip's stage 0 computes them (same factorisation, bit for bit).
BEAM_HD AdjElem adj_elem_real(double L, double E, double Ie, double gV, double gM) {
  const double rl = fast_rcp(L);
  const double c2 = 2.0 * E * rl, c6 = 3.0 * c2 * rl, c12 = 2.0 * c6 * rl;
  return AdjElem{c2, c6, c12, L, Ie, gV, gM};
}
// The forward's padding: element Ne has no stiffness, the elements beyond it are unit elements; neither carries a load.
BEAM_HD AdjElem adj_elem_pad(bool unit) {
  return unit ? AdjElem{2.0, 6.0, 12.0, 1.0, 1.0, 0.0, 0.0} : AdjElem{0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
}

// k_e^T [gV, gM, 0, 0]^T = gV k_e[:,0] + gM k_e[:,1], split by node: a (left), b (right)
struct ElemLoad { Vec2 a, b; };
BEAM_HD ElemLoad adj_elem_load(const ElemK& k, double gV, double gM) {
  const double sv = __builtin_fma(gV, k.kA, gM * k.kB);
  return ElemLoad{Vec2{sv, __builtin_fma(gV, k.kB, gM * k.kC)}, Vec2{-sv, __builtin_fma(gV, k.kB, gM * k.kD)}};
}

// (gI, gwy) of one element from lambda and u on its two nodes (see the header comment).
BEAM_HD void adj_elem_grads(const AdjElem& e, const Vec2& ua, const Vec2& ub, const Vec2& la, const Vec2& lb,
                            double& gI, double& gw) {
  const ElemK h = elem_k(e.c2, e.c6, e.c12, 1.0);
  const double dv = ua.x - ub.x;
  const double r0 = __builtin_fma(h.kA, dv, h.kB * (ua.y + ub.y));
  const double r1 = __builtin_fma(h.kB, dv, __builtin_fma(h.kC, ua.y, h.kD * ub.y));
  const double r3 = __builtin_fma(h.kB, dv, __builtin_fma(h.kD, ua.y, h.kC * ub.y));
  gI = __builtin_fma(e.gV - la.x + lb.x, r0, __builtin_fma(e.gM - la.y, r1, -lb.y * r3));
  const double hl = 0.5 * e.L, ql = e.L * e.L * (1.0 / 12.0);
  gw = __builtin_fma(la.x + lb.x - e.gV, hl, (la.y - lb.y - e.gM) * ql);
}

// Acc supplies the lane's inputs by LOCAL index:
//   elem(i) -> AdjElem        element i in [0, M) (padding included, see adj_elem_pad)
//   gn(i)   -> Vec2           nodal cotangent (gv, gt) at local node i in [0, M); zero on padding nodes
//   u(i)    -> Vec2           the forward's (v, theta) at local node i in [0, M]; zero on padding nodes
//   fixbits(), fence()        as in beam_math.hpp
// Phase A with the adjoint load: statement for statement seg_condense, loads from adj_elem_load + gn.
template <int M, bool RZ, class Acc>
BEAM_HD void seg_condense_adj(SegState<M>& s, const Acc& acc, int& bad) {
  const unsigned long long fb = acc.fixbits();
  {
    const AdjElem e = acc.elem(0);
    const ElemK k = elem_k(e.c2, e.c6, e.c12, e.Ie);
    const ElemLoad q = adj_elem_load(k, e.gV, e.gM);
    const Vec2 gn = acc.gn(0);
    s.SLL = Sym2{k.kA, k.kB, k.kC};
    s.SLc = Mat2{-k.kA, k.kB, -k.kB, k.kD};
    s.Scc = Sym2{k.kA, -k.kB, k.kC};
    s.gL = Vec2{q.a.x + gn.x, q.a.y + gn.y};
    s.gc = q.b;
  }
#pragma unroll
  for (int i = 1; i < M; ++i) {
    acc.fence();
    const Flags<RZ> c = node_flags<RZ>(fb, i);
    const AdjElem e = acc.elem(i);
    const ElemK k = elem_k(e.c2, e.c6, e.c12, e.Ie);
    const ElemLoad q = adj_elem_load(k, e.gV, e.gM);
    const Vec2 gn = acc.gn(i);
    const Sym2 G = proj_inv(Sym2{s.Scc.a + k.kA, s.Scc.b + k.kB, s.Scc.c + k.kC}, c, bad);
    const Vec2 gi{s.gc.x + q.a.x + gn.x, s.gc.y + q.a.y + gn.y};
    const Mat2 Kr{-k.kA, k.kB, -k.kB, k.kD};
    s.Ginv[i] = G;
    const Mat2 Pm = mul(s.SLc, G);
    const Mat2 Qm = mulT(Kr, G);
    s.SLL = sub_mulT(s.SLL, Pm, s.SLc);
    s.gL = sub_mul(s.gL, Pm, gi);
    s.SLc = neg_mul(Pm, Kr);
    s.Scc = sub_mul(Sym2{k.kA, -k.kB, k.kC}, Qm, Kr);
    s.gc = sub_mul(q.b, Qm, gi);
  }
}

// Phase C with the adjoint load: seg_solve's sweep and back substitution for lambda, then the contractions instead of the
// force recovery.  lL, lR: lambda at the lane's left and right boundary nodes (from the interface solve).
// Out receives: elem(i, gI, gwy) for i in [0, M), node(i, lambda) for local node i in [0, M).
template <int M, bool RZ, class Acc, class Out>
BEAM_HD void seg_solve_adj(const SegState<M>& s, const Acc& acc, const Vec2& lL, const Vec2& lR, Out& out) {
  (void)acc.fixbits();
  Vec2 h[M];
  {
    const AdjElem e0 = acc.elem(0);
    const ElemK k0 = elem_k(e0.c2, e0.c6, e0.c12, e0.Ie);
    Vec2 carry = sub_mulT(adj_elem_load(k0, e0.gV, e0.gM).b, Mat2{-k0.kA, k0.kB, -k0.kB, k0.kD}, lL);
#pragma unroll
    for (int i = 1; i < M; ++i) {
      acc.fence();
      const AdjElem e = acc.elem(i);
      const ElemK k = elem_k(e.c2, e.c6, e.c12, e.Ie);
      const ElemLoad q = adj_elem_load(k, e.gV, e.gM);
      const Vec2 gn = acc.gn(i);
      h[i] = Vec2{carry.x + q.a.x + gn.x, carry.y + q.a.y + gn.y};
      if (i + 1 < M) {
        const Vec2 y = mul(s.Ginv[i], h[i]);
        carry = sub_mulT(q.b, Mat2{-k.kA, k.kB, -k.kB, k.kD}, y);
      }
    }
  }
  Vec2 ln = lR;          // lambda at local node i+1
  Vec2 un = acc.u(M);    // u at local node i+1
#pragma unroll
  for (int i = M - 1; i >= 0; --i) {
    acc.fence();
    const AdjElem e = acc.elem(i);
    const Vec2 ui = acc.u(i);
    Vec2 li;
    if (i > 0) {
      const ElemK k = elem_k(e.c2, e.c6, e.c12, e.Ie);
      li = mul(s.Ginv[i], sub_mul(h[i], Mat2{-k.kA, k.kB, -k.kB, k.kD}, ln));
    } else {
      li = lL;
    }
    double gI, gw;
    adj_elem_grads(e, ui, un, li, ln, gI, gw);
    out.elem(i, gI, gw);
    out.node(i, li);
    ln = li;
    un = ui;
  }
}

}  // namespace opsamd
