// Arithmetic of the linear buckling load factors on the kept factorisation: plain C++ that compiles for the device
// (csrc/frame_loads.hip) and with g++ for the host (tests/test_frame_buckling_host.py builds a stand-alone program from this file).
// The eigenproblem is K(I) phi = lambda S(N) phi on the free DOFs, S = -K_g(N) the negated geometric stiffness of the axial forces
// N_e (tension positive) of a reference static solution; the critical load factors are the positive lambda, ascending.  S is
// indefinite (members in tension) and can be rank deficient, so the roles of the two matrices are swapped against frame_modes.hpp:
// one iteration on P vectors is X = K^-1 R (the re-solve of csrc/frame_resolve.hpp), SX = S X (fb_node_geom) and the Ritz step below.
//
//   axial     N_e = ((c f3 + s f4) - (c f0 + s f1)) / 2 from the global end forces f of the reference solve: the mean of the two ends
//   geometric y[n,:] = sum over the element ends at node n of (S_e x_e)[end of e at n], the node walk of frame_adjoint.hpp; S_e =
//             -N_e k_g,unit,e, k_g,unit the rotated consistent matrix on (v1, th1, v2, th2), or [[1, -1], [-1, 1]] / L on (v1, v2)
//   Ritz      Kr = sym(X^T R) (= X^T K X), Sr = X^T SX (upper triangle), Kr = G G^T, A = G^-1 Sr G^-T, cyclic Jacobi on A, Ritz
//             values mu DESCENDING, Z = G^-T V, Q = X Z (K-orthonormal), R <- SX Z; lambda = 1 / mu where mu > 0, else +inf.  The
//             partial sums and the update are fm_ritz_partials / fm_ritz_update of frame_modes.hpp with SX in the place of MX.
//   gradient  dlambda_j/dI_e = lambda_j phi_j,e . (K_b,e phi_j,e) + lambda_j^2 sum_e' w_j,e' dN_e'/dI_e, w_j,e = phi_j,e . (k_g,unit,e
//             phi_j,e): the first term and the cotangent of the reference solve's end forces that carries the second (fb_elem_grad).
#pragma once
#include <math.h>
#include <stdint.h>

#include "frame_modes.hpp"

namespace opsamd {

// A Cholesky pivot of Kr below this fraction of its diagonal entry counts as zero.  Kr = X^T R is a sum of terms of both signs, and
// where p exceeds the rank of S a pivot is rounding noise of either sign (measured up to 1.4e-14 of the diagonal entry): d > 0 alone
// let such frames through.  A pivot this small has lost 40 of its 52 bits; cond(Kr) up to about 1e12 is served.
constexpr double FB_MIN_PIVOT = 9.094947017729282e-13;      // 2^-40

// the axial force of an element of direction (c, s) from its six global end forces, tension positive
FA_HD double fb_axial(double c, double s, const double f[6]) { return ((c * f[3] + s * f[4]) - (c * f[0] + s * f[1])) / 2; }

// y = S_e x = -N k_g,unit x for the six global end DOFs of an element of length L and direction (c, s); the axial DOFs get nothing
FA_HD void fb_elem_geom(double L, double c, double s, double N, int consistent, const double x[6], double y[6]) {
  const double u1 = -s * x[0] + c * x[1], u4 = -s * x[3] + c * x[4];
  double y1, y2 = 0.0, y5 = 0.0;
  if (consistent) {
    const double u2 = x[2], u5 = x[5], g = -N / (30 * L), L2 = L * L;
    y1 = g * (36 * u1 + 3 * L * u2 - 36 * u4 + 3 * L * u5);
    y2 = g * (3 * L * u1 + 4 * L2 * u2 - 3 * L * u4 - L2 * u5);
    y5 = g * (3 * L * u1 - L2 * u2 - 3 * L * u4 + 4 * L2 * u5);
  } else {
    y1 = -N / L * (u1 - u4);
  }
  y[0] = -s * y1; y[1] = c * y1; y[2] = y2;
  y[3] = s * y1; y[4] = -(c * y1); y[5] = y5;
}

// the three components at node n of S x[row]; x [R,Nn,3], forces [B,Ne,6] the reference solve's end forces, frame = the frame of the
// row: the node's incident element ends in table order
FA_HD void fb_node_geom(int n_nodes, int n_elems, const double* elem_geo, const int32_t* conn, const int32_t* node_elem_ptr,
                        const int32_t* node_elem_idx, const double* forces, int consistent, const double* x, long row, long frame,
                        int n, double y[3]) {
  const double* f = forces + frame * 6 * n_elems;
  y[0] = y[1] = y[2] = 0.0;
  fa_walk(node_elem_ptr, node_elem_idx, n, y, [&](int e, double v[6]) {
    double xe[6];
    fa_gather(n_nodes, conn, x, row, e, xe);
    const double c = elem_geo[3 * e + 1], s = elem_geo[3 * e + 2];
    fb_elem_geom(elem_geo[3 * e], c, s, fb_axial(c, s, f + 6 * (long)e), consistent, xe, v);
  });
}

// Element e of frame b, summed over the m requested modes in mode order, those with a finite lambda: *direct = sum_j g_j lambda_j
// phi_j,e . (K_b,e phi_j,e) and gf[6] = (sum_j g_j lambda_j^2 w_j,e) (-c/2, -s/2, 0, c/2, s/2, 0), the cotangent of the reference
// solve's end forces.  phi [B,p,Nn,3] K-normalised, lambda and g_lambda [B,m]
FA_HD void fb_elem_grad(int m, int p, int n_nodes, const double* elem_geo, const double* elem_E, const int32_t* conn, int consistent,
                        const double* phi, const double* lambda, const double* g_lambda, long b, int e, double* direct, double gf[6]) {
  const double L = elem_geo[3 * e], c = elem_geo[3 * e + 1], s = elem_geo[3 * e + 2];
  double d = 0.0, a = 0.0;
  for (int j = 0; j < m; ++j) {
    const double l = lambda[b * m + j], g = g_lambda[b * m + j];
    if (!(fabs(l) < INFINITY)) continue;
    double u[6], y[6];
    fa_gather(n_nodes, conn, phi, b * p + j, e, u);
    fa_apply_k(L, c, s, 0.0, elem_E[e], u, y);
    double q = 0.0, w = 0.0;
    for (int k = 0; k < 6; ++k) q += u[k] * y[k];
    fb_elem_geom(L, c, s, -1.0, consistent, u, y);
    for (int k = 0; k < 6; ++k) w += u[k] * y[k];
    d += g * l * q;
    a += g * (l * l) * w;
  }
  *direct = d;
  gf[0] = -(c / 2) * a; gf[1] = -(s / 2) * a; gf[2] = 0.0;
  gf[3] = (c / 2) * a; gf[4] = (s / 2) * a; gf[5] = 0.0;
}

// The small dense part of the Ritz step, from the sums over all lanes (the layout of FmRitz<P>: P * P of x_i . r_j, then the upper
// triangle of x_i . sx_j): Z [P,P] (row i, column j: the weight of x_i in q_j), mu descending, lam = 1 / mu where mu > 0, else
// +inf, change = |mu - mu_prev| / |mu| (mu_prev = +inf: +inf).  Returns 0, or 2 when Kr is not positive definite to FB_MIN_PIVOT
// (nothing is written then).  *sweeps: the Jacobi sweeps that ran (FM_MAX_SWEEPS: the cap ended the loop).
template <int P>
FA_HD int fb_ritz_small(const double acc[FmRitz<P>::NACC], const double mu_prev[P], double Z[P * P], double mu[P], double lam[P],
                        double change[P], int* sweeps) {
  double A[P * P], G[P * P], V[P * P];
  // sym(Kr) = G G^T, G lower
  for (int i = 0; i < P; ++i)
    for (int j = 0; j <= i; ++j) G[i * P + j] = (acc[i * P + j] + acc[j * P + i]) / 2;
  for (int j = 0; j < P; ++j) {
    const double kjj = G[j * P + j];
    double d = kjj;
    for (int k = 0; k < j; ++k) d -= G[j * P + k] * G[j * P + k];
    if (!(d > FB_MIN_PIVOT * kjj)) return 2;
    d = sqrt(d);
    G[j * P + j] = d;
    for (int i = j + 1; i < P; ++i) {
      double v = G[i * P + j];
      for (int k = 0; k < j; ++k) v -= G[i * P + k] * G[j * P + k];
      G[i * P + j] = v / d;
    }
  }
  // A = G^-1 Sr G^-T, Sr the upper triangle mirrored: the rows by forward substitution, then the columns
  {
    int k = FmRitz<P>::NK;
    for (int i = 0; i < P; ++i)
      for (int j = i; j < P; ++j) A[i * P + j] = A[j * P + i] = acc[k++];
  }
  for (int j = 0; j < P; ++j)          // A <- G^-1 A, column by column
    for (int i = 0; i < P; ++i) {
      double v = A[i * P + j];
      for (int k = 0; k < i; ++k) v -= G[i * P + k] * A[k * P + j];
      A[i * P + j] = v / G[i * P + i];
    }
  for (int i = 0; i < P; ++i)          // A <- A G^-T, row by row
    for (int j = 0; j < P; ++j) {
      double v = A[i * P + j];
      for (int k = 0; k < j; ++k) v -= G[j * P + k] * A[i * P + k];
      A[i * P + j] = v / G[j * P + j];
    }
  for (int i = 0; i < P; ++i)
    for (int j = i + 1; j < P; ++j) A[i * P + j] = A[j * P + i] = (A[i * P + j] + A[j * P + i]) / 2;
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < P; ++j) V[i * P + j] = i == j ? 1.0 : 0.0;
  // cyclic Jacobi in row-cyclic order, until the off-diagonal sum of squares is at most (2^-52)^2 times the sum of all squares (the
  // trace of an indefinite A can vanish)
  int sw = 0;
  for (; sw < FM_MAX_SWEEPS; ++sw) {
    double off = 0.0, all = 0.0;
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < P; ++j) {
        const double v = A[i * P + j] * A[i * P + j];
        all += v;
        if (j != i) off += v;
      }
    if (off <= (2.220446049250313e-16 * 2.220446049250313e-16) * all) break;
    for (int a = 0; a < P; ++a)
      for (int b = a + 1; b < P; ++b) {
        const double apq = A[a * P + b];
        if (apq == 0.0) continue;
        const double theta = (A[b * P + b] - A[a * P + a]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < P; ++k) {                  // columns a, b
          const double ka = A[k * P + a], kb = A[k * P + b];
          A[k * P + a] = c * ka - s * kb;
          A[k * P + b] = s * ka + c * kb;
        }
        for (int k = 0; k < P; ++k) {                  // rows a, b
          const double ak = A[a * P + k], bk = A[b * P + k];
          A[a * P + k] = c * ak - s * bk;
          A[b * P + k] = s * ak + c * bk;
        }
        A[a * P + b] = A[b * P + a] = 0.0;
        for (int k = 0; k < P; ++k) {
          const double ka = V[k * P + a], kb = V[k * P + b];
          V[k * P + a] = c * ka - s * kb;
          V[k * P + b] = s * ka + c * kb;
        }
      }
  }
  *sweeps = sw;
  for (int i = 0; i < P; ++i) mu[i] = A[i * P + i];
  // descending, by exchanges of neighbours at fixed places (a stable order of equal values)
  for (int pass = 0; pass < P - 1; ++pass)
    for (int j = 0; j + 1 < P - pass; ++j)
      if (mu[j] < mu[j + 1]) {
        const double l = mu[j]; mu[j] = mu[j + 1]; mu[j + 1] = l;
        for (int k = 0; k < P; ++k) {
          const double v = V[k * P + j]; V[k * P + j] = V[k * P + j + 1]; V[k * P + j + 1] = v;
        }
      }
  // Z = G^-T V: back substitution, column by column
  for (int j = 0; j < P; ++j)
    for (int i = P - 1; i >= 0; --i) {
      double v = V[i * P + j];
      for (int k = i + 1; k < P; ++k) v -= G[k * P + i] * Z[k * P + j];
      Z[i * P + j] = v / G[i * P + i];
    }
  for (int j = 0; j < P; ++j) {
    lam[j] = mu[j] > 0.0 ? 1.0 / mu[j] : INFINITY;
    change[j] = fabs(mu[j] - mu_prev[j]) / fabs(mu[j]);
  }
  return 0;
}

}  // namespace opsamd
