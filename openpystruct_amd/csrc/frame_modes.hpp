// Arithmetic of the natural frequencies and mode shapes on the kept factorisation: plain C++ that compiles for
// the device (csrc/frame_loads.hip) and with g++ for the host (tests/test_frame_modes_host.py builds a stand-alone program from
// this file).  The generalised eigenproblem is K(I) phi = lambda M phi on the free DOFs; one iteration of the subspace (inverse)
// iteration on P vectors is X = K^-1 R (the re-solve of csrc/frame_resolve.hpp), MX = M X (fm_node_mass) and the Ritz step below.
//
//   mass      y[n,:] = nodal_mass[n,:] * x[n,:] + sum over the element ends at node n of (M_e x_e)[end of e at n], the node walk
//             of frame_adjoint.hpp; M_e the rotated consistent 6 x 6 matrix of a mass per unit length, or mL/2 on the four
//             translations (lumped).  M does not depend on I.
//   Ritz      Kr = sym(X^T R), Mr = X^T MX (upper triangle), Mr = G G^T, A = G^-1 Kr G^-T, cyclic Jacobi on A, Ritz values
//             ascending, Z = G^-T V, Q = X Z, R <- MX Z.  The dot products are per-lane strided partial sums (fm_ritz_partials)
//             that the caller adds over the 64 lanes by a fixed butterfly; the small dense part (fm_ritz_small) is the same
//             arithmetic on every lane; fm_ritz_update writes the lane's entries of Q and R.
//   gradient  dlambda_j/dI_e = phi_j,e . (K_b,e phi_j,e) for M-normalised phi (M does not depend on I: no adjoint solve).
//   floor     the natural-frequency floor of design sizing: the hinge of the m lowest eigenvalues against a floor and
//             its gradient, the gradient above with coefficients formed from lambda (fm_elem_floor).
#pragma once
#include <math.h>
#include <stdint.h>

#include "frame_adjoint.hpp"

namespace opsamd {

constexpr int FM_MAX_VECTORS = 8;
constexpr int FM_LANES = 64;
constexpr int FM_MAX_SWEEPS = 16;

// y = M_e x for the six global end DOFs of an element of length L, direction (c, s) and mass per unit length mbar
FA_HD void fm_elem_mass(double L, double c, double s, double mbar, int consistent, const double x[6], double y[6]) {
  if (!consistent) {
    const double h = mbar * L / 2;
    y[0] = h * x[0]; y[1] = h * x[1]; y[2] = 0.0;
    y[3] = h * x[3]; y[4] = h * x[4]; y[5] = 0.0;
    return;
  }
  const double u0 = c * x[0] + s * x[1], u1 = -s * x[0] + c * x[1], u2 = x[2];
  const double u3 = c * x[3] + s * x[4], u4 = -s * x[3] + c * x[4], u5 = x[5];
  const double m = mbar * L / 420, L2 = L * L;
  const double y0 = m * (140 * u0 + 70 * u3);
  const double y1 = m * (156 * u1 + 22 * L * u2 + 54 * u4 - 13 * L * u5);
  const double y2 = m * (22 * L * u1 + 4 * L2 * u2 + 13 * L * u4 - 3 * L2 * u5);
  const double y3 = m * (70 * u0 + 140 * u3);
  const double y4 = m * (54 * u1 + 13 * L * u2 + 156 * u4 - 22 * L * u5);
  const double y5 = m * (-13 * L * u1 - 3 * L2 * u2 - 22 * L * u4 + 4 * L2 * u5);
  y[0] = c * y0 - s * y1; y[1] = s * y0 + c * y1; y[2] = y2;
  y[3] = c * y3 - s * y4; y[4] = s * y3 + c * y4; y[5] = y5;
}

// the three components at node n of M x[row]; x [R,Nn,3], frame = the frame of the row (nodal_bstride 0: one [Nn,3] nodal mass for
// the batch, else 3 Nn; nodal_mass NULL: none): the node's own term first, then its incident element ends in table order
FA_HD void fm_node_mass(int n_nodes, const double* elem_geo, const int32_t* conn, const int32_t* node_elem_ptr,
                        const int32_t* node_elem_idx, const double* elem_mass, int consistent, const double* nodal_mass,
                        long nodal_bstride, const double* x, long row, long frame, int n, double y[3]) {
  const double* xn = x + (row * n_nodes + n) * 3;
  const double* nm = nodal_mass ? nodal_mass + frame * nodal_bstride + 3 * (long)n : nullptr;
  for (int k = 0; k < 3; ++k) y[k] = nm ? nm[k] * xn[k] : 0.0;
  fa_walk(node_elem_ptr, node_elem_idx, n, y, [&](int e, double v[6]) {
    double xe[6];
    fa_gather(n_nodes, conn, x, row, e, xe);
    fm_elem_mass(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], elem_mass[e], consistent, xe, v);
  });
}

// gI of element e of frame b: sum over the m requested modes, in mode order, of g_lambda[b,j] phi_j,e . (K_b,e phi_j,e);
// phi [B,p,Nn,3], g_lambda [B,m]
FA_HD double fm_elem_grad(int m, int p, int n_nodes, const double* elem_geo, const double* elem_E, const int32_t* conn,
                          const double* phi, const double* g_lambda, long b, int e) {
  double acc = 0.0;
  for (int j = 0; j < m; ++j) {
    double u[6], y[6];
    fa_gather(n_nodes, conn, phi, b * p + j, e, u);
    fa_apply_k(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], 0.0, elem_E[e], u, y);
    double q = 0.0;
    for (int k = 0; k < 6; ++k) q += u[k] * y[k];
    acc += g_lambda[b * m + j] * q;
  }
  return acc;
}

// ---- the natural-frequency floor of design sizing ----
// h = max(0, 1 - lambda / floor); a NaN lambda stays NaN
FA_HD double fm_floor_hinge(double lam, double floor) {
  const double h = 1.0 - lam / floor;
  return h < 0.0 ? 0.0 : h;
}

// dP_f/dI of element e of design b, P_f = alpha sum over j < m of h_j^2: the sum over the m tracked modes, in mode order, of
// (-2 alpha h_j / floor) phi_j,e . (K_b,e phi_j,e), the coefficients formed here from lambda [B,p]; phi [B,p,Nn,3].  *penalty: P_f.
// With every hinge off the sum is +0.0 (a sum of zeros of either sign that starts from +0.0) and P_f is 0.0
FA_HD double fm_elem_floor(int m, int p, int n_nodes, const double* elem_geo, const double* elem_E, const int32_t* conn,
                           const double* phi, const double* lambda, double floor, double alpha, long b, int e, double* penalty) {
  double acc = 0.0, pen = 0.0;
  for (int j = 0; j < m; ++j) {
    const double h = fm_floor_hinge(lambda[b * p + j], floor);
    pen += h * h;
    const double coef = -2.0 * alpha * h / floor;
    double u[6], y[6];
    fa_gather(n_nodes, conn, phi, b * p + j, e, u);
    fa_apply_k(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], 0.0, elem_E[e], u, y);
    double q = 0.0;
    for (int k = 0; k < 6; ++k) q += u[k] * y[k];
    acc += coef * q;
  }
  *penalty = alpha * pen;
  return acc;
}

// ---- the Ritz step of one frame on P vectors of n = 3 Nn entries each (x, mx, r: that frame's [P,n]) ----

// number of partial sums: P * P of X^T R, P (P + 1) / 2 of the upper triangle of X^T MX
template <int P>
struct FmRitz {
  static constexpr int NK = P * P, NM = P * (P + 1) / 2, NACC = NK + NM;
};

// the lane's partial sums over its entries lane, lane + 64, ...: acc[i P + j] = x_i . r_j, then the rows of the upper triangle
// of x_i . mx_j (j >= i)
template <int P>
FA_HD void fm_ritz_partials(long n, const double* x, const double* mx, const double* r, int lane, double acc[FmRitz<P>::NACC]) {
  for (int k = 0; k < FmRitz<P>::NACC; ++k) acc[k] = 0.0;
  for (long t = lane; t < n; t += FM_LANES) {
    double xv[P], mv[P], rv[P];
    for (int i = 0; i < P; ++i) {
      xv[i] = x[i * n + t];
      mv[i] = mx[i * n + t];
      rv[i] = r[i * n + t];
    }
    int k = FmRitz<P>::NK;
    for (int i = 0; i < P; ++i) {
      for (int j = 0; j < P; ++j) acc[i * P + j] += xv[i] * rv[j];
      for (int j = i; j < P; ++j) acc[k++] += xv[i] * mv[j];
    }
  }
}

// The small dense part, from the sums over all lanes: Z [P,P] (row i, column j: the weight of x_i in q_j), lam ascending,
// change = |lam - lam_prev| / lam (lam_prev = +inf: +inf).  Returns 0, or 2 when Mr is not positive definite (nothing is
// written then).  *sweeps: the Jacobi sweeps that ran (FM_MAX_SWEEPS: the cap ended the loop).
template <int P>
FA_HD int fm_ritz_small(const double acc[FmRitz<P>::NACC], const double lam_prev[P], double Z[P * P], double lam[P],
                        double change[P], int* sweeps) {
  double A[P * P], G[P * P], V[P * P];
  // Mr (upper triangle mirrored) = G G^T, G lower
  {
    int k = FmRitz<P>::NK;
    for (int i = 0; i < P; ++i)
      for (int j = i; j < P; ++j) G[j * P + i] = acc[k++];      // the lower triangle holds Mr
  }
  for (int j = 0; j < P; ++j) {
    double d = G[j * P + j];
    for (int k = 0; k < j; ++k) d -= G[j * P + k] * G[j * P + k];
    if (!(d > 0.0)) return 2;
    d = sqrt(d);
    G[j * P + j] = d;
    for (int i = j + 1; i < P; ++i) {
      double v = G[i * P + j];
      for (int k = 0; k < j; ++k) v -= G[i * P + k] * G[j * P + k];
      G[i * P + j] = v / d;
    }
  }
  // A = G^-1 sym(Kr) G^-T: the rows by forward substitution, then the columns
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < P; ++j) A[i * P + j] = (acc[i * P + j] + acc[j * P + i]) / 2;
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
  // cyclic Jacobi in row-cyclic order, until the off-diagonal sum of squares is at most (2^-52 trace)^2
  int sw = 0;
  for (; sw < FM_MAX_SWEEPS; ++sw) {
    double off = 0.0, tr = 0.0;
    for (int i = 0; i < P; ++i) {
      tr += A[i * P + i];
      for (int j = 0; j < P; ++j)
        if (j != i) off += A[i * P + j] * A[i * P + j];
    }
    const double lim = 2.220446049250313e-16 * tr;
    if (off <= lim * lim) break;
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
  for (int i = 0; i < P; ++i) lam[i] = A[i * P + i];
  // ascending, by exchanges of neighbours at fixed places (a stable order of equal values)
  for (int pass = 0; pass < P - 1; ++pass)
    for (int j = 0; j + 1 < P - pass; ++j)
      if (lam[j] > lam[j + 1]) {
        const double l = lam[j]; lam[j] = lam[j + 1]; lam[j + 1] = l;
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
  for (int j = 0; j < P; ++j) change[j] = fabs(lam[j] - lam_prev[j]) / lam[j];
  return 0;
}

// the lane's entries of q_j = sum_i x_i Z[i,j] and r_j = sum_i mx_i Z[i,j]
template <int P>
FA_HD void fm_ritz_update(long n, const double* x, const double* mx, const double* Z, int lane, double* q, double* r) {
  for (long t = lane; t < n; t += FM_LANES) {
    double xv[P], mv[P];
    for (int i = 0; i < P; ++i) {
      xv[i] = x[i * n + t];
      mv[i] = mx[i * n + t];
    }
    for (int j = 0; j < P; ++j) {
      double a = 0.0, b = 0.0;
      for (int i = 0; i < P; ++i) {
        a += xv[i] * Z[i * P + j];
        b += mv[i] * Z[i * P + j];
      }
      q[j * n + t] = a;
      r[j * n + t] = b;
    }
  }
}

}  // namespace opsamd
