// Lane-level CPU emulation of the gradient kernel of openpystruct_amd/csrc/sizing_grad.hip -- TEST CODE ONLY.
//
// Runs the kernel's per-lane arithmetic (sizing_grad_math.hpp over beam_adjoint.hpp, shared verbatim) with the cross-lane
// traffic (interface hand-over, cyclic reduction, right-boundary fetch, the sum of the deflection term over a beam's lanes)
// replaced by array reads, as tests/csrc/emul_beam_vjp.cpp does for the VJP.  Nothing under openpystruct_amd/ loads it.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../openpystruct_amd/csrc/sizing_grad_math.hpp"

using namespace opsamd;

namespace {
// one lane's view: pointers already offset to the lane's first element / node; nE, nN real ones from there on
template <int M>
struct HostGradAcc {
  const double *x, *E, *I, *V, *v, *th;
  const SizingObj* o;
  bool E_pe;
  int nE, nN;
  unsigned long long bits;
  SizingQuot q[M];
  AdjElem elem(int i) const {
    if (i >= nE) return adj_elem_pad(i > nE);
    return adj_elem_real(x[i + 1] - x[i], E_pe ? E[i] : E[0], I[i], sizing_gV(*o, q[i]), sizing_gM(*o, q[i]));
  }
  Vec2 gn(int i) const { return i < nN ? Vec2{sizing_gv(*o, v[i]), 0.0} : Vec2{0.0, 0.0}; }
  Vec2 u(int i) const { return i < nN ? Vec2{v[i], th[i]} : Vec2{0.0, 0.0}; }
  unsigned long long fixbits() const { return bits; }
  void fence() const {}
};
template <int M>
struct HostGradOut {
  const HostGradAcc<M>& acc;
  double* grad;
  double defl;
  void elem(int i, double gI, double) {
    if (i < acc.nE) grad[i] = sizing_explicit(*acc.o, acc.I[i], acc.V[i], acc.q[i]) + gI;
  }
  void node(int i, const Vec2&) {
    if (i < acc.nN) defl += sizing_defl(*acc.o, acc.v[i]);
  }
};

template <int P, int M>
int grad_one(int Ne, const double* x, const double* E, bool E_pe, const double* I, const uint8_t* fix, const double* v,
             const double* th, const double* V, const double* Mm, const SizingObj& o, double* grad, double* extra) {
  constexpr int PM = P * M;
  const int N = Ne + 1;
  std::vector<double> og(PM, 0.0), od(P, 0.0);
  std::vector<SegState<M>> st(P);
  std::vector<HostGradAcc<M>> acc(P);
  int bad = 0;
  for (int j = 0; j < P; ++j) {
    const int e0 = j * M;
    acc[j] = HostGradAcc<M>{x + e0, E_pe ? E + e0 : E, I + e0, V + e0, v + e0, th + e0, &o, E_pe, Ne - e0, N - e0, 0ull, {}};
    for (int i = 0; i <= M; ++i)
      if (e0 + i < N) acc[j].bits |= (unsigned long long)(fix[e0 + i] & 3) << (2 * i);
    for (int i = 0; i < M; ++i)
      acc[j].q[i] = i < acc[j].nE ? sizing_quot(o, I[e0 + i], V[e0 + i], Mm[e0 + i]) : SizingQuot{0.0, 0.0};
    seg_condense_adj<M, true>(st[j], acc[j], bad);
  }
  std::vector<IfaceRow> row(P), nxt(P);
  std::vector<Mat2> cup(P);
  const Sym2 z3{0, 0, 0}; const Mat2 z4{0, 0, 0, 0}; const Vec2 z2{0, 0};
  for (int j = 0; j < P; ++j) cup[j] = masked_cup<M, true>(st[j], acc[j].bits);
  for (int j = 0; j < P; ++j)
    row[j] = make_row<M, true>(st[j], cup[j], j ? st[j - 1].Scc : z3, j ? st[j - 1].gc : z2, j ? cup[j - 1] : z4, acc[j].bits);
  for (int s = 1; s < P; s *= 2) {
    std::vector<Sym2> G(P);
    for (int j = 0; j < P; ++j) G[j] = inv_spd(row[j].D, bad);
    nxt = row;
    for (int j = 0; j < P; ++j) {
      if (!cr_active(j, s)) continue;
      const bool okm = j >= s, okp = j + s < P;
      if (2 * s < P)
        cr_eliminate<false>(nxt[j], okm ? G[j - s] : z3, okm ? row[j - s].Alow : z4, okm ? row[j - s].f : z2,
                            okp ? G[j + s] : z3, okp ? row[j + s].Cup : z4, okp ? row[j + s].f : z2);
      else
        cr_eliminate<true>(nxt[j], okm ? G[j - s] : z3, z4, okm ? row[j - s].f : z2, okp ? G[j + s] : z3, z4,
                           okp ? row[j + s].f : z2);
    }
    row = nxt;
  }
  std::vector<Sym2> Gf(P);
  std::vector<Vec2> lam(P, z2);
  for (int j = 0; j < P; ++j) Gf[j] = inv_spd(row[j].D, bad);
  lam[0] = mul(Gf[0], row[0].f);
  int top = 1;
  while (2 * top < P) top *= 2;
  for (int s = top; s >= 1; s /= 2)
    for (int j = 0; j < P; ++j)
      if (cr_frozen(j, s)) lam[j] = cr_back(row[j], Gf[j], j >= s ? lam[j - s] : z2, j + s < P ? lam[j + s] : z2);
  for (int j = 0; j < P; ++j) {
    HostGradOut<M> out{acc[j], &og[j * M], 0.0};
    seg_solve_adj<M, true>(st[j], acc[j], lam[j], j + 1 < P ? lam[j + 1] : z2, out);
    od[j] = out.defl;
  }
  for (int s = P / 2; s >= 1; s /= 2)      // the kernel's butterfly
    for (int j = 0; j < s; ++j) od[j] += od[j + s];
  for (int e = 0; e < Ne; ++e) grad[e] = bad ? NAN : og[e];
  if (extra) *extra = bad ? NAN : od[0];
  return bad;
}
}  // namespace

// Arguments as ops_beam_sizing_grad_f64 without wy, active and the stream, the objective as the kernel's constants
// (obj[7]: aM, aV, 2E, bend_eps, G * area_coef, aD, v_lim), plus (P, M).
extern "C" int emul_beam_sizing_grad_f64(int P, int M, int B, int Ne, const double* x, long x_bs, const double* E, long E_bs,
                                         const double* I, long I_bs, const uint8_t* fix, long fix_bs, const double* v,
                                         const double* theta, const double* V, const double* Mm, const double* obj,
                                         double* grad, double* loss_extra, int32_t* status) {
  const int N = Ne + 1;
  if (P * M < N) return -1;
  const SizingObj o{obj[0], obj[1], obj[2], obj[3], obj[4], obj[5], obj[6]};
  for (int b = 0; b < B; ++b) {
    const long bn = (long)b * N, be = (long)b * Ne;
    int r = -2;
#define CASE(p_, m_)                                                                                                    \
  if (P == p_ && M == m_)                                                                                               \
    r = grad_one<p_, m_>(Ne, x + b * x_bs, E + b * E_bs, E_bs != 0, I + b * I_bs, fix + b * fix_bs, v + bn, theta + bn, \
                         V + be, Mm + be, o, grad + be, loss_extra ? loss_extra + b : nullptr);
    CASE(16, 7) CASE(32, 4) CASE(64, 4) CASE(64, 8) CASE(64, 16)
#undef CASE
    if (r == -2) return -2;
    if (status) status[b] = r;
  }
  return 0;
}
