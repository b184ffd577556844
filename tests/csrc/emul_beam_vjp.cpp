// Lane-level CPU emulation of openpystruct_amd/csrc/beam_vjp.hip -- TEST CODE ONLY.
//
// Runs the kernel's per-lane adjoint arithmetic (beam_adjoint.hpp over beam_math.hpp, shared verbatim) with the
// cross-lane traffic (interface hand-over, cyclic reduction, right-boundary fetch) replaced by array reads, so that the
// VJP can be checked against a dense reference on a machine without a GPU.  Nothing under openpystruct_amd/ loads it.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../openpystruct_amd/csrc/beam_adjoint.hpp"

using namespace opsamd;

namespace {
// one lane's view: pointers already offset to the lane's first element / node; nE, nN real ones from there on
struct HostAdjAcc {
  const double *x, *E, *I, *gV, *gM, *gv, *gt, *v, *th;
  bool E_pe;
  int nE, nN;
  unsigned long long bits;
  AdjElem elem(int i) const {
    if (i >= nE) return adj_elem_pad(i > nE);
    return adj_elem_real(x[i + 1] - x[i], E_pe ? E[i] : E[0], I[i], gV ? gV[i] : 0.0, gM ? gM[i] : 0.0);
  }
  Vec2 gn(int i) const { return i < nN ? Vec2{gv ? gv[i] : 0.0, gt ? gt[i] : 0.0} : Vec2{0.0, 0.0}; }
  Vec2 u(int i) const { return i < nN ? Vec2{v[i], th[i]} : Vec2{0.0, 0.0}; }
  unsigned long long fixbits() const { return bits; }
  void fence() const {}
};
struct HostAdjOut {
  double *gI, *gw, *gF;
  void elem(int i, double a, double b) { gI[i] = a; gw[i] = b; }
  void node(int i, const Vec2& l) { gF[i] = l.x; }
};

template <int P, int M>
int vjp_one(int Ne, const double* x, const double* E, bool E_pe, const double* I, const uint8_t* fix, const double* v,
            const double* th, const double* gv, const double* gt, const double* gV, const double* gM, double* gI,
            double* gFy, double* gwy) {
  constexpr int PM = P * M;
  const int N = Ne + 1;
  std::vector<double> oI(PM), ow(PM), oF(PM);
  std::vector<SegState<M>> st(P);
  std::vector<HostAdjAcc> acc(P);
  int bad = 0;
  for (int j = 0; j < P; ++j) {
    const int e0 = j * M;
    acc[j] = HostAdjAcc{x + e0, E_pe ? E + e0 : E, I + e0, gV ? gV + e0 : nullptr, gM ? gM + e0 : nullptr,
                        gv ? gv + e0 : nullptr, gt ? gt + e0 : nullptr, v + e0, th + e0, E_pe, Ne - e0, N - e0, 0ull};
    for (int i = 0; i <= M; ++i)
      if (e0 + i < N) acc[j].bits |= (unsigned long long)(fix[e0 + i] & 3) << (2 * i);
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
    const int e0 = j * M;
    HostAdjOut out{&oI[e0], &ow[e0], &oF[e0]};
    seg_solve_adj<M, true>(st[j], acc[j], lam[j], j + 1 < P ? lam[j + 1] : z2, out);
  }
  for (int e = 0; e < Ne; ++e) { gI[e] = bad ? NAN : oI[e]; gwy[e] = bad ? NAN : ow[e]; }
  for (int n = 0; n < N; ++n) gFy[n] = bad ? NAN : oF[n];
  return bad;
}
}  // namespace

// Arguments as ops_beam_solve_vjp_f64 (v, theta, gv, gt, gV, gM, gI, gFy, gwy dense; cotangents may be NULL), plus (P, M).
extern "C" int emul_beam_solve_vjp_f64(int P, int M, int B, int Ne, const double* x, long x_bs, const double* E, long E_bs,
                                       const double* I, long I_bs, const uint8_t* fix, long fix_bs, const double* v,
                                       const double* theta, const double* gv, const double* gt, const double* gV,
                                       const double* gM, double* gI, double* gFy, double* gwy, int32_t* status) {
  const int N = Ne + 1;
  if (P * M < N) return -1;
  for (int b = 0; b < B; ++b) {
    const long bn = (long)b * N, be = (long)b * Ne;
    int r = -2;
#define CASE(p_, m_)                                                                                                  \
  if (P == p_ && M == m_)                                                                                             \
    r = vjp_one<p_, m_>(Ne, x + b * x_bs, E + b * E_bs, E_bs != 0, I + b * I_bs, fix + b * fix_bs, v + bn, theta + bn, \
                        gv ? gv + bn : nullptr, gt ? gt + bn : nullptr, gV ? gV + be : nullptr, gM ? gM + be : nullptr, \
                        gI + be, gFy + bn, gwy + be);
    CASE(16, 7) CASE(32, 4) CASE(64, 4) CASE(64, 8) CASE(64, 16)
#undef CASE
    if (r == -2) return -2;
    if (status) status[b] = r;
  }
  return 0;
}
