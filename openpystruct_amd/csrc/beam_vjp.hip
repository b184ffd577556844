// Vector-Jacobian product of the batched beam solve for gfx950 (MI355X): the adjoint solve K lambda = g_u and the
// per-element contractions gI, gFy, gwy fused in one kernel.  C ABI: include/openpystruct_amd.h
// (ops_beam_solve_vjp_f64).  Arithmetic: beam_adjoint.hpp over beam_math.hpp.  Design: DESIGN.md §9e.
//
// Mapping as in beam_solve.hip: one 64-lane wavefront per workgroup, P lanes per beam, M elements per lane, the
// interface system by cyclic reduction over the P lanes (DPP / ds_bpermute exchange, beam_io.hpp).  The factorisation
// is recomputed from x, E, I and fix rather than stored by the forward (three doubles per node the forward never
// writes).  Unlike the forward, inputs are read straight from global memory by each lane (no LDS staging and no element
// table): a lane's M consecutive elements are one short contiguous run, the wave's runs together cover its beams' rows,
// and the fences between elements bound the registers that in-flight loads hold.  Outputs are stored the same way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openpystruct_amd.h"
#include "beam_adjoint.hpp"
#include "beam_io.hpp"
#include "library.hpp"

namespace opsamd {

struct VjpParams {
  int B, Ne;
  const double* x;  long x_bs;
  const double* E;  long E_bs;
  const double* I;  long I_bs;
  const uint8_t* fix; long fix_bs;
  const double* v; const double* theta;    // [B,N] dense
  const double* gv; const double* gt;      // [B,N] dense or NULL
  const double* gV; const double* gM;      // [B,Ne] dense or NULL
  double* gI; double* gFy; double* gwy;    // [B,Ne], [B,N], [B,Ne]; gFy / gwy may be NULL
  int32_t* status;
};

// one lane's view (beam_adjoint.hpp "Acc"): pointers offset to the lane's first element / node of its beam;
// nE / nN: real elements / nodes from there on (may be <= 0 for a lane that owns padding only)
struct VjpAcc {
  const double *x, *E, *I, *gV, *gM, *gv, *gt, *v, *th;
  bool E_pe;
  int nE, nN;
  unsigned long long bits;
  __device__ __forceinline__ AdjElem elem(int i) const {
    if (i >= nE) return adj_elem_pad(i > nE);
    return adj_elem_real(x[i + 1] - x[i], E_pe ? E[i] : E[0], I[i], gV ? gV[i] : 0.0, gM ? gM[i] : 0.0);
  }
  __device__ __forceinline__ Vec2 gn(int i) const {
    return i < nN ? Vec2{gv ? gv[i] : 0.0, gt ? gt[i] : 0.0} : Vec2{0.0, 0.0};
  }
  __device__ __forceinline__ Vec2 u(int i) const { return i < nN ? Vec2{v[i], th[i]} : Vec2{0.0, 0.0}; }
  __device__ __forceinline__ unsigned long long fixbits() const { return bits; }
  __device__ __forceinline__ void fence() const { __asm__ volatile("" ::: "memory"); }
};

// results of a lane, stored as they come out of the back substitution; `store` false for the lanes of a beam beyond B
struct VjpOut {
  double *gI, *gw, *gF;
  int nE, nN;
  bool store, nan;
  __device__ __forceinline__ void elem(int i, double a, double b) {
    if (store && i < nE) {
      gI[i] = nan ? __builtin_nan("") : a;
      if (gw) gw[i] = nan ? __builtin_nan("") : b;
    }
  }
  __device__ __forceinline__ void node(int i, const Vec2& l) {
    if (store && gF && i < nN) gF[i] = nan ? __builtin_nan("") : l.x;
  }
};

template <int P, int M>
__global__ __launch_bounds__(64) void beam_vjp_kernel(const VjpParams p) {
  constexpr int BPW = 64 / P;
  const int lane = threadIdx.x, g = lane / P, j = lane - g * P, e0 = j * M;
  const int Ne = p.Ne, N = Ne + 1;
  const long braw = (long)blockIdx.x * BPW + g;
  const bool live = braw < p.B;
  const long b = live ? braw : (long)p.B - 1;   // lanes of a beam beyond B repeat beam B-1's arithmetic, store nothing
  const long bn = b * N + e0, be = b * Ne + e0;

  VjpAcc acc;
  acc.x = p.x + b * p.x_bs + e0;
  acc.E_pe = p.E_bs != 0;
  acc.E = acc.E_pe ? p.E + b * p.E_bs + e0 : p.E;
  acc.I = p.I + b * p.I_bs + e0;
  acc.gV = p.gV ? p.gV + be : nullptr;
  acc.gM = p.gM ? p.gM + be : nullptr;
  acc.gv = p.gv ? p.gv + bn : nullptr;
  acc.gt = p.gt ? p.gt + bn : nullptr;
  acc.v = p.v + bn;
  acc.th = p.theta + bn;
  acc.nE = Ne - e0;
  acc.nN = N - e0;
  {
    const uint8_t* fb = p.fix + b * p.fix_bs + e0;
    unsigned long long bits = 0;
#pragma unroll
    for (int i = 0; i <= M; ++i)   // nodes at or beyond N are padding: free
      if (i < acc.nN) bits |= (unsigned long long)(fb[i] & 3) << (2 * i);
    acc.bits = bits;
  }

  // the forward's phases A and B (solve_lanes in beam_solve.hip) with the adjoint load; RZ = true always (the
  // fixed-rotation-free fast path only skips multiplications by 1.0, the results are the same)
  using X = Xch<P>;
  int bad = 0;
  SegState<M> st;
  seg_condense_adj<M, true>(st, acc, bad);
  IfaceRow row;
  {
    const Mat2 cup = masked_cup<M, true>(st, acc.bits);
    const Sym2 pc = X::template from_minus<1>(st.Scc, lane, j);
    const Vec2 pg = X::template from_minus<1>(st.gc, lane, j);
    const Mat2 pb = X::template from_minus<1>(cup, lane, j);
    row = make_row<M, true>(st, cup, pc, pg, pb, acc.bits);
  }
  cr_forward<P, 1>(row, lane, j, bad);
  const Sym2 G = inv_spd(row.D, bad);
  Vec2 lL = mul(G, row.f);
  if (j != 0) lL = Vec2{0.0, 0.0};
  cr_backward<P, P / 2>(row, G, lL, lane, j);
  const Vec2 lR = X::template from_plus<1>(lL, lane, j);

  // a beam is bad if any of its P lanes met a non-positive pivot: NaN gradients, status 1
  const unsigned long long bal = __ballot(bad != 0);
  const unsigned long long grp = (P == 64) ? ~0ull : (((1ull << (P % 64)) - 1ull) << (g * P));
  const bool gbad = (bal & grp) != 0ull;
  if (j == 0 && live && p.status) p.status[b] = gbad ? 1 : 0;

  VjpOut out{p.gI + be, p.gwy ? p.gwy + be : nullptr, p.gFy ? p.gFy + bn : nullptr, acc.nE, acc.nN, live, gbad};
  seg_solve_adj<M, true>(st, acc, lL, lR, out);
}

// The VJP's tilings: a tiling serves Ne with Ne + 1 <= P * M; the first one that serves is used.  16 lanes per beam covers
// the reference's beams (Ne <= 111) with four beams per wave; the 64-lane ones reach the forward's largest Ne (1023).
struct VjpTiling { int P, M; };
static const VjpTiling kVjpTilings[] = {{16, 7}, {32, 4}, {64, 4}, {64, 8}, {64, 16}};

template <int P, int M>
static hipError_t launch_vjp(const VjpParams& p, hipStream_t stream) {
  constexpr int BPW = 64 / P;
  const unsigned grid = (unsigned)((p.B + BPW - 1) / BPW);
  hipLaunchKernelGGL((beam_vjp_kernel<P, M>), dim3(grid), dim3(64), 0, stream, p);
  return hipGetLastError();
}

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_beam_solve_vjp_f64(int B, int Ne, const double* x, long x_bstride, const double* E, long E_bstride,
                                      const double* I, long I_bstride, const uint8_t* fix, long fix_bstride,
                                      const double* wy, long wy_bstride, const double* v, const double* theta,
                                      const double* gv, const double* gt, const double* gV, const double* gM, double* gI,
                                      double* gFy, double* gwy, int32_t* status, void* stream) {
  if (B < 0 || Ne < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!x || !E || !I || !fix || !wy || !v || !theta || !gI) return OPS_AMD_ERR_INVALID_ARG;
  if (I_bstride < Ne || (x_bstride != 0 && x_bstride < Ne + 1) || (fix_bstride != 0 && fix_bstride < Ne + 1) ||
      (E_bstride != 0 && E_bstride < Ne) || (wy_bstride != 0 && wy_bstride < Ne))
    return OPS_AMD_ERR_INVALID_ARG;
  if (Ne > ops_amd_max_elements()) return OPS_AMD_ERR_UNSUPPORTED;
  const VjpTiling* t = nullptr;
  for (const VjpTiling& c : kVjpTilings)
    if (c.P * c.M >= Ne + 1) { t = &c; break; }
  if (!t) return OPS_AMD_ERR_UNSUPPORTED;
  // wy does not enter the arithmetic (the gradient is linear in the loads and u already holds them); it is validated
  // like the forward's so that one argument list serves both calls
  const VjpParams p{B, Ne, x, x_bstride, E, E_bstride, I, I_bstride, fix, fix_bstride, v, theta, gv, gt, gV, gM, gI, gFy, gwy, status};
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSuccess;
  if (t->P == 16 && t->M == 7) err = launch_vjp<16, 7>(p, s);
  else if (t->P == 32 && t->M == 4) err = launch_vjp<32, 4>(p, s);
  else if (t->P == 64 && t->M == 4) err = launch_vjp<64, 4>(p, s);
  else if (t->P == 64 && t->M == 8) err = launch_vjp<64, 8>(p, s);
  else err = launch_vjp<64, 16>(p, s);
  return launch_status(err);
}
