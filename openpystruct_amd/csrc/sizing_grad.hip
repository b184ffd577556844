// Exact-gradient beam sizing for gfx950 (MI355X): dL/dI of the sizing objective with M, V and v as functions of I, in one
// launch, and the optimiser step that consumes it.  C ABI: include/openpystruct_amd_sizing_grad.h.  Arithmetic:
// sizing_grad_math.hpp over beam_adjoint.hpp.  Design: DESIGN.md §9g.
//
// The gradient kernel is beam_vjp.hip's kernel -- same mapping (one 64-lane wavefront per workgroup, P lanes per beam, M
// elements per lane, interface by cyclic reduction), same tilings, same instantiation of seg_condense_adj / seg_solve_adj --
// with another accessor and another sink: the accessor forms the cotangents gV, gM, gv of the objective from this epoch's
// forward (V, M, v) and I in registers, the sink adds the explicit part of dL/dI to the adjoint's gI before the one store.  The
// cotangents never exist in memory (a streaming cotangent kernel in front of ops_beam_solve_vjp_f64 would write and read back
// 2 Ne + N doubles per beam and epoch).  The accessor is asked for an element three times (condensation, forward sweep, back
// substitution): the two quotients that hold its divisions and square root are computed once and kept in 4 M registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openpystruct_amd_sizing_grad.h"
#include "beam_io.hpp"
#include "library.hpp"
#include "sizing_grad_math.hpp"
#include "sizing_math.hpp"

namespace opsamd {

struct GradParams {
  int B, Ne;
  const double* x;  long x_bs;
  const double* E;  long E_bs;
  const double* I;  long I_bs;
  const uint8_t* fix; long fix_bs;
  const double* v; const double* theta;    // [B,N] dense: this epoch's forward
  const double* V; const double* M;        // [B,Ne] dense
  SizingObj o;
  const uint8_t* active;                   // [B] or NULL
  double* grad; double* loss_extra;        // [B,Ne], [B] or NULL
  int32_t* status;
};

// one lane's view (beam_adjoint.hpp "Acc"), as VjpAcc of beam_vjp.hip: pointers offset to the lane's first element / node
template <int M>
struct GradAcc {
  const double *x, *E, *I, *V, *v, *th;
  const SizingObj& o;
  bool E_pe;
  int nE, nN;
  unsigned long long bits;
  SizingQuot q[M];
  __device__ __forceinline__ AdjElem elem(int i) const {
    if (i >= nE) return adj_elem_pad(i > nE);
    return adj_elem_real(x[i + 1] - x[i], E_pe ? E[i] : E[0], I[i], sizing_gV(o, q[i]), sizing_gM(o, q[i]));
  }
  __device__ __forceinline__ Vec2 gn(int i) const { return i < nN ? Vec2{sizing_gv(o, v[i]), 0.0} : Vec2{0.0, 0.0}; }
  __device__ __forceinline__ Vec2 u(int i) const { return i < nN ? Vec2{v[i], th[i]} : Vec2{0.0, 0.0}; }
  __device__ __forceinline__ unsigned long long fixbits() const { return bits; }
  __device__ __forceinline__ void fence() const { __asm__ volatile("" ::: "memory"); }
};

// the sink: dL/dI_e = explicit part + the adjoint's gI_e, stored once; the lane's share of the deflection term on the way
template <int M>
struct GradOut {
  const GradAcc<M>& acc;
  double* grad;
  bool store, nan;
  double defl;
  __device__ __forceinline__ void elem(int i, double gI, double) {
    if (store && i < acc.nE)
      grad[i] = nan ? __builtin_nan("") : sizing_explicit(acc.o, acc.I[i], acc.V[i], acc.q[i]) + gI;
  }
  __device__ __forceinline__ void node(int i, const Vec2&) {
    if (i < acc.nN) defl += sizing_defl(acc.o, acc.v[i]);
  }
};

template <int P, int M>
__global__ __launch_bounds__(64) void sizing_grad_kernel(const GradParams p) {
  constexpr int BPW = 64 / P;
  const int lane = threadIdx.x, g = lane / P, j = lane - g * P, e0 = j * M;
  const int Ne = p.Ne, N = Ne + 1;
  const long braw = (long)blockIdx.x * BPW + g;
  const bool live = braw < p.B && (!p.active || p.active[braw]);
  if (__ballot(live) == 0ull) return;             // every beam of the wave is finished (or beyond B)
  const long b = braw < p.B ? braw : (long)p.B - 1;   // lanes of a beam beyond B repeat beam B-1's arithmetic, store nothing
  const long bn = b * N + e0, be = b * Ne + e0;

  GradAcc<M> acc{p.x + b * p.x_bs + e0, nullptr, p.I + b * p.I_bs + e0, p.V + be, p.v + bn, p.theta + bn, p.o,
                 p.E_bs != 0, Ne - e0, N - e0, 0ull, {}};
  acc.E = acc.E_pe ? p.E + b * p.E_bs + e0 : p.E;
  {
    const uint8_t* fb = p.fix + b * p.fix_bs + e0;
    const double* Mb = p.M + be;
    unsigned long long bits = 0;
#pragma unroll
    for (int i = 0; i <= M; ++i)   // nodes at or beyond N are padding: free
      if (i < acc.nN) bits |= (unsigned long long)(fb[i] & 3) << (2 * i);
    acc.bits = bits;
#pragma unroll
    for (int i = 0; i < M; ++i)
      acc.q[i] = i < acc.nE ? sizing_quot(p.o, acc.I[i], acc.V[i], Mb[i]) : SizingQuot{0.0, 0.0};
  }

  // from here to the status: beam_vjp_kernel's phases, statement for statement
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

  const unsigned long long bal = __ballot(bad != 0);
  const unsigned long long grp = (P == 64) ? ~0ull : (((1ull << (P % 64)) - 1ull) << (g * P));
  const bool gbad = (bal & grp) != 0ull;
  if (j == 0 && live && p.status) p.status[b] = gbad ? 1 : 0;

  GradOut<M> out{acc, p.grad + be, live, gbad, 0.0};
  seg_solve_adj<M, true>(st, acc, lL, lR, out);

  if (p.loss_extra) {      // the beam's sum over its P lanes: a butterfly, the same order in every launch
    double d = out.defl;
#pragma unroll
    for (int s = P / 2; s >= 1; s >>= 1) d += __shfl_xor(d, s, 64);
    if (j == 0 && live) p.loss_extra[b] = gbad ? __builtin_nan("") : d;
  }
}

// beam_vjp.hip's tilings (kVjpTilings there): a tiling serves Ne with Ne + 1 <= P * M; the first one that serves is used
struct GradTiling { int P, M; };
static const GradTiling kGradTilings[] = {{16, 7}, {32, 4}, {64, 4}, {64, 8}, {64, 16}};

template <int P, int M>
static hipError_t launch_grad(const GradParams& p, hipStream_t stream) {
  constexpr int BPW = 64 / P;
  const unsigned grid = (unsigned)((p.B + BPW - 1) / BPW);
  hipLaunchKernelGGL((sizing_grad_kernel<P, M>), dim3(grid), dim3(64), 0, stream, p);
  return hipGetLastError();
}

// ops_beam_sizing_step_f32's kernel (sizing_step.hip) with the gradient read from memory
__global__ __launch_bounds__(256) void sizing_step_grad_kernel(int B, int Ne, const double* __restrict__ V,
                                                               const double* __restrict__ M, const double* __restrict__ grad,
                                                               const double* __restrict__ loss_extra, const SizingArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + wave;
  if (b >= B) return;
  if (!a.active[b]) return;   // wave-uniform
  const double* Vb = V + b * Ne;
  const double* Mb = M + b * Ne;
  sizing_case(lane, b, Ne, a, [&](int e) { return (float)Vb[e]; }, [&](int e) { return (float)Mb[e]; },
              GivenGrad{grad + b * Ne, loss_extra ? loss_extra + b : nullptr});
}

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_beam_sizing_grad_f64(int B, int Ne, const double* x, long x_bstride, const double* E, long E_bstride,
                                        const double* I, long I_bstride, const uint8_t* fix, long fix_bstride,
                                        const double* wy, long wy_bstride, const double* v, const double* theta,
                                        const double* V, const double* M, const ops_sizing_params* hp,
                                        const ops_sizing_objective* obj, const uint8_t* active, double* grad,
                                        double* loss_extra, int32_t* status, void* stream) {
  if (B < 0 || Ne < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!x || !E || !I || !fix || !wy || !v || !theta || !V || !M || !hp || !obj || !grad) return OPS_AMD_ERR_INVALID_ARG;
  if (!(obj->alpha_deflection >= 0.0)) return OPS_AMD_ERR_INVALID_ARG;
  if (obj->alpha_deflection > 0.0 && (!(obj->deflection_limit > 0.0) || !loss_extra)) return OPS_AMD_ERR_INVALID_ARG;
  if (I_bstride < Ne || (x_bstride != 0 && x_bstride < Ne + 1) || (fix_bstride != 0 && fix_bstride < Ne + 1) ||
      (E_bstride != 0 && E_bstride < Ne) || (wy_bstride != 0 && wy_bstride < Ne))
    return OPS_AMD_ERR_INVALID_ARG;
  if (Ne > ops_amd_max_elements()) return OPS_AMD_ERR_UNSUPPORTED;
  const GradTiling* t = nullptr;
  for (const GradTiling& c : kGradTilings)
    if (c.P * c.M >= Ne + 1) { t = &c; break; }
  if (!t) return OPS_AMD_ERR_UNSUPPORTED;
  // wy does not enter the arithmetic (V and M already hold the loads); validated like the forward's, as in the VJP
  const SizingObj o{hp->alpha_moment, hp->alpha_shear, 2.0 * hp->E, hp->bend_eps, hp->G * hp->area_coef,
                    obj->alpha_deflection, obj->alpha_deflection > 0.0 ? obj->deflection_limit : 1.0};
  const GradParams p{B, Ne, x, x_bstride, E, E_bstride, I, I_bstride, fix, fix_bstride, v, theta, V, M, o, active, grad, loss_extra, status};
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSuccess;
  if (t->P == 16 && t->M == 7) err = launch_grad<16, 7>(p, s);
  else if (t->P == 32 && t->M == 4) err = launch_grad<32, 4>(p, s);
  else if (t->P == 64 && t->M == 4) err = launch_grad<64, 4>(p, s);
  else if (t->P == 64 && t->M == 8) err = launch_grad<64, 8>(p, s);
  else err = launch_grad<64, 16>(p, s);
  return launch_status(err);
}

extern "C" int ops_beam_sizing_step_grad_f32(int B, int Ne, float* I, double* I64, const double* V, const double* M,
                                             const double* grad, const double* loss_extra, float* exp_avg, float* exp_avg_sq,
                                             float* best_loss, int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active,
                                             float* last_loss, float* V32, float* M32, const ops_sizing_params* hp,
                                             const float* schedule, void* stream) {
  if (B < 0 || Ne < 1 || Ne > kSizingMaxElems) return Ne > kSizingMaxElems ? OPS_AMD_ERR_UNSUPPORTED : OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!I || !I64 || !V || !M || !grad || !exp_avg || !exp_avg_sq || !best_loss || !patience_cnt || !epochs_run || !active ||
      !last_loss || ((V32 == nullptr) != (M32 == nullptr)) || !hp)
    return OPS_AMD_ERR_INVALID_ARG;
  SizingArgs a = sizing_args(I, exp_avg, exp_avg_sq, best_loss, patience_cnt, epochs_run, active, last_loss, hp);
  a.I64 = I64; a.V32 = V32; a.M32 = M32; a.schedule = schedule;
  return launch_wave_rows(sizing_step_grad_kernel, B, stream, B, Ne, V, M, grad, loss_extra, a);
}
