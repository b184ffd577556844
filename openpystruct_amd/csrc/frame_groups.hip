// Frame sizing of one design under C load cases with LINKED design variables for gfx950 (MI355X): the design step of
// frame_designs.hip owning Ng <= Ne variables, one per group of elements that share a section.  C ABI:
// include/openpystruct_amd_frame_groups.h.  Arithmetic: frame_designs_math.hpp -- the walk over the cases, Adam on one variable and
// the early stop are the design step's own functions, called here on other variables.  Design: DESIGN.md §9n.
//
// Mapping: the design step's -- one 64-lane wavefront per design, four designs per 256-thread block, lane l takes elements
// l, l + 64, ... (K = 1, 2, 4, 8 per lane) through the walk -- and, once the walk has ended and the case registers are dead, lane l
// takes groups l, l + 64, ...  The exchange between the two roles goes through two LDS strips of the wave's own (64 K doubles:
// the per-element gradients; 64 K words: first group_elems, then the new variables): no atomics, a fixed summation order, and no
// workgroup barrier, because the waves of idle or out-of-range designs have returned.  LDS operations of one wave execute in issue
// order; fw_fence (lane_common.hpp) keeps the compiler from reordering across the hand-over and drains lgkmcnt before the reads.
#include "frame_stream.hpp"

#include "../../include/openpystruct_amd_frame_groups.h"
#include "../../include/openpystruct_amd_frame_frequency.h"
#include "frame_designs_math.hpp"

namespace opsamd {

struct FrameGroupArgs {
  FrameDesignArgs d;                 // d.s.I [G,Ne]: written only; d.s.exp_avg, d.s.exp_avg_sq, d.grad_out: [G,Ng]
  int Ng;
  const int32_t* elem_group;         // [Ne]
  const int32_t* group_ptr;          // [Ng+1]
  const int32_t* group_elems;        // [Ne]
  float* X;                          // [G,Ng]
};

struct FrameGroupDynArgs { FrameGroupArgs g; FrameStepExtras x; };      // the arguments of ops_frame_group_step_dyn_f32's kernels
template <bool DYN> using FrameGroupKernelArgs = std::conditional_t<DYN, FrameGroupDynArgs, FrameGroupArgs>;
__device__ __forceinline__ const FrameGroupArgs& fg_plain(const FrameGroupArgs& a) { return a; }
__device__ __forceinline__ const FrameGroupArgs& fg_plain(const FrameGroupDynArgs& a) { return a.g; }
__device__ __forceinline__ const FrameStepExtras* fg_extras(const FrameGroupArgs&) { return nullptr; }
__device__ __forceinline__ const FrameStepExtras* fg_extras(const FrameGroupDynArgs& a) { return &a.x; }

// gs: 64 K doubles, ws: 64 K words, both this wave's own.  DYN: the element gradients take x->grad_extra before the per-group sum
template <int K, bool SUM, bool DYN = false>
__device__ __forceinline__ void frame_group_step(int lane, long g, int Ne, const FrameGroupArgs& ga, double* gs, int32_t* ws,
                                                 const FrameStepExtras* x = nullptr) {
  const FrameDesignArgs& a = ga.d;
  const SizingArgs& s = a.s;
  const ops_sizing_params& hp = s.hp;
  const int Ng = ga.Ng;
  float* Xg = ga.X + g * Ng;
  float I32[K], Xo[K], m[K], v[K];
  int ge[K], eg[K], gp0[K], gp1[K];
  [[maybe_unused]] double gx[K], px;
  FdWalk<K> w;
  // the float32 inertia of element e is its group's variable (a label outside the table's range is held to it: the tables are the
  // caller's, and this is the one read of global memory they index)
  fd_design_walk<K, SUM>(lane, g, Ne, a, I32, [&](int ee) { return Xg[min((unsigned)ga.elem_group[ee], (unsigned)(Ng - 1))]; }, [&]() {
#pragma unroll
    for (int k = 0; k < K; ++k) {                 // everything the hand-over reads from memory, in flight under the last reductions:
      const int j = lane + 64 * k, e = j, jj = j < Ng ? j : 0, ee = e < Ne ? e : 0;
      const long o = g * Ng + jj;
      Xo[k] = ga.X[o];                            // this lane's groups: the variable, Adam's moments, the CSR range
      m[k] = s.exp_avg[o];
      v[k] = s.exp_avg_sq[o];
      gp0[k] = ga.group_ptr[jj];
      gp1[k] = ga.group_ptr[jj + 1];
      ge[k] = ga.group_elems[ee];                 // this lane's elements: their slice of the CSR's element list, their group
      eg[k] = ga.elem_group[ee];
      if constexpr (DYN) gx[k] = x->grad_extra[g * Ne + ee];
    }
    if constexpr (DYN) px = x->penalty_extra[g];
  }, w);
  if constexpr (DYN) fd_add_extras<K>(gx, px, w);

  // 1. the per-element gradients and the CSR's element list into the wave's strips
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    if (e < Ne) {
      gs[e] = w.g64[k];
      ws[e] = ge[k];
    }
  }
  fw_fence();
  // 2. gX[j] = g[e_0] + g[e_1] + ... in group_elems order, by the lane that owns group j.  The reads of a turn are issued together
  //    (positions past the group's end read its last element and are not added); the additions keep their order
  double gX[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane + 64 * k;
    gX[k] = 0.0;
    if (j < Ng) {
      const int p1 = min(gp1[k], Ne), p0 = min(max(gp0[k], 0), Ne - 1), last = p1 - 1;
      double acc = gs[ws[p0]];
      for (int p = p0 + 1; p < p1; p += 4) {
        const double t0 = gs[ws[p]], t1 = gs[ws[min(p + 1, last)]], t2 = gs[ws[min(p + 2, last)]], t3 = gs[ws[min(p + 3, last)]];
        acc += t0;
        if (p + 1 < p1) acc += t1;
        if (p + 2 < p1) acc += t2;
        if (p + 3 < p1) acc += t3;
      }
      gX[k] = acc;
    }
  }
  fw_fence();                                     // every lane has read the element list: its strip now takes the new variables
  // 3., 4. Adam and the clamp on the lane's groups (step_case); the new variables to memory and to the strip
  const FdAdam z = fd_adam_sizes(s, w.t_ep);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane + 64 * k;
    if (j < Ng) {
      const long o = g * Ng + j;
      if (a.grad_out) a.grad_out[o] = gX[k];
      float ea, es;
      const float Xn = fd_adam_var(hp, z, Xo[k], (float)gX[k], m[k], v[k], ea, es);
      s.exp_avg[o] = ea;
      s.exp_avg_sq[o] = es;
      ga.X[o] = Xn;
      ws[j] = __float_as_int(Xn);
    }
  }
  const bool stop = fd_early_stop(hp, w);
  fw_fence();
  // 5. the expansion I[e] = X[elem_group[e]], coalesced; I64 is what the next factorisation reads, once per design that goes on
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    if (e < Ne) {
      const float In = __int_as_float(ws[eg[k]]);
      s.I[g * Ne + e] = In;
      if (!stop) s.I64[g * Ne + e] = (double)In;
    }
  }
  fd_store_design(lane, g, a, w, stop);
}

template <int K, bool SUM, bool DYN = false>
__global__ __launch_bounds__(256) void frame_group_step_kernel(int G, int Ne, const FrameGroupKernelArgs<DYN> ka) {
  const FrameGroupArgs& a = fg_plain(ka);
  __shared__ double gs[4][64 * K];
  __shared__ int32_t ws[4][64 * K];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * 4 + wave;
  if (g >= G) return;
  if (!a.d.s.active[g]) return;   // wave-uniform
  frame_group_step<K, SUM, DYN>(lane, g, Ne, a, gs[wave], ws[wave], fg_extras(ka));
}

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_frame_group_step_f32(int G, int C, int n_nodes, int n_elems, int n_groups, const double* elem_geo,
                                        const double* elem_E, const int32_t* conn, const int32_t* elem_group, const int32_t* group_ptr,
                                        const int32_t* group_elems, float* X, float* I, double* I64, const double* disp, const double* V,
                                        const double* M, const double* lambda, const double* loss_extra, const int32_t* status_fwd,
                                        const int32_t* status_adj, const double* weights, int aggregate, float* exp_avg,
                                        float* exp_avg_sq, float* best_loss, int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active,
                                        float* last_loss, float* case_penalty, int32_t* governing, double* grad_out,
                                        const ops_sizing_params* hp, const float* schedule, void* stream) {
  if (n_groups < 1 || n_groups > n_elems) return OPS_AMD_ERR_INVALID_ARG;      // then the design step's refusals, in its order
  FrameGroupArgs a{};
  const int rc = frame_design_args(G, C, n_nodes, n_elems, elem_geo, elem_E, conn, I, I64, disp, V, M, lambda, loss_extra, status_fwd,
                                   status_adj, weights, aggregate, exp_avg, exp_avg_sq, best_loss, patience_cnt, epochs_run, active,
                                   last_loss, case_penalty, governing, grad_out, hp, schedule, &a.d);
  if (rc != OPS_AMD_OK || G == 0) return rc;
  if (!elem_group || !group_ptr || !group_elems || !X) return OPS_AMD_ERR_INVALID_ARG;
  a.Ng = n_groups; a.elem_group = elem_group; a.group_ptr = group_ptr; a.group_elems = group_elems; a.X = X;
  // K as a value and a table of template-ids, not the dispatch with a lambda: the order in which the eight kernels are named here
  // is their order in the code object, and that is kept
  const int K = sizing_lane_elems(n_elems);
  void (*kernel)(int, int, const FrameGroupArgs) = nullptr;
  if (aggregate == 0) kernel = K == 1 ? frame_group_step_kernel<1, true> : K == 2 ? frame_group_step_kernel<2, true> : K == 4 ? frame_group_step_kernel<4, true> : frame_group_step_kernel<8, true>;
  else kernel = K == 1 ? frame_group_step_kernel<1, false> : K == 2 ? frame_group_step_kernel<2, false> : K == 4 ? frame_group_step_kernel<4, false> : frame_group_step_kernel<8, false>;
  return launch_wave_rows(kernel, G, stream, G, n_elems, a);
}

// behind the plain step's eight kernels, in the same order
extern "C" int ops_frame_group_step_dyn_f32(int G, int C, int n_nodes, int n_elems, int n_groups, const double* elem_geo,
                                            const double* elem_E, const int32_t* conn, const int32_t* elem_group,
                                            const int32_t* group_ptr, const int32_t* group_elems, float* X, float* I, double* I64,
                                            const double* disp, const double* V, const double* M, const double* lambda,
                                            const double* loss_extra, const int32_t* status_fwd, const int32_t* status_adj,
                                            const double* weights, int aggregate, float* exp_avg, float* exp_avg_sq, float* best_loss,
                                            int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active, float* last_loss,
                                            float* case_penalty, int32_t* governing, double* grad_out, const ops_sizing_params* hp,
                                            const float* schedule, const double* grad_extra, const double* penalty_extra,
                                            void* stream) {
  if (n_groups < 1 || n_groups > n_elems) return OPS_AMD_ERR_INVALID_ARG;
  FrameGroupDynArgs a{};
  const int rc = frame_design_args(G, C, n_nodes, n_elems, elem_geo, elem_E, conn, I, I64, disp, V, M, lambda, loss_extra, status_fwd,
                                   status_adj, weights, aggregate, exp_avg, exp_avg_sq, best_loss, patience_cnt, epochs_run, active,
                                   last_loss, case_penalty, governing, grad_out, hp, schedule, &a.g.d);
  if (rc != OPS_AMD_OK || G == 0) return rc;
  if (!elem_group || !group_ptr || !group_elems || !X || !grad_extra || !penalty_extra) return OPS_AMD_ERR_INVALID_ARG;
  a.g.Ng = n_groups; a.g.elem_group = elem_group; a.g.group_ptr = group_ptr; a.g.group_elems = group_elems; a.g.X = X;
  a.x = FrameStepExtras{grad_extra, penalty_extra};
  const int K = sizing_lane_elems(n_elems);
  void (*kernel)(int, int, const FrameGroupDynArgs) = nullptr;
  if (aggregate == 0) kernel = K == 1 ? frame_group_step_kernel<1, true, true> : K == 2 ? frame_group_step_kernel<2, true, true> : K == 4 ? frame_group_step_kernel<4, true, true> : frame_group_step_kernel<8, true, true>;
  else kernel = K == 1 ? frame_group_step_kernel<1, false, true> : K == 2 ? frame_group_step_kernel<2, false, true> : K == 4 ? frame_group_step_kernel<4, false, true> : frame_group_step_kernel<8, false, true>;
  return launch_wave_rows(kernel, G, stream, G, n_elems, a);
}
