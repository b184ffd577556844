// Frame sizing of ONE design under C load cases for gfx950 (MI355X): the two launches that tie the cases of a design together
// around the kept factorisation of §9k.  C ABI: include/openpystruct_amd_frame_designs.h.  Arithmetic: frame_designs_math.hpp over
// frame_sizing_math.hpp (§9h) and sizing_multicase_math.hpp (§9j).  Design: DESIGN.md §9l.
//
// rhs kernel: frame_sizing_rhs_kernel's mapping -- a group of W lanes per row (W the smallest of 4 .. 64 that is >= min(Nn, 64)),
// lane j of a group takes nodes j, j + W, ... in ascending order, a butterfly inside the group adds the partial hinge sums -- on the
// G * C rows, the inertia read by design (row / C) and `active` per design.  No LDS, no atomics.
// step kernel: sizing_multicase_kernel's mapping -- one 64-lane wavefront per design, four designs per 256-thread block, lane e
// takes elements e, e + 64, ... (K = 1, 2, 4, 8 per lane) -- with the gradient of every case formed in registers from the end-node
// values of disp and lambda: the [G*C, Ne] gradient rows of §9h never exist in memory and the inertias exist once per design.
// The wave walks the cases in index order; the next case's loads are issued before this case's wave reductions.
#include "frame_stream.hpp"

#include "../../include/openpystruct_amd_frame_designs.h"
#include "../../include/openpystruct_amd_frame_frequency.h"
#include "frame_designs_math.hpp"

namespace opsamd {

struct FrameDesignRhsParams : FrameStreamTopo {      // B: the G * C rows
  int C;
  const double* I;                 // [G,Ne]
  const double* disp;              // [B,Nn,3]
  const double* V; const double* M;   // [B,Ne]
  FrameSizingObj o;
  const uint8_t* active;           // [G] or NULL
  double* rhs;                     // [B,Nn,3]
  double* loss_extra;              // [B] or NULL
};

template <int W>
__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_design_rhs_kernel(const FrameDesignRhsParams p) {
  constexpr int RPW = 64 / W;           // rows per wavefront
  const int lane = threadIdx.x & 63, q = lane / W, j = lane - q * W;
  const long groups = ((long)p.B + RPW - 1) / RPW;
  const long wave = (long)blockIdx.x * (FRAME_STREAM_BLOCK / 64) + (threadIdx.x >> 6), waves = (long)gridDim.x * (FRAME_STREAM_BLOCK / 64);
  for (long w = wave; w < groups; w += waves) {      // wave-uniform trip count: every lane reaches the butterfly
    const long b = w * RPW + q;
    const bool inb = b < p.B;
    const long d = inb ? (long)((unsigned)b / (unsigned)p.C) : 0;      // the row's design (B fits 31 bits)
    const bool live = inb && (!p.active || p.active[d]);
    double h = 0.0;
    if (inb) {
      for (int n = j; n < p.Nn; n += W) {
        double r[3] = {0.0, 0.0, 0.0};
        if (live)
          h += fd_node_rhs(p.o, p.Nn, p.Ne, p.elem_geo, p.elem_EA, p.elem_E, p.node_elem_ptr, p.node_elem_idx, p.I, p.disp,
                           p.V, p.M, d, b, n, r);
        double* o = p.rhs + (b * p.Nn + n) * 3;      // an inactive design's rows: zeros, nothing loaded
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
      }
    }
    if (p.loss_extra && __ballot(live) != 0ull) {
#pragma unroll
      for (int s = W / 2; s >= 1; s >>= 1) h += __shfl_xor(h, s, 64);
      if (j == 0 && live) p.loss_extra[b] = h;
    }
  }
}

// DYN: the step of ops_frame_design_step_dyn_f32, which takes a gradient and a penalty formed outside it (FrameStepExtras)
template <int K, bool SUM, bool DYN = false>
__global__ __launch_bounds__(256) void frame_design_step_kernel(int G, int Ne, const FrameDesignKernelArgs<DYN> ka) {
  const FrameDesignArgs& a = fd_plain(ka);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * 4 + wave;      // a scalar: every row base of the design is one
  if (g >= G) return;
  if (!a.s.active[g]) return;   // wave-uniform
  frame_design_step<K, SUM, DYN>(lane, g, Ne, a, fd_extras(ka));
}

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_frame_design_max_cases(void) { return kFrameDesignMaxCases; }

extern "C" int ops_frame_design_rhs_f64(int G, int C, int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA,
                                        const double* elem_E, const int32_t* node_elem_ptr, const int32_t* node_elem_idx,
                                        const double* I64, const double* disp, const double* V, const double* M,
                                        const ops_sizing_params* hp, const ops_frame_sizing_objective* obj,
                                        const uint8_t* active, double* rhs, double* loss_extra, void* stream) {
  if (G < 0 || C < 1 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (n_elems > kSizingMaxElems || C > kFrameDesignMaxCases || (long)G * C > 0x7fffffffL) return OPS_AMD_ERR_UNSUPPORTED;
  if (G == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_EA || !elem_E || !node_elem_ptr || !node_elem_idx || !I64 || !disp || !V || !M || !hp || !obj || !rhs)
    return OPS_AMD_ERR_INVALID_ARG;
  if (const int rc = frame_sizing_obj_check(obj, loss_extra); rc != OPS_AMD_OK) return rc;
  FrameDesignRhsParams p{};
  p.B = G * C; p.Nn = n_nodes; p.Ne = n_elems; p.C = C;
  p.elem_geo = elem_geo; p.elem_EA = elem_EA; p.elem_E = elem_E;
  p.node_elem_ptr = node_elem_ptr; p.node_elem_idx = node_elem_idx;
  p.I = I64; p.disp = disp; p.V = V; p.M = M;
  p.o = frame_sizing_obj(hp, obj->alpha_sway, obj->sway_limit, obj->alpha_deflection, obj->deflection_limit);
  p.active = active; p.rhs = rhs; p.loss_extra = loss_extra;
  return frame_rhs_width(n_nodes, [&](auto W) { return frame_stream_launch(frame_design_rhs_kernel<W>, p, frame_rhs_threads(p.B, W), stream); });
}

extern "C" int ops_frame_design_step_f32(int G, int C, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                                         const int32_t* conn, float* I, double* I64, const double* disp, const double* V,
                                         const double* M, const double* lambda, const double* loss_extra,
                                         const int32_t* status_fwd, const int32_t* status_adj, const double* weights,
                                         int aggregate, float* exp_avg, float* exp_avg_sq, float* best_loss,
                                         int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active, float* last_loss,
                                         float* case_penalty, int32_t* governing, double* grad_out, const ops_sizing_params* hp,
                                         const float* schedule, void* stream) {
  FrameDesignArgs a{};
  const int rc = frame_design_args(G, C, n_nodes, n_elems, elem_geo, elem_E, conn, I, I64, disp, V, M, lambda, loss_extra, status_fwd,
                                   status_adj, weights, aggregate, exp_avg, exp_avg_sq, best_loss, patience_cnt, epochs_run, active,
                                   last_loss, case_penalty, governing, grad_out, hp, schedule, &a);
  if (rc != OPS_AMD_OK || G == 0) return rc;
  // K as a value and a table of template-ids, not the dispatch with a lambda: the order in which the eight kernels are named here
  // is their order in the code object, and that is kept
  const int K = sizing_lane_elems(n_elems);
  void (*kernel)(int, int, const FrameDesignArgs) = nullptr;
  if (aggregate == 0) kernel = K == 1 ? frame_design_step_kernel<1, true> : K == 2 ? frame_design_step_kernel<2, true> : K == 4 ? frame_design_step_kernel<4, true> : frame_design_step_kernel<8, true>;
  else kernel = K == 1 ? frame_design_step_kernel<1, false> : K == 2 ? frame_design_step_kernel<2, false> : K == 4 ? frame_design_step_kernel<4, false> : frame_design_step_kernel<8, false>;
  return launch_wave_rows(kernel, G, stream, G, n_elems, a);
}

// behind the plain step's eight kernels, in the same order: K = 1, 2, 4, 8 under "sum", then under "max"
extern "C" int ops_frame_design_step_dyn_f32(int G, int C, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                                             const int32_t* conn, float* I, double* I64, const double* disp, const double* V,
                                             const double* M, const double* lambda, const double* loss_extra,
                                             const int32_t* status_fwd, const int32_t* status_adj, const double* weights,
                                             int aggregate, float* exp_avg, float* exp_avg_sq, float* best_loss,
                                             int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active, float* last_loss,
                                             float* case_penalty, int32_t* governing, double* grad_out, const ops_sizing_params* hp,
                                             const float* schedule, const double* grad_extra, const double* penalty_extra,
                                             void* stream) {
  FrameDesignDynArgs a{};
  const int rc = frame_design_args(G, C, n_nodes, n_elems, elem_geo, elem_E, conn, I, I64, disp, V, M, lambda, loss_extra, status_fwd,
                                   status_adj, weights, aggregate, exp_avg, exp_avg_sq, best_loss, patience_cnt, epochs_run, active,
                                   last_loss, case_penalty, governing, grad_out, hp, schedule, &a.a);
  if (rc != OPS_AMD_OK || G == 0) return rc;
  if (!grad_extra || !penalty_extra) return OPS_AMD_ERR_INVALID_ARG;
  a.x = FrameStepExtras{grad_extra, penalty_extra};
  const int K = sizing_lane_elems(n_elems);
  void (*kernel)(int, int, const FrameDesignDynArgs) = nullptr;
  if (aggregate == 0) kernel = K == 1 ? frame_design_step_kernel<1, true, true> : K == 2 ? frame_design_step_kernel<2, true, true> : K == 4 ? frame_design_step_kernel<4, true, true> : frame_design_step_kernel<8, true, true>;
  else kernel = K == 1 ? frame_design_step_kernel<1, false, true> : K == 2 ? frame_design_step_kernel<2, false, true> : K == 4 ? frame_design_step_kernel<4, false, true> : frame_design_step_kernel<8, false, true>;
  return launch_wave_rows(kernel, G, stream, G, n_elems, a);
}
