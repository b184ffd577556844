// Exact-gradient frame sizing for gfx950 (MI355X): the two streaming kernels around the adjoint solve that give dL/dI of the
// sizing objective with M, V, ux and uy as functions of I.  C ABI: include/openpystruct_amd_frame_sizing.h.  Arithmetic:
// frame_sizing_math.hpp over frame_adjoint.hpp and sizing_grad_math.hpp.  Design: DESIGN.md §9h.
//
// They are frame_vjp.hip's two kernels with the objective's cotangents formed in registers from this epoch's forward (disp, V,
// M, I) instead of read from arrays: gV, gM and g_disp never exist in memory.  The adjoint solve between them is the caller's
// (ops_frame_solve_batched_f64_ex, loads = rhs): the band kernels stay as they are.
//
// rhs kernel: the value of the two hinge terms is a sum over a frame's nodes, which one thread per (frame, node) cannot form
// without atomics.  A group of G lanes serves one frame, G the smallest of 4, 8, 16, 32, 64 that is >= min(Nn, 64): 64 / G frames
// per wavefront, lane j of a group takes nodes j, j + G, ... in ascending order, and a butterfly inside the group adds the G
// partial sums.  The order of every addition is a function of Nn alone: loss_extra does not depend on B, on the frame's place in
// the batch or on the grid.  Frames are dealt to wavefronts in order, so a wavefront stores one contiguous run of rhs rows per
// pass (with idle lanes where Nn < G).  No LDS, no atomics.
// grad kernel: one thread per (frame, element), as frame_grad_contract_kernel (frame_stream.hpp's row loop; both kernels go
// through its launch).
#include "frame_stream.hpp"

#include "../../include/openpystruct_amd_frame_sizing.h"
#include "frame_sizing_math.hpp"

namespace opsamd {

struct FrameSizingParams : FrameStreamTopo {
  const double* I;                 // [B,Ne]
  const double* disp;              // [B,Nn,3]  this epoch's forward
  const double* V; const double* M;   // [B,Ne]
  const double* lambda;            // [B,Nn,3]
  FrameSizingObj o;
  const uint8_t* active;           // [B] or NULL
  const int32_t* status_fwd; const int32_t* status_adj;   // [B] or NULL
  double* rhs;                     // [B,Nn,3]
  double* loss_extra;              // [B] or NULL
  double* grad;                    // [B,Ne]
};

template <int G>
__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_sizing_rhs_kernel(const FrameSizingParams p) {
  constexpr int FPW = 64 / G;           // frames per wavefront
  const int lane = threadIdx.x & 63, g = lane / G, j = lane - g * G;
  const long groups = ((long)p.B + FPW - 1) / FPW;
  const long wave = (long)blockIdx.x * (FRAME_STREAM_BLOCK / 64) + (threadIdx.x >> 6), waves = (long)gridDim.x * (FRAME_STREAM_BLOCK / 64);
  for (long w = wave; w < groups; w += waves) {      // wave-uniform trip count: every lane reaches the butterfly
    const long b = w * FPW + g;
    const bool inb = b < p.B;
    const bool live = inb && (!p.active || p.active[b]);
    double h = 0.0;
    if (inb) {
      for (int n = j; n < p.Nn; n += G) {
        double r[3] = {0.0, 0.0, 0.0};
        if (live)
          h += fs_node_rhs(p.o, p.Nn, p.Ne, p.elem_geo, p.elem_EA, p.elem_E, p.node_elem_ptr, p.node_elem_idx, p.I, p.disp,
                           p.V, p.M, b, n, r);
        double* o = p.rhs + (b * p.Nn + n) * 3;      // an inactive frame's rows: zeros, nothing loaded
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
      }
    }
    if (p.loss_extra && __ballot(live) != 0ull) {
#pragma unroll
      for (int s = G / 2; s >= 1; s >>= 1) h += __shfl_xor(h, s, 64);
      if (j == 0 && live) p.loss_extra[b] = h;
    }
  }
}

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_sizing_grad_kernel(const FrameSizingParams p) {
  frame_stream_rows(p.B, p.Ne, [&](long i, long b, int e) {
    if (p.active && !p.active[b]) return;
    const bool bad = (p.status_fwd && p.status_fwd[b] != 0) || (p.status_adj && p.status_adj[b] != 0);
    const double g = fs_elem_grad(p.o, p.Nn, p.Ne, p.elem_geo, p.elem_E, p.conn, p.I, p.V, p.M, p.disp, p.lambda, b, e);
    p.grad[i] = bad ? __builtin_nan("") : g;
  });
}

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_frame_sizing_rhs_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA,
                                        const double* elem_E, const int32_t* node_elem_ptr, const int32_t* node_elem_idx,
                                        const double* I, const double* disp, const double* V, const double* M,
                                        const ops_sizing_params* hp, const ops_frame_sizing_objective* obj,
                                        const uint8_t* active, double* rhs, double* loss_extra, void* stream) {
  if (B < 0 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_EA || !elem_E || !node_elem_ptr || !node_elem_idx || !I || !disp || !V || !M || !hp || !obj || !rhs)
    return OPS_AMD_ERR_INVALID_ARG;
  if (const int rc = frame_sizing_obj_check(obj, loss_extra); rc != OPS_AMD_OK) return rc;
  FrameSizingParams p{};
  p.B = B; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.elem_EA = elem_EA; p.elem_E = elem_E;
  p.node_elem_ptr = node_elem_ptr; p.node_elem_idx = node_elem_idx;
  p.I = I; p.disp = disp; p.V = V; p.M = M;
  p.o = frame_sizing_obj(hp, obj->alpha_sway, obj->sway_limit, obj->alpha_deflection, obj->deflection_limit);
  p.active = active; p.rhs = rhs; p.loss_extra = loss_extra;
  return frame_rhs_width(n_nodes, [&](auto W) { return frame_stream_launch(frame_sizing_rhs_kernel<W>, p, frame_rhs_threads(B, W), stream); });
}

extern "C" int ops_frame_sizing_grad_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                                         const int32_t* conn, const double* I, const double* disp, const double* V,
                                         const double* M, const double* lambda, const ops_sizing_params* hp,
                                         const uint8_t* active, const int32_t* status_fwd, const int32_t* status_adj,
                                         double* grad, void* stream) {
  if (B < 0 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_E || !conn || !I || !disp || !V || !M || !lambda || !hp || !grad) return OPS_AMD_ERR_INVALID_ARG;
  FrameSizingParams p{};
  p.B = B; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.elem_E = elem_E; p.conn = conn;
  p.I = I; p.disp = disp; p.V = V; p.M = M; p.lambda = lambda;
  p.o = frame_sizing_obj(hp, 0.0, 0.0, 0.0, 0.0);      // the hinges reach the gradient through lambda alone
  p.active = active; p.status_fwd = status_fwd; p.status_adj = status_adj; p.grad = grad;
  return frame_stream_launch(frame_sizing_grad_kernel, p, (long)B * n_elems, stream);
}
