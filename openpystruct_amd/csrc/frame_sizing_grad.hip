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
// grad kernel: one thread per (frame, element), as frame_grad_contract_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openpystruct_amd_frame_sizing.h"
#include "frame_sizing_math.hpp"
#include "library.hpp"

namespace opsamd {

struct FrameSizingParams {
  int B, Nn, Ne;
  const double* elem_geo;          // [Ne,3]  L, cos, sin
  const double* elem_EA;           // [Ne]
  const double* elem_E;            // [Ne]
  const int32_t* conn;             // [Ne,2]
  const int32_t* node_elem_ptr;    // [Nn+1]
  const int32_t* node_elem_idx;    // [2 Ne]  2 * element + end
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

constexpr int FS_BLOCK = 256;
constexpr long FS_MAX_GRID = 2048;     // memory-bound: a few workgroups per CU, the rest by grid stride

template <int G>
__global__ __launch_bounds__(FS_BLOCK) void frame_sizing_rhs_kernel(const FrameSizingParams p) {
  constexpr int FPW = 64 / G;           // frames per wavefront
  const int lane = threadIdx.x & 63, g = lane / G, j = lane - g * G;
  const long groups = ((long)p.B + FPW - 1) / FPW;
  const long wave = (long)blockIdx.x * (FS_BLOCK / 64) + (threadIdx.x >> 6), waves = (long)gridDim.x * (FS_BLOCK / 64);
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

// frame of row i of `total` rows, `per` rows to a frame (frame_vjp.hip: the 64-bit division is a long instruction sequence)
__device__ __forceinline__ long fs_row_frame(long i, int per, bool small) {
  return small ? (long)((unsigned)i / (unsigned)per) : i / per;
}

__global__ __launch_bounds__(FS_BLOCK) void frame_sizing_grad_kernel(const FrameSizingParams p) {
  const long total = (long)p.B * p.Ne, stride = (long)gridDim.x * FS_BLOCK;
  for (long i = (long)blockIdx.x * FS_BLOCK + threadIdx.x; i < total; i += stride) {
    const long b = fs_row_frame(i, p.Ne, total <= 0x7fffffffL);
    if (p.active && !p.active[b]) continue;
    const int e = (int)(i - b * p.Ne);
    const bool bad = (p.status_fwd && p.status_fwd[b] != 0) || (p.status_adj && p.status_adj[b] != 0);
    const double g = fs_elem_grad(p.o, p.Nn, p.Ne, p.elem_geo, p.elem_E, p.conn, p.I, p.V, p.M, p.disp, p.lambda, b, e);
    p.grad[i] = bad ? __builtin_nan("") : g;
  }
}

template <int G>
static hipError_t launch_rhs(const FrameSizingParams& p, hipStream_t stream) {
  constexpr int FPW = 64 / G;
  const long groups = ((long)p.B + FPW - 1) / FPW, per_block = FS_BLOCK / 64;
  const long need = (groups + per_block - 1) / per_block;
  const unsigned grid = (unsigned)(need < FS_MAX_GRID ? need : FS_MAX_GRID);
  hipLaunchKernelGGL((frame_sizing_rhs_kernel<G>), dim3(grid), dim3(FS_BLOCK), 0, stream, p);
  return hipGetLastError();
}

static int launched(hipError_t err) {
  if (err != hipSuccess) {
    set_last_error(hipGetErrorString(err));
    return OPS_AMD_ERR_LAUNCH;
  }
  return OPS_AMD_OK;
}

static FrameSizingObj objective(const ops_sizing_params* hp, double aS, double s_lim, double aD, double d_lim) {
  return frame_sizing_obj(hp->alpha_moment, hp->alpha_shear, hp->E, hp->bend_eps, hp->G, hp->area_coef, aS, s_lim, aD, d_lim);
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
  if (!(obj->alpha_sway >= 0.0) || !(obj->alpha_deflection >= 0.0)) return OPS_AMD_ERR_INVALID_ARG;
  if (obj->alpha_sway > 0.0 && !(obj->sway_limit > 0.0)) return OPS_AMD_ERR_INVALID_ARG;
  if (obj->alpha_deflection > 0.0 && !(obj->deflection_limit > 0.0)) return OPS_AMD_ERR_INVALID_ARG;
  if (obj->alpha_sway + obj->alpha_deflection > 0.0 && !loss_extra) return OPS_AMD_ERR_INVALID_ARG;
  FrameSizingParams p{};
  p.B = B; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.elem_EA = elem_EA; p.elem_E = elem_E;
  p.node_elem_ptr = node_elem_ptr; p.node_elem_idx = node_elem_idx;
  p.I = I; p.disp = disp; p.V = V; p.M = M;
  p.o = objective(hp, obj->alpha_sway, obj->sway_limit, obj->alpha_deflection, obj->deflection_limit);
  p.active = active; p.rhs = rhs; p.loss_extra = loss_extra;
  hipStream_t s = (hipStream_t)stream;
  if (n_nodes <= 4) return launched(launch_rhs<4>(p, s));
  if (n_nodes <= 8) return launched(launch_rhs<8>(p, s));
  if (n_nodes <= 16) return launched(launch_rhs<16>(p, s));
  if (n_nodes <= 32) return launched(launch_rhs<32>(p, s));
  return launched(launch_rhs<64>(p, s));
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
  p.o = objective(hp, 0.0, 0.0, 0.0, 0.0);      // the hinges reach the gradient through lambda alone
  p.active = active; p.status_fwd = status_fwd; p.status_adj = status_adj; p.grad = grad;
  const long need = ((long)B * n_elems + FS_BLOCK - 1) / FS_BLOCK;
  const unsigned grid = (unsigned)(need < FS_MAX_GRID ? need : FS_MAX_GRID);
  hipLaunchKernelGGL(frame_sizing_grad_kernel, dim3(grid), dim3(FS_BLOCK), 0, (hipStream_t)stream, p);
  return launched(hipGetLastError());
}
