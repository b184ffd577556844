// Per-frame element loads around the batched frame solve for gfx950 (MI355X): three streaming kernels.  C ABI:
// include/openpystruct_amd_frame_loads.h.  Arithmetic: frame_loads.hpp.  Design: DESIGN.md §9i.
//
// The solve is linear in the element loads, so the band kernels stay as they are: the caller runs
// ops_frame_solve_batched_f64_ex between the first two kernels (loads = rhs, per frame; elem_w = zeros).  All three kernels
// are one thread per output row, (frame, node) or (frame, element), by frame_stream.hpp's row loop and launch: the same bits
// for every batch size and every position of a frame in the batch.
#include "frame_stream.hpp"

#include "../../include/openpystruct_amd_frame_loads.h"
#include "frame_loads.hpp"

namespace opsamd {

struct FrameLoadParams : FrameStreamTopo {
  const double* loads;             // [Nn,3] or [B,Nn,3]
  const double* elem_w;            // [Ne,2] or [B,Ne,2]  wy, wx
  long loads_bstride, w_bstride;
  const double* lambda;            // [B,Nn,3]
  const double* g_forces;          // [B,Ne,6] or NULL
  const double* gV; const double* gM;   // [B,Ne] or NULL
  const int32_t* status; const int32_t* status_adj;   // [B] or NULL
  double* rhs;                     // [B,Nn,3]
  double* forces;                  // [B,Ne,6]
  double* V; double* M;            // [B,Ne]
  double* g_w;                     // [B,Ne,2]
};

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_load_rhs_kernel(const FrameLoadParams p) {
  frame_stream_rows(p.B, p.Nn, [&](long i, long b, int n) {
    double r[3];
    fl_node_rhs(p.Nn, p.elem_geo, p.node_elem_ptr, p.node_elem_idx, p.loads, p.loads_bstride, p.elem_w, p.w_bstride, b, n, r);
    double* o = p.rhs + i * 3;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
  });
}

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_load_forces_kernel(const FrameLoadParams p) {
  frame_stream_rows(p.B, p.Ne, [&](long i, long b, int e) {
    if (p.status && p.status[b] != 0) return;         // a failed frame keeps the solve's NaN rows
    double* fo = p.forces + i * 6;
    double f[6];
    for (int k = 0; k < 6; ++k) f[k] = fo[k];
    fl_elem_forces(p.elem_geo, p.elem_w, p.w_bstride, b, e, f);
    for (int k = 0; k < 6; ++k) fo[k] = f[k];
    p.V[i] = f[1];
    p.M[i] = f[2];
  });
}

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_load_vjp_kernel(const FrameLoadParams p) {
  frame_stream_rows(p.B, p.Ne, [&](long i, long b, int e) {
    const bool bad = (p.status && p.status[b] != 0) || (p.status_adj && p.status_adj[b] != 0);
    double gw[2];
    fl_elem_gw(p.Nn, p.Ne, p.elem_geo, p.conn, p.lambda, p.g_forces, p.gV, p.gM, b, e, gw);
    p.g_w[2 * i] = bad ? __builtin_nan("") : gw[0];
    p.g_w[2 * i + 1] = bad ? __builtin_nan("") : gw[1];
  });
}

static bool stride_ok(long stride, long full) { return stride == 0 || stride == full; }

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_frame_load_rhs_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const int32_t* node_elem_ptr,
                                      const int32_t* node_elem_idx, const double* loads, long loads_bstride,
                                      const double* elem_w, long w_bstride, double* rhs, void* stream) {
  if (B < 0 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (!stride_ok(loads_bstride, 3L * n_nodes) || !stride_ok(w_bstride, 2L * n_elems)) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !node_elem_ptr || !node_elem_idx || !loads || !elem_w || !rhs) return OPS_AMD_ERR_INVALID_ARG;
  FrameLoadParams p{};
  p.B = B; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.node_elem_ptr = node_elem_ptr; p.node_elem_idx = node_elem_idx;
  p.loads = loads; p.loads_bstride = loads_bstride; p.elem_w = elem_w; p.w_bstride = w_bstride; p.rhs = rhs;
  return frame_stream_launch(frame_load_rhs_kernel, p, (long)B * n_nodes, stream);
}

extern "C" int ops_frame_load_forces_f64(int B, int n_elems, const double* elem_geo, const double* elem_w, long w_bstride,
                                         const int32_t* status, double* forces, double* V, double* M, void* stream) {
  if (B < 0 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (!stride_ok(w_bstride, 2L * n_elems)) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_w || !forces || !V || !M) return OPS_AMD_ERR_INVALID_ARG;
  FrameLoadParams p{};
  p.B = B; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.elem_w = elem_w; p.w_bstride = w_bstride; p.status = status;
  p.forces = forces; p.V = V; p.M = M;
  return frame_stream_launch(frame_load_forces_kernel, p, (long)B * n_elems, stream);
}

extern "C" int ops_frame_load_vjp_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const int32_t* conn,
                                      const double* lambda, const double* g_forces, const double* gV, const double* gM,
                                      const int32_t* status_fwd, const int32_t* status_adj, double* g_w, void* stream) {
  if (B < 0 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !conn || !lambda || !g_w) return OPS_AMD_ERR_INVALID_ARG;
  FrameLoadParams p{};
  p.B = B; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.conn = conn; p.lambda = lambda; p.g_forces = g_forces; p.gV = gV; p.gM = gM;
  p.status = status_fwd; p.status_adj = status_adj; p.g_w = g_w;
  return frame_stream_launch(frame_load_vjp_kernel, p, (long)B * n_elems, stream);
}
