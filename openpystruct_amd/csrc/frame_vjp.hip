// Vector-Jacobian product of the batched frame solve for gfx950 (MI355X): the two streaming kernels around the adjoint
// solve.  C ABI: include/openpystruct_amd_frame_vjp.h.  Arithmetic:
// frame_adjoint.hpp.  Design: DESIGN.md §9f.
//
// The stiffness matrix is symmetric, so the adjoint system is the forward system with another right-hand side: the caller
// runs ops_frame_solve_batched_f64_ex between the two kernels (loads = rhs, per frame; elem_w = zeros) and the band kernels
// stay as they are.  Both kernels are one thread per output row, (frame, node) and (frame, element): the row loop and the
// launch are frame_stream.hpp's.
#include "frame_stream.hpp"

#include "../../include/openpystruct_amd_frame_vjp.h"
#include "frame_adjoint.hpp"

namespace opsamd {

struct FrameVjpParams : FrameStreamTopo {
  const double* I;                 // [B,Ne]
  const double* disp;              // [B,Nn,3]
  const double* lambda;            // [B,Nn,3]
  const double* g_disp;            // [B,Nn,3] or NULL
  const double* g_forces;          // [B,Ne,6] or NULL
  const double* gV; const double* gM;   // [B,Ne] or NULL
  const int32_t* status_fwd; const int32_t* status_adj;   // [B] or NULL
  double* rhs;                     // [B,Nn,3]
  double* gI;                      // [B,Ne]
};

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_adjoint_rhs_kernel(const FrameVjpParams p) {
  frame_stream_rows(p.B, p.Nn, [&](long i, long b, int n) {
    double r[3];
    fa_node_rhs(p.Nn, p.Ne, p.elem_geo, p.elem_EA, p.elem_E, p.node_elem_ptr, p.node_elem_idx, p.I, p.g_disp, p.g_forces,
                p.gV, p.gM, b, n, r);
    double* o = p.rhs + i * 3;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
  });
}

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_grad_contract_kernel(const FrameVjpParams p) {
  frame_stream_rows(p.B, p.Ne, [&](long i, long b, int e) {
    const bool bad = (p.status_fwd && p.status_fwd[b] != 0) || (p.status_adj && p.status_adj[b] != 0);
    const double g = fa_elem_gI(p.Nn, p.Ne, p.elem_geo, p.elem_E, p.conn, p.disp, p.lambda, p.g_forces, p.gV, p.gM, b, e);
    p.gI[i] = bad ? __builtin_nan("") : g;
  });
}

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_frame_adjoint_rhs_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA,
                                         const double* elem_E, const int32_t* conn, const int32_t* node_elem_ptr,
                                         const int32_t* node_elem_idx, const double* I, const double* g_disp,
                                         const double* g_forces, const double* gV, const double* gM, double* rhs,
                                         void* stream) {
  if (B < 0 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_EA || !elem_E || !conn || !node_elem_ptr || !node_elem_idx || !I || !rhs) return OPS_AMD_ERR_INVALID_ARG;
  FrameVjpParams p{};
  p.B = B; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.elem_EA = elem_EA; p.elem_E = elem_E;
  p.conn = conn; p.node_elem_ptr = node_elem_ptr; p.node_elem_idx = node_elem_idx;
  p.I = I; p.g_disp = g_disp; p.g_forces = g_forces; p.gV = gV; p.gM = gM; p.rhs = rhs;
  return frame_stream_launch(frame_adjoint_rhs_kernel, p, (long)B * n_nodes, stream);
}

extern "C" int ops_frame_grad_contract_f64(int B, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E,
                                           const int32_t* conn, const double* disp, const double* lambda,
                                           const double* g_forces, const double* gV, const double* gM,
                                           const int32_t* status_fwd, const int32_t* status_adj, double* gI, void* stream) {
  if (B < 0 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_E || !conn || !disp || !lambda || !gI) return OPS_AMD_ERR_INVALID_ARG;
  FrameVjpParams p{};
  p.B = B; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.elem_E = elem_E; p.conn = conn;
  p.disp = disp; p.lambda = lambda; p.g_forces = g_forces; p.gV = gV; p.gM = gM;
  p.status_fwd = status_fwd; p.status_adj = status_adj; p.gI = gI;
  return frame_stream_launch(frame_grad_contract_kernel, p, (long)B * n_elems, stream);
}
