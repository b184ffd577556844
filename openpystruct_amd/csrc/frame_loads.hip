// Per-frame element loads around the batched frame solve for gfx950 (MI355X): three streaming kernels.  C ABI:
// include/openpystruct_amd_frame_loads.h.  Arithmetic: frame_loads.hpp.  Design: DESIGN.md §9i.
// Behind them, on the same node-walk tables: the three kernels of the natural frequencies on the kept factorisation (mass apply,
// Ritz step, eigenvalue gradient).  Arithmetic: frame_modes.hpp.  Design: DESIGN.md §9p.
// And the three kernels of the linear buckling load factors (geometric-stiffness apply, Ritz step of the swapped pencil, gradient
// terms).  Arithmetic: frame_buckling.hpp.  Design: DESIGN.md §9q.
// Last, the kernel of the natural-frequency floor of design sizing (the hinge on the eigenvalues and its gradient).  Arithmetic:
// frame_modes.hpp.  C ABI: include/openpystruct_amd_frame_frequency.h.  Design: DESIGN.md §9r.
//
// The solve is linear in the element loads, so the band kernels stay as they are: the caller runs
// ops_frame_solve_batched_f64_ex between the first two kernels (loads = rhs, per frame; elem_w = zeros).  All three kernels
// are one thread per output row, (frame, node) or (frame, element), by frame_stream.hpp's row loop and launch: the same bits
// for every batch size and every position of a frame in the batch.
#include "frame_stream.hpp"

#include "../../include/openpystruct_amd_frame_loads.h"
#include "../../include/openpystruct_amd_frame_frequency.h"
#include "frame_loads.hpp"
#include "frame_buckling.hpp"
#include "frame_modes.hpp"
#include "sizing_math.hpp"

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

// ---- natural frequencies on the kept factorisation ----
struct FrameModeParams : FrameStreamTopo {      // B: the rows of the mass apply, the frames of the gradient
  const double* elem_mass;         // [Ne] mass per unit length
  const double* nodal_mass;        // [Nn,3], [B,Nn,3] or NULL
  long nodal_bstride;
  int consistent, rows_per_frame, m, p;
  const double* x;                 // [R,Nn,3]; the gradient: phi [B,p,Nn,3]
  double* y;                       // [R,Nn,3]
  const double* g_lambda;          // [B,m]
  const int32_t* status;           // [B]
  double* gI;                      // [B,Ne]
};

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_mass_apply_kernel(const FrameModeParams p) {
  frame_stream_rows(p.B, p.Nn, [&](long i, long row, int n) {
    double y[3];
    fm_node_mass(p.Nn, p.elem_geo, p.conn, p.node_elem_ptr, p.node_elem_idx, p.elem_mass, p.consistent, p.nodal_mass,
                 p.nodal_bstride, p.x, row, row / p.rows_per_frame, n, y);
    double* o = p.y + i * 3;
    o[0] = y[0]; o[1] = y[1]; o[2] = y[2];
  });
}

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_modes_grad_kernel(const FrameModeParams p) {
  frame_stream_rows(p.B, p.Ne, [&](long i, long b, int e) {
    const double g = fm_elem_grad(p.m, p.p, p.Nn, p.elem_geo, p.elem_E, p.conn, p.x, p.g_lambda, b, e);
    p.gI[i] = p.status[b] != 0 ? __builtin_nan("") : g;
  });
}

struct FrameRitzArgs {
  const double* X; const double* MX;     // [B,P,Nn,3]
  double* R; double* Q;                  // [B,P,Nn,3]  R: read as M Q of the iteration before, written as the next one's
  double* lambda; double* change;        // [B,P]       lambda: read as the iteration before's
  const int32_t* row_status;             // [B,P]
  int32_t* status;                       // [B]
};

// one wavefront per frame: the partial sums of the lane's entries, the butterfly over the 64 lanes (every lane ends with the same
// bits: an addition does not depend on the order of its two operands), the small dense part on every lane, the lane's entries of Q, R
template <int P>
__global__ __launch_bounds__(256) void frame_modes_ritz_kernel(int B, int n_nodes, const FrameRitzArgs a) {
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const long n = 3L * n_nodes, base = b * P * n;
  const double *x = a.X + base, *mx = a.MX + base;
  double *r = a.R + base, *q = a.Q + base;
  int st = 0;
  for (int j = 0; j < P; ++j) st |= a.row_status[b * P + j] != 0;
  double Z[P * P], lam[P], change[P];
  if (st == 0) {
    double acc[FmRitz<P>::NACC];
    fm_ritz_partials<P>(n, x, mx, r, lane, acc);
#pragma unroll
    for (int k = 0; k < FmRitz<P>::NACC; ++k)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    double prev[P];
#pragma unroll
    for (int j = 0; j < P; ++j) prev[j] = a.lambda[b * P + j];
    int sweeps;
    st = fm_ritz_small<P>(acc, prev, Z, lam, change, &sweeps);
  }
  if (st != 0) {      // NaN for this frame alone; R stays, so the next iteration fails the same way with the same status
    const double nan = __builtin_nan("");
    for (long t = lane; t < P * n; t += 64) q[t] = nan;
#pragma unroll
    for (int j = 0; j < P; ++j) lam[j] = change[j] = nan;
  } else {
    fm_ritz_update<P>(n, x, mx, Z, lane, q, r);
  }
  if (lane < P) {
    double l = lam[0], c = change[0];
#pragma unroll
    for (int j = 1; j < P; ++j)
      if (lane == j) { l = lam[j]; c = change[j]; }
    a.lambda[b * P + lane] = l;
    a.change[b * P + lane] = c;
  }
  if (lane == 0) a.status[b] = st;
}

// ---- linear buckling load factors on the kept factorisation ----
struct FrameBucklingParams : FrameStreamTopo {  // B: the rows of the geometric apply, the frames of the gradient
  const double* forces;            // [B,Ne,6] the reference solve's end forces
  int consistent, rows_per_frame, m, p;
  const double* x;                 // [R,Nn,3]; the gradient: phi [B,p,Nn,3]
  double* y;                       // [R,Nn,3]
  const double* lambda;            // [B,m]
  const double* g_lambda;          // [B,m]
  const int32_t* status;           // [B]
  double* gI_direct;               // [B,Ne]
  double* g_forces;                // [B,Ne,6]
};

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_geom_apply_kernel(const FrameBucklingParams p) {
  frame_stream_rows(p.B, p.Nn, [&](long i, long row, int n) {
    double y[3];
    fb_node_geom(p.Nn, p.Ne, p.elem_geo, p.conn, p.node_elem_ptr, p.node_elem_idx, p.forces, p.consistent, p.x, row,
                 row / p.rows_per_frame, n, y);
    double* o = p.y + i * 3;
    o[0] = y[0]; o[1] = y[1]; o[2] = y[2];
  });
}

__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_buckling_grad_kernel(const FrameBucklingParams p) {
  frame_stream_rows(p.B, p.Ne, [&](long i, long b, int e) {
    double d, gf[6];
    fb_elem_grad(p.m, p.p, p.Nn, p.elem_geo, p.elem_E, p.conn, p.consistent, p.x, p.lambda, p.g_lambda, b, e, &d, gf);
    const bool bad = p.status[b] != 0;
    p.gI_direct[i] = bad ? __builtin_nan("") : d;
    for (int k = 0; k < 6; ++k) p.g_forces[i * 6 + k] = bad ? __builtin_nan("") : gf[k];
  });
}

struct FrameBucklingRitzArgs {
  const double* X; const double* SX;     // [B,P,Nn,3]
  double* R; double* Q;                  // [B,P,Nn,3]  R: read as S Q of the iteration before, written as the next one's
  double* mu; double* lambda; double* change;   // [B,P]  mu: read as the iteration before's
  const int32_t* row_status;             // [B,P]
  int32_t* status;                       // [B]
};

// one wavefront per frame, as frame_modes_ritz_kernel: partial sums, the fixed butterfly, the small part on every lane, the update
template <int P>
__global__ __launch_bounds__(256) void frame_buckling_ritz_kernel(int B, int n_nodes, const FrameBucklingRitzArgs a) {
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const long n = 3L * n_nodes, base = b * P * n;
  const double *x = a.X + base, *sx = a.SX + base;
  double *r = a.R + base, *q = a.Q + base;
  int st = 0;
  for (int j = 0; j < P; ++j) st |= a.row_status[b * P + j] != 0;
  double Z[P * P], mu[P], lam[P], change[P];
  if (st == 0) {
    double acc[FmRitz<P>::NACC];
    fm_ritz_partials<P>(n, x, sx, r, lane, acc);
#pragma unroll
    for (int k = 0; k < FmRitz<P>::NACC; ++k)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    double prev[P];
#pragma unroll
    for (int j = 0; j < P; ++j) prev[j] = a.mu[b * P + j];
    int sweeps;
    st = fb_ritz_small<P>(acc, prev, Z, mu, lam, change, &sweeps);
  }
  if (st != 0) {      // NaN for this frame alone; R stays, so the next iteration fails the same way with the same status
    const double nan = __builtin_nan("");
    for (long t = lane; t < P * n; t += 64) q[t] = nan;
#pragma unroll
    for (int j = 0; j < P; ++j) mu[j] = lam[j] = change[j] = nan;
  } else {
    fm_ritz_update<P>(n, x, sx, Z, lane, q, r);
  }
  if (lane < P) {
    double u = mu[0], l = lam[0], c = change[0];
#pragma unroll
    for (int j = 1; j < P; ++j)
      if (lane == j) { u = mu[j]; l = lam[j]; c = change[j]; }
    a.mu[b * P + lane] = u;
    a.lambda[b * P + lane] = l;
    a.change[b * P + lane] = c;
  }
  if (lane == 0) a.status[b] = st;
}

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

extern "C" int ops_frame_mass_apply_f64(int R, int rows_per_frame, int n_nodes, int n_elems, const double* elem_geo,
                                        const int32_t* conn, const int32_t* node_elem_ptr, const int32_t* node_elem_idx,
                                        const double* elem_mass, int consistent, const double* nodal_mass, long nodal_bstride,
                                        const double* x, double* y, void* stream) {
  if (R < 0 || rows_per_frame < 1 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (!stride_ok(nodal_bstride, 3L * n_nodes)) return OPS_AMD_ERR_INVALID_ARG;
  if (R == 0) return OPS_AMD_OK;
  if (!elem_geo || !conn || !node_elem_ptr || !node_elem_idx || !elem_mass || !x || !y) return OPS_AMD_ERR_INVALID_ARG;
  FrameModeParams p{};
  p.B = R; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.conn = conn; p.node_elem_ptr = node_elem_ptr; p.node_elem_idx = node_elem_idx;
  p.elem_mass = elem_mass; p.consistent = consistent != 0; p.nodal_mass = nodal_mass; p.nodal_bstride = nodal_bstride;
  p.rows_per_frame = rows_per_frame; p.x = x; p.y = y;
  return frame_stream_launch(frame_mass_apply_kernel, p, (long)R * n_nodes, stream);
}

extern "C" int ops_frame_modes_ritz_f64(int B, int p, int n_nodes, const double* X, const double* MX, double* R, double* Q,
                                        double* lambda, double* change, const int32_t* row_status, int32_t* status,
                                        void* stream) {
  if (B < 0 || p < 1 || p > FM_MAX_VECTORS || n_nodes < 2) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!X || !MX || !R || !Q || !lambda || !change || !row_status || !status) return OPS_AMD_ERR_INVALID_ARG;
  const FrameRitzArgs a{X, MX, R, Q, lambda, change, row_status, status};
  void (*kernel)(int, int, const FrameRitzArgs) =
      p == 1 ? frame_modes_ritz_kernel<1> : p == 2 ? frame_modes_ritz_kernel<2> : p == 3 ? frame_modes_ritz_kernel<3>
      : p == 4 ? frame_modes_ritz_kernel<4> : p == 5 ? frame_modes_ritz_kernel<5> : p == 6 ? frame_modes_ritz_kernel<6>
      : p == 7 ? frame_modes_ritz_kernel<7> : frame_modes_ritz_kernel<8>;
  return launch_wave_rows(kernel, B, stream, B, n_nodes, a);
}

extern "C" int ops_frame_modes_grad_f64(int B, int m, int p, int n_nodes, int n_elems, const double* elem_geo,
                                        const double* elem_E, const int32_t* conn, const double* phi, const double* g_lambda,
                                        const int32_t* status, double* gI, void* stream) {
  if (B < 0 || p < 1 || p > FM_MAX_VECTORS || m < 1 || m > p || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_E || !conn || !phi || !g_lambda || !status || !gI) return OPS_AMD_ERR_INVALID_ARG;
  FrameModeParams q{};
  q.B = B; q.Nn = n_nodes; q.Ne = n_elems;
  q.elem_geo = elem_geo; q.elem_E = elem_E; q.conn = conn;
  q.m = m; q.p = p; q.x = phi; q.g_lambda = g_lambda; q.status = status; q.gI = gI;
  return frame_stream_launch(frame_modes_grad_kernel, q, (long)B * n_elems, stream);
}

extern "C" int ops_frame_geom_apply_f64(int R, int rows_per_frame, int n_nodes, int n_elems, const double* elem_geo,
                                        const int32_t* conn, const int32_t* node_elem_ptr, const int32_t* node_elem_idx,
                                        const double* forces, int consistent, const double* x, double* y, void* stream) {
  if (R < 0 || rows_per_frame < 1 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (R == 0) return OPS_AMD_OK;
  if (!elem_geo || !conn || !node_elem_ptr || !node_elem_idx || !forces || !x || !y) return OPS_AMD_ERR_INVALID_ARG;
  FrameBucklingParams p{};
  p.B = R; p.Nn = n_nodes; p.Ne = n_elems;
  p.elem_geo = elem_geo; p.conn = conn; p.node_elem_ptr = node_elem_ptr; p.node_elem_idx = node_elem_idx;
  p.forces = forces; p.consistent = consistent != 0; p.rows_per_frame = rows_per_frame; p.x = x; p.y = y;
  return frame_stream_launch(frame_geom_apply_kernel, p, (long)R * n_nodes, stream);
}

extern "C" int ops_frame_buckling_ritz_f64(int B, int p, int n_nodes, const double* X, const double* SX, double* R, double* Q,
                                           double* mu, double* lambda, double* change, const int32_t* row_status,
                                           int32_t* status, void* stream) {
  if (B < 0 || p < 1 || p > FM_MAX_VECTORS || n_nodes < 2) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!X || !SX || !R || !Q || !mu || !lambda || !change || !row_status || !status) return OPS_AMD_ERR_INVALID_ARG;
  const FrameBucklingRitzArgs a{X, SX, R, Q, mu, lambda, change, row_status, status};
  void (*kernel)(int, int, const FrameBucklingRitzArgs) =
      p == 1 ? frame_buckling_ritz_kernel<1> : p == 2 ? frame_buckling_ritz_kernel<2> : p == 3 ? frame_buckling_ritz_kernel<3>
      : p == 4 ? frame_buckling_ritz_kernel<4> : p == 5 ? frame_buckling_ritz_kernel<5> : p == 6 ? frame_buckling_ritz_kernel<6>
      : p == 7 ? frame_buckling_ritz_kernel<7> : frame_buckling_ritz_kernel<8>;
  return launch_wave_rows(kernel, B, stream, B, n_nodes, a);
}

extern "C" int ops_frame_buckling_grad_f64(int B, int m, int p, int n_nodes, int n_elems, const double* elem_geo,
                                           const double* elem_E, const int32_t* conn, int consistent, const double* phi,
                                           const double* lambda, const double* g_lambda, const int32_t* status,
                                           double* gI_direct, double* g_forces, void* stream) {
  if (B < 0 || p < 1 || p > FM_MAX_VECTORS || m < 1 || m > p || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (B == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_E || !conn || !phi || !lambda || !g_lambda || !status || !gI_direct || !g_forces)
    return OPS_AMD_ERR_INVALID_ARG;
  FrameBucklingParams q{};
  q.B = B; q.Nn = n_nodes; q.Ne = n_elems;
  q.elem_geo = elem_geo; q.elem_E = elem_E; q.conn = conn; q.consistent = consistent != 0;
  q.m = m; q.p = p; q.x = phi; q.lambda = lambda; q.g_lambda = g_lambda; q.status = status;
  q.gI_direct = gI_direct; q.g_forces = g_forces;
  return frame_stream_launch(frame_buckling_grad_kernel, q, (long)B * n_elems, stream);
}

// ---- the natural-frequency floor of design sizing (C ABI: include/openpystruct_amd_frame_frequency.h) ----
// Behind every other kernel of this file: their order in the code object stays what it was.
namespace opsamd {

struct FrameFloorParams : FrameStreamTopo {     // B: the designs
  int m, p;
  const double* phi;               // [G,p,Nn,3]
  const double* lambda;            // [G,p]
  const int32_t* status;           // [G]
  const double* floor;             // [1] or [G]
  long floor_stride;
  double alpha;
  const uint8_t* active;           // [G] or NULL
  double* grad_extra;              // [G,Ne]
  double* penalty;                 // [G]
};

// one thread per (design, element), as frame_modes_grad_kernel; the m coefficients live in registers; no LDS, no atomics
__global__ __launch_bounds__(FRAME_STREAM_BLOCK) void frame_frequency_floor_kernel(const FrameFloorParams p) {
  frame_stream_rows(p.B, p.Ne, [&](long i, long g, int e) {
    if (p.active && !p.active[g]) return;
    double pen;
    const double v = fm_elem_floor(p.m, p.p, p.Nn, p.elem_geo, p.elem_E, p.conn, p.phi, p.lambda, p.floor[g * p.floor_stride],
                                   p.alpha, g, e, &pen);
    const bool bad = p.status[g] != 0;
    p.grad_extra[i] = bad ? __builtin_nan("") : v;
    if (e == 0) p.penalty[g] = bad ? __builtin_nan("") : pen;
  });
}

}  // namespace opsamd

extern "C" int ops_frame_frequency_floor_f64(int G, int m, int p, int n_nodes, int n_elems, const double* elem_geo,
                                             const double* elem_E, const int32_t* conn, const double* phi, const double* lambda,
                                             const int32_t* status, const double* floor, long floor_stride, double alpha,
                                             const uint8_t* active, double* grad_extra, double* penalty, void* stream) {
  if (G < 0 || p < 1 || p > FM_MAX_VECTORS || m < 1 || m > p || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (!(alpha >= 0.0) || (floor_stride != 0 && floor_stride != 1)) return OPS_AMD_ERR_INVALID_ARG;
  if (G == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_E || !conn || !phi || !lambda || !status || !floor || !grad_extra || !penalty) return OPS_AMD_ERR_INVALID_ARG;
  FrameFloorParams q{};
  q.B = G; q.Nn = n_nodes; q.Ne = n_elems;
  q.elem_geo = elem_geo; q.elem_E = elem_E; q.conn = conn;
  q.m = m; q.p = p; q.phi = phi; q.lambda = lambda; q.status = status;
  q.floor = floor; q.floor_stride = floor_stride; q.alpha = alpha; q.active = active;
  q.grad_extra = grad_extra; q.penalty = penalty;
  return frame_stream_launch(frame_frequency_floor_kernel, q, (long)G * n_elems, stream);
}
