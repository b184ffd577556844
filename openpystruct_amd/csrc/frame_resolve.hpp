// Batched 2-D frame solve: C right-hand sides per frame on the factor a KEEPING solve left behind.
// (included by frame_solve.hip behind frame_wave.hpp; FrameParams, write_results, fw_* come from there)
//
// The wave-per-frame kernel (frame_wave.hpp) leaves column j of every frame's L in that frame's own workspace slot, at
// [j * W, j * W + kd).  Instantiated with KEEP it also leaves 1 / d_j at j * W + W - 1, and with that the slot is the whole
// factorisation K = L D L^T.  The kernel below does substitution only: ONE WAVEFRONT PER (FRAME, PASS), NR right-hand sides per
// pass, a last pass repeating its last case where C is no multiple of NR (computed, not written).
//
//   * forward: lane (R mod 64) owns row R of the right-hand sides, as in the factorisation: y[r] in a register.  Per column j ONE
//     coalesced load serves the NR right-hand sides -- lane (j + rel) mod 64 reads L[j + rel][j], the pivot row's lane reads
//     1 / d_j in the same instruction -- and then, per right-hand side, exactly fw_step's operations in fw_step's order:
//     z_j = readlane(y), w_j = z_j * rd_j, y = fma(-l, z_j, y).  Columns are loaded eight at a time, one block of eight ahead of
//     use.  Rows enter eight at a time as well: the lanes of the rows a block has finished take rows j0 + 56 .. j0 + 63 from LDS
//     (read one block ahead), where the right-hand sides were parked in equation order at the start.
//   * backward: fw_backward's blocked dot form with the loads of L shared by the NR right-hand sides and its arithmetic, in its
//     order, per right-hand side.
//   * write_results per right-hand side with all-zero element loads (a zeroed [Ne,2] kept in front of the factors), the inertias
//     of the FRAME, into row b * C + c.
//
// A case's results are a function of its frame's factor and its own right-hand side alone: no atomics, nothing shared between
// the right-hand sides of a pass but the loads of L, so B, C, NR and the position do not enter.  Traffic: the factor is read twice
// per pass (2 n W 8 bytes per frame), which is what a pass costs at large batches; LDS: NR (n + 64) doubles per wave.
#pragma once
#include "frame_wave.hpp"

namespace opsamd {

constexpr int FR_CH = 8;      // columns per block of the forward sweep

__host__ __device__ inline size_t fr_lds_doubles(int n, int NR) { return (size_t)NR * (size_t)(n + 64); }

// fw_backward for NR right-hand sides: xs[r * XS + ...], the same loads of L for all of them
template <int W, int NR>
__device__ __forceinline__ void fr_backward(const double* __restrict__ rows, double* __restrict__ xs, int XS, int n, int kd, int lane) {
  constexpr int MF = (W + 7) / 8;
  const int u = lane >> 3, k = lane & 7;
#pragma unroll
  for (int r = 0; r < NR; ++r) xs[r * XS + n + lane] = 0.0;
  fw_fence();
  double fA[MF], bA[7], fB[MF], bB[7];
  auto issue = [&](int jb, double (&f)[MF], double (&bv)[7]) {      // unconditional loads from clamped addresses
    const int ju = jb - u, jc = ju > 0 ? ju : 0;
    const double* col = rows + (size_t)jc * W;
#pragma unroll
    for (int m = 0; m < MF; ++m) f[m] = col[k + 8 * m < W ? k + 8 * m : W - 1];
#pragma unroll
    for (int v = 0; v < 7; ++v) bv[v] = col[u - v - 1 > 0 ? u - v - 1 : 0];
  };
  auto block = [&](int jb, const double (&lf)[MF], const double (&lbv)[7]) {   // (jb < 0: every lane masked, no write)
    const int ju = jb - u, jc = ju > 0 ? ju : 0;
    const int kdj = ju >= 0 ? (kd < n - 1 - ju ? kd : n - 1 - ju) : 0;      // rows of this column below the diagonal
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      double* x_ = xs + r * XS;
      double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
      for (int m = 0; m < MF; ++m) {
        const int rel = k + 1 + 8 * m;
        const bool far = rel <= kdj && (m > 0 || k >= u);
        const double l = far ? lf[m] : 0.0;
        const double x = x_[jc + rel];
        if (m & 1) acc1 = __builtin_fma(l, x, acc1); else acc0 = __builtin_fma(l, x, acc0);
      }
      double s_ = acc0 + acc1;
      s_ += dpp_mov<0xB1>(s_);
      s_ += dpp_mov<0x4E>(s_);
      s_ += dpp_mov<0x141>(s_);
      double t = x_[jc] - s_;
#pragma unroll
      for (int v = 0; v < 7; ++v) {
        const double xv = fw_readlane(t, 8 * v);
        const double l = (v < u && u - v <= kdj) ? lbv[v] : 0.0;
        t = __builtin_fma(-l, xv, t);
      }
      if (k == 0 && ju >= 0) x_[ju] = t;
    }
    fw_fence();
  };
  int jb = n - 1;
  issue(jb, fA, bA);
  for (; jb >= 0; jb -= 16) {
    issue(jb - 8, fB, bB);
    block(jb, fA, bA);
    issue(jb - 16, fA, bA);
    block(jb - 8, fB, bB);
  }
}

template <int W, int NR>
__global__ __launch_bounds__(64) void frame_resolve_kernel(const FrameParams p, int C, int npass, const int32_t* __restrict__ factor_status,
                                                           const double* __restrict__ factors, const FwPlan pl) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const long b = (long)(blockIdx.x / (unsigned)npass);
  const int c0 = (int)(blockIdx.x % (unsigned)npass) * NR;
  const int n = p.n_eq, kd = p.kd, XS = n + 64;
  double* xs = lds;                                         // [NR][n + 64]: right-hand sides, then w, then x, in equation order
  const bool failed = factor_status[b] != 0;                // the whole wave: a failed frame's factor is not read at all
  if (!failed) {
    const double* rows = factors + (size_t)b * fw_frame_doubles(n, kd);
    // the right-hand sides, parked in equation order (0.0 + value: what the factorisation's assembly gives a row without element loads)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = c0 + r < C ? c0 + r : C - 1;
      const double* src = p.loads + b * p.loads_bs + (long)c * p.Nn * 3;
      for (int i = lane; i < XS; i += 64) xs[r * XS + i] = i < n ? 0.0 + src[pl.eq_dof[i]] : 0.0;
    }
    fw_fence();
    double y[NR], yn[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) { y[r] = xs[r * XS + lane]; yn[r] = 0.0; }
    double LA[FR_CH], LB[FR_CH];
    auto issue = [&](int j0, double (&L)[FR_CH]) {          // column j: L[j + rel][j] for the window's lanes, 1 / d_j for every other one
#pragma unroll
      for (int s = 0; s < FR_CH; ++s) {
        const int j = j0 + s, jc = j < n ? j : n - 1, rel = (lane - j) & 63;
        L[s] = rows[(size_t)jc * W + ((rel >= 1 && rel <= kd) ? rel - 1 : W - 1)];
      }
    };
    auto chunk = [&](int j0, const double (&L)[FR_CH]) {    // j0 % 8 == 0
      const int rel0 = (lane - j0) & 63;
      const int nxt = j0 + rel0 + 64 < XS ? j0 + rel0 + 64 : XS - 1;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (j0 > 0 && rel0 >= 64 - FR_CH) y[r] = yn[r];     // rows j0 + 56 .. j0 + 63 enter (first inside the window at step j0 + 1)
        yn[r] = xs[r * XS + nxt];                           // the rows this lane takes at the next block, if it is one of the first eight
      }
#pragma unroll
      for (int s = 0; s < FR_CH; ++s) {
        const int j = j0 + s, rel = (lane - j) & 63;
        const bool inwin = rel >= 1 && rel <= kd && j + rel < n;
        const double rdj = fw_readlane(L[s], j & 63);
        const double l = inwin ? L[s] : 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const double zj = fw_readlane(y[r], j & 63);
          if (rel == 0 && j < n) xs[r * XS + j] = zj * rdj;
          y[r] = __builtin_fma(-l, zj, y[r]);
        }
      }
    };
    issue(0, LA);
    for (int j0 = 0; j0 < n; j0 += 2 * FR_CH) {
      issue(j0 + FR_CH, LB);
      chunk(j0, LA);
      issue(j0 + 2 * FR_CH, LA);
      chunk(j0 + FR_CH, LB);
    }
    fw_fence();
    fr_backward<W, NR>(rows, xs, XS, n, kd, lane);
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int c = c0 + r;
    if (c >= C) break;
    const long row = b * C + c;                             // write_results indexes the outputs and the inertias by one number: the
    FrameParams q = p;                                      // outputs are moved so that frame b's inertias go with row b * C + c
    q.disp = p.disp + (row - b) * (long)p.Nn * 3;
    q.forces = p.forces + (row - b) * (long)p.Ne * 6;
    q.V = p.V + (row - b) * (long)p.Ne;
    q.M = p.M + (row - b) * (long)p.Ne;
    q.status = p.status ? p.status + (row - b) : nullptr;
    write_results(q, b, xs + r * XS, failed, lane, 64);
  }
}

}  // namespace opsamd
