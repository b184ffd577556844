// The sizing objective of PREDICTED designs for gfx950 (MI355X): the two streaming launches that bracket the unchanged solve and
// gradient launches.  C ABI: include/openpystruct_amd_design_loss.h.  Arithmetic: design_loss_math.hpp.
//
//   design_prep_kernel     one thread per (sample, node): the inertia of element n from the standardised prediction (inverse scaler,
//                          floor) widened into the sample's C beam rows, and node n of the C load vectors gathered by the sample's row
//   design_finish_kernel   sizing_multicase_kernel's mapping -- one 64-lane wavefront per sample, four samples per 256-thread block,
//                          lane e handles elements e, e + 64, ... (Ne <= 512), the elements per lane a template parameter -- walking
//                          the sample's cases in index order in float64 with the next case's rows loading while this case's two sums
//                          are reduced: the objective, its gradient, the chain to the predictions, the sample's share of the value
//   design_value_kernel    one workgroup adds the B shares in a fixed order: the value
// No atomics, no LDS outside the value's workgroup sum, nothing waits on another workgroup, plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openpystruct_amd_design_loss.h"
#include "design_loss_math.hpp"
#include "lane_common.hpp"
#include "sizing_math.hpp"

namespace opsamd {

constexpr int kDesignMaxCases = 64;

// the row of Fy_src / ref that sample b reads: rows[b] wrapped into [0, G)
__device__ __forceinline__ long design_row(const ops_design_loss_args& a, long b) {
  if (!a.rows) return b;          // (the host refused G < B)
  long r = (long)(a.rows[b] % (int64_t)a.G);
  return r < 0 ? r + a.G : r;
}

__global__ __launch_bounds__(256) void design_prep_kernel(const ops_design_loss_args a) {
  const int N = a.Ne + 1;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.B * N) return;
  const long b = idx / N;
  const int n = (int)(idx - b * N);
  const long row0 = b * a.C;
  if (n < a.Ne) {
    const float raw = design_raw(design_pred(a.preds, a.preds_bf16, b * a.ldp + n), a.I_scale[n], a.I_mean[n]);
    const double I = design_inertia(raw, a.I_min);
    for (int c = 0; c < a.C; ++c) a.I_rows[(row0 + c) * a.Ne + n] = I;
  }
  const long src0 = design_row(a, b) * a.C;
  for (int c = 0; c < a.C; ++c) a.Fy_rows[(row0 + c) * N + n] = a.Fy_src[(src0 + c) * N + n];
}

// what one load case contributes, as one wavefront holds it between its loads and its arithmetic
template <int K>
struct DesignRowRegs {
  double V[K], M[K], g[K];
  double extra, w;
};

// issue the loads of beam row `row` (nothing waits here)
template <int K, bool GRAD>
__device__ __forceinline__ void design_load_row(int lane, long row, int c, const ops_design_loss_args& a, DesignRowRegs<K>& q) {
  q.extra = a.loss_extra ? a.loss_extra[row] : 0.0;
  q.w = a.weights ? a.weights[c] : 1.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    const long o = row * a.Ne + (e < a.Ne ? e : 0);
    q.V[k] = a.V[o];
    q.M[k] = a.M[o];
    if constexpr (GRAD) q.g[k] = a.grad[o];
  }
}

template <int K>
__global__ __launch_bounds__(256) void design_finish_kernel(const ops_design_loss_args a, const DesignConsts kc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + wave;
  if (b >= a.B) return;           // wave-uniform
  const int C = a.C, Ne = a.Ne;
  const bool sum = a.aggregate == 0;
  const long row0 = b * C;
  DesignRowRegs<K> cur, nxt;
  if (sum) design_load_row<K, true>(lane, row0, 0, a, cur); else design_load_row<K, false>(lane, row0, 0, a, cur);

  // a failed row of either launch in the middle (C <= 64: one row per lane)
  int flag = 0;
  if (lane < C) {
    if (a.status_solve) flag |= a.status_solve[row0 + lane] != 0;
    if (a.status_grad) flag |= a.status_grad[row0 + lane] != 0;
  }
  // the design's own terms: the two denominators of every element, once for all cases
  double I[K], den_b[K], den_s[K];
  double lsum_I = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    I[k] = 0.0; den_b[k] = 1.0; den_s[k] = 1.0;
    if (e < Ne) {
      I[k] = a.I_rows[row0 * Ne + e];
      den_b[k] = design_den_bend(kc, I[k]);
      den_s[k] = design_den_shear(kc, I[k]);
      lsum_I += I[k];
      flag |= I[k] != I[k];
    }
  }
  const double sum_I = wave_sum(lsum_I);
  DesignWalk walk;
  walk.start(sum_I);
  double gacc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) gacc[k] = 0.0;
  for (int c = 0; c < C; ++c) {
    if (c + 1 < C) {
      if (sum) design_load_row<K, true>(lane, row0 + c + 1, c + 1, a, nxt); else design_load_row<K, false>(lane, row0 + c + 1, c + 1, a, nxt);
    }
    double lsum_b = 0.0, lsum_s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (lane + 64 * k < Ne) design_case_terms(cur.M[k], cur.V[k], den_b[k], den_s[k], lsum_b, lsum_s);
    const double sb = wave_sum(lsum_b), ss = wave_sum(lsum_s);
    const double P = walk.add_case(kc, c, sb, ss, a.loss_extra != nullptr, cur.extra, a.weights != nullptr, cur.w, sum);
    if (sum) {
#pragma unroll
      for (int k = 0; k < K; ++k) gacc[k] = design_grad_acc(gacc[k], cur.w, cur.g[k]);
    }
    if (a.case_penalty && lane == 0) a.case_penalty[row0 + c] = P;
    if (c + 1 < C) cur = nxt;
  }
  const bool bad = wave_sum(flag) != 0 || walk.bad;
  const double nan = __builtin_nan("");
  const double L = bad ? nan : walk.finish(sum_I, sum);
  const long src = design_row(a, b);
  const double ref = a.ref ? a.ref[src] : 1.0;
  const double coef = design_coef(a.weight, a.B, ref);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    if (e < Ne) {
      double g = sum ? design_grad_sum(gacc[k], walk.wsum) : a.grad[(row0 + walk.gov) * Ne + e];   // the governing row, read now that it is known
      if (bad) g = nan;
      if (a.gI) a.gI[b * Ne + e] = g;
      if (a.dpreds) {
        const long o = b * a.ldp + e;
        const float scale = a.I_scale[e];
        const float raw = design_raw(design_pred(a.preds, a.preds_bf16, o), scale, a.I_mean[e]);
        const double d = bad ? nan : design_dpred(coef, g, scale, design_live(raw, a.I_min));
        if (a.preds_bf16) ((uint16_t*)a.dpreds)[o] = design_f32_to_bf16((float)d);
        else ((float*)a.dpreds)[o] = (float)d;
      }
    }
  }
  if (lane == 0) {
    if (a.sample_loss) a.sample_loss[b] = L;
    if (a.governing) a.governing[b] = walk.gov;
    if (a.part) a.part[b] = L / ref;
  }
}

// one workgroup: thread t adds shares t, t + 256, ... in index order, then the workgroup's 256 sums in a fixed order
__global__ __launch_bounds__(256) void design_value_kernel(const ops_design_loss_args a) {
  __shared__ double s_red[4];
  double acc[1] = {0.0};
  for (long b = threadIdx.x; b < a.B; b += 256) acc[0] += a.part[b];
  block_sum<4, false>(acc, s_red);
  if (threadIdx.x == 0) {
    a.value[0] = (float)((double)a.weight * (acc[0] / (double)a.B));
    if (a.value_sum) a.value_sum[0] += a.value[0];
  }
}

// what both entry points refuse
static int design_args(const ops_design_loss_args* a) {
  if (!a || a->B < 0 || a->C < 1 || a->Ne < 1 || a->G < 0) return OPS_AMD_ERR_INVALID_ARG;
  if (a->aggregate != 0 && a->aggregate != 1) return OPS_AMD_ERR_INVALID_ARG;
  if (a->aggregate == 1 && a->weights) return OPS_AMD_ERR_INVALID_ARG;
  if (a->Ne > kSizingMaxElems || a->C > kDesignMaxCases) return OPS_AMD_ERR_UNSUPPORTED;
  if (a->preds && a->ldp < a->Ne) return OPS_AMD_ERR_INVALID_ARG;
  if ((a->rows || a->ref || a->Fy_src) && a->G < 1 && a->B > 0) return OPS_AMD_ERR_INVALID_ARG;
  if (!a->rows && (a->ref || a->Fy_src) && a->G < a->B) return OPS_AMD_ERR_INVALID_ARG;
  return OPS_AMD_OK;
}

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_design_loss_max_cases(void) { return kDesignMaxCases; }
extern "C" size_t ops_design_loss_part_doubles(int B) { return B > 0 ? (size_t)B : 0; }

extern "C" int ops_design_loss_prep(const ops_design_loss_args* q, void* stream) {
  const int rc = design_args(q);
  if (rc != OPS_AMD_OK) return rc;
  if (q->B == 0) return OPS_AMD_OK;
  if (!q->preds || !q->I_scale || !q->I_mean || !q->I_rows || !q->Fy_src || !q->Fy_rows) return OPS_AMD_ERR_INVALID_ARG;
  const long n = (long)q->B * (q->Ne + 1);
  hipLaunchKernelGGL(design_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *q);
  return launch_status();
}

extern "C" int ops_design_loss_finish(const ops_design_loss_args* q, const ops_sizing_params* hp, void* stream) {
  const int rc = design_args(q);
  if (rc != OPS_AMD_OK) return rc;
  if (!hp) return OPS_AMD_ERR_INVALID_ARG;
  if (q->alpha_deflection < 0.0 || q->alpha_deflection != q->alpha_deflection) return OPS_AMD_ERR_INVALID_ARG;
  if (q->alpha_deflection > 0.0 && (!(q->deflection_limit > 0.0) || !q->loss_extra)) return OPS_AMD_ERR_INVALID_ARG;
  if (q->B == 0) return OPS_AMD_OK;
  if (!q->I_rows || !q->V || !q->M || !q->grad) return OPS_AMD_ERR_INVALID_ARG;
  if (q->dpreds && (!q->preds || !q->I_scale || !q->I_mean)) return OPS_AMD_ERR_INVALID_ARG;
  if ((q->value || q->value_sum) && (!q->value || !q->part)) return OPS_AMD_ERR_INVALID_ARG;
  const DesignConsts kc{hp->alpha_moment, hp->alpha_shear, 2.0 * hp->E, hp->bend_eps, hp->G * hp->area_coef};
  const unsigned grid = (unsigned)((q->B + 3) / 4);
  hipStream_t s = (hipStream_t)stream;
  if (q->Ne <= 64) hipLaunchKernelGGL(design_finish_kernel<1>, dim3(grid), dim3(256), 0, s, *q, kc);
  else if (q->Ne <= 128) hipLaunchKernelGGL(design_finish_kernel<2>, dim3(grid), dim3(256), 0, s, *q, kc);
  else if (q->Ne <= 256) hipLaunchKernelGGL(design_finish_kernel<4>, dim3(grid), dim3(256), 0, s, *q, kc);
  else hipLaunchKernelGGL(design_finish_kernel<8>, dim3(grid), dim3(256), 0, s, *q, kc);
  if (q->value) hipLaunchKernelGGL(design_value_kernel, dim3(1), dim3(256), 0, s, *q);
  return launch_status();
}
