// One optimiser epoch of ONE design under C load cases, executed by a whole 64-lane wavefront (csrc/sizing_multicase.hip; contract:
// include/openpystruct_amd_sizing_multicase.h).  The design's state is a case's of sizing_math.hpp (SizingArgs, CaseRegs, load_case)
// and the Adam / clamp / early-stop arithmetic below is step_case's, statement for statement: with C == 1, the weighted sum and no
// weights every field comes out as step_case<K, ..., GivenGrad> writes it (the library is built with -ffp-contract=off, so equal
// expressions round equally).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_common.hpp"
#include "sizing_math.hpp"

namespace opsamd {

struct MultiCaseArgs {
  SizingArgs s;                      // the design's state [G, ...]; s.I64 == the C rows per design (I64_rows), V32 / M32 / I_last unused
  int C, aggregate;                  // 0: weighted sum, 1: worst case
  const double* V; const double* M; const double* grad;   // [G*C, Ne]
  const double* loss_extra;          // [G*C] or NULL
  const double* weights;             // [C] or NULL (all 1)
  uint8_t* active_rows;              // [G*C]
  float* case_penalty;               // [G*C] or NULL
  int32_t* governing;                // [G] or NULL
};

// what one load case contributes, as one wavefront holds it between its loads and its arithmetic
template <int K>
struct CaseRowRegs {
  double V[K], M[K], g[K];
  double extra, w;
};

// issue the loads of beam row `row` (nothing waits here: the next case's loads fly while this case's sums are formed)
template <int K, bool GRAD>
__device__ __forceinline__ void load_case_row(int lane, long row, int c, int Ne, const MultiCaseArgs& a, CaseRowRegs<K>& q) {
  q.extra = a.loss_extra ? a.loss_extra[row] : 0.0;
  q.w = a.weights ? a.weights[c] : 1.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    const long o = row * Ne + (e < Ne ? e : 0);
    q.V[k] = a.V[o];
    q.M[k] = a.M[o];
    if constexpr (GRAD) q.g[k] = a.grad[o];
  }
}

template <int K>
__device__ __forceinline__ void multicase_design(int lane, long g, int Ne, const MultiCaseArgs& a) {
  const SizingArgs& s = a.s;
  const ops_sizing_params& hp = s.hp;
  const int C = a.C;
  const bool sum = a.aggregate == 0;
  const long row0 = g * C;
  CaseRegs<K> r;
  load_case<K>(lane, g, Ne, s, r);
  CaseRowRegs<K> cur, nxt;
  if (sum) load_case_row<K, true>(lane, row0, 0, Ne, a, cur); else load_case_row<K, false>(lane, row0, 0, Ne, a, cur);

  const int t = r.t;
  const float twoE = (float)(2.0 * hp.E), Gf = (float)hp.G;
  float step_size, bc2s;
  if (s.schedule) {
    step_size = s.schedule[2 * t];
    bc2s = s.schedule[2 * t + 1];
  } else {
    const float lr_t = (float)(hp.lr * pow(hp.gamma, (double)t));
    const float bc1 = (float)(1.0 - pow(hp.beta1, (double)(t + 1)));
    bc2s = (float)sqrt(1.0 - pow(hp.beta2, (double)(t + 1)));
    step_size = lr_t / bc1;
  }
  const float omb1 = (float)(1.0 - hp.beta1), omb2 = (float)(1.0 - hp.beta2);

  // the design's own terms: the two denominators of every element, once for all cases
  float den_b[K], den_s[K];
  float lsum_I = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    den_b[k] = 1.f;
    den_s[k] = 1.f;
    if (e < Ne) {
      const float Ie = r.I[k];
      den_b[k] = twoE * Ie + (float)hp.bend_eps;
      den_s[k] = Gf * ((float)hp.area_coef * sqrtf(Ie));
      lsum_I += Ie;
    }
  }
  const float sum_I = wave_sum(lsum_I);

  // the walk over the cases: two partial sums per lane and case, the float64 gradient accumulator, the running maximum
  float loss = sum_I, top = 0.f;
  int gov = 0;
  double wsum = 0.0;
  double gacc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) gacc[k] = 0.0;
  for (int c = 0; c < C; ++c) {
    if (c + 1 < C) {
      if (sum) load_case_row<K, true>(lane, row0 + c + 1, c + 1, Ne, a, nxt); else load_case_row<K, false>(lane, row0 + c + 1, c + 1, Ne, a, nxt);
    }
    float lsum_b = 0.f, lsum_s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = lane + 64 * k;
      if (e < Ne) {
        const float m = (float)cur.M[k], v = (float)cur.V[k];
        lsum_b += (m * m) / den_b[k];
        lsum_s += (v * v) / den_s[k];
      }
    }
    const float sb = wave_sum(lsum_b), ss = wave_sum(lsum_s);
    float P = (float)hp.alpha_moment * sb + (float)hp.alpha_shear * ss;
    if (a.loss_extra) P += (float)cur.extra;
    float score = P;                              // what the governing case is the largest of
    if (sum) {
      if (a.weights) {
        score = (float)cur.w * P;
        loss += score;
      } else if (c == 0) {                        // step_case's order: ((sum I + a_M b) + a_S s) + extra
        loss = sum_I + (float)hp.alpha_moment * sb + (float)hp.alpha_shear * ss;
        if (a.loss_extra) loss += (float)cur.extra;
      } else {
        loss += P;
      }
      wsum += cur.w;
#pragma unroll
      for (int k = 0; k < K; ++k) gacc[k] += cur.w * cur.g[k];
    }
    if (c == 0 || score > top) { top = score; gov = c; }      // ties keep the lowest index
    if (a.case_penalty && lane == 0) a.case_penalty[row0 + c] = P;
    if (c + 1 < C) cur = nxt;
  }
  float gf[K];
  if (sum) {
    const double once = wsum - 1.0;               // every row of grad carries the weight term's 1
#pragma unroll
    for (int k = 0; k < K; ++k) gf[k] = (float)(gacc[k] - once);
  } else {
    loss = sum_I + top;
#pragma unroll
    for (int k = 0; k < K; ++k) {                 // the governing row, read now that it is known
      const int e = lane + 64 * k;
      gf[k] = (float)a.grad[(row0 + gov) * Ne + (e < Ne ? e : 0)];
    }
  }

  // Adam, clamp (step_case)
  float Inew[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    Inew[k] = 0.f;
    if (e < Ne) {
      const long o = g * Ne + e;
      const float Ie = r.I[k];
      const float gk = gf[k];
      const float ea = (float)hp.beta1 * r.m[k] + omb1 * gk;
      const float es = (float)hp.beta2 * r.v[k] + omb2 * gk * gk;
      s.exp_avg[o] = ea;
      s.exp_avg_sq[o] = es;
      const float denom = sqrtf(es) / bc2s + (float)hp.adam_eps;
      float In = Ie - step_size * (ea / denom);
      In = fmaxf(In, (float)hp.clamp_min);
      s.I[o] = In;
      Inew[k] = In;
    }
  }
  // early stopping, one decision per design
  float best = r.best;
  int cnt = r.cnt;
  if (loss < best - (float)hp.tolerance) { best = loss; cnt = 0; } else { cnt += 1; }
  const bool stop = (cnt >= hp.patience) || (t + 1 >= hp.max_epochs);
  if (!stop) {
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = lane + 64 * k;
        if (e < Ne) s.I64[(row0 + c) * Ne + e] = (double)Inew[k];   // what the next solve and gradient launches read, C times
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) a.active_rows[row0 + c] = 0;
  }
  if (lane == 0) {
    s.best_loss[g] = best;
    s.patience_cnt[g] = cnt;
    s.epochs_run[g] = t + 1;
    s.last_loss[g] = loss;
    if (a.governing) a.governing[g] = gov;
    if (stop) s.active[g] = 0;
  }
}

}  // namespace opsamd
