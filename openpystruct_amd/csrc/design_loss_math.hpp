// The per-lane arithmetic of the design-objective term (csrc/design_loss.hip; contract: include/openpystruct_amd_design_loss.h;
// DESIGN.md §9m).  Like beam_math.hpp and sizing_grad_math.hpp this header is compiled by hipcc into the kernels and by g++ into the
// lane-level emulator under tests/ (tests/csrc/emul_design_loss.cpp): no I/O, no cross-lane traffic -- the kernel reduces the two
// partial sums of a case over its wave between `design_case_terms` and `DesignWalk::add_case`, the emulator over an array.
// Built with -ffp-contract=off on both sides: equal expressions round equally.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define DESIGN_HD __host__ __device__ __forceinline__
#else
#define DESIGN_HD inline
#endif

namespace opsamd {

// ---- the predictions' side -------------------------------------------------------------------------------------------------------
DESIGN_HD float design_bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
DESIGN_HD uint32_t design_f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
DESIGN_HD float design_bf16_to_f32(uint16_t h) { return design_bits_f32((uint32_t)h << 16); }
// float -> bfloat16, round to nearest even; NaN stays NaN (lane_common.hpp f32_to_bf16, here for the host as well)
DESIGN_HD uint16_t design_f32_to_bf16(float f) {
  uint32_t u = design_f32_bits(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
DESIGN_HD float design_pred(const void* preds, int bf16, long o) {
  return bf16 ? design_bf16_to_f32(((const uint16_t*)preds)[o]) : ((const float*)preds)[o];
}
// StandardScalerT.inverse_transform in float32: the product rounded, then the sum rounded
DESIGN_HD float design_raw(float p, float scale, float mean) {
  const float ps = p * scale;
  return ps + mean;
}
// clamp_min's semantics: only raw < I_min is clamped, a NaN stays NaN
DESIGN_HD double design_inertia(float raw, float I_min) { return (double)(raw < I_min ? I_min : raw); }
// the clamp's derivative as the term chains it: 1 where the prediction is above the floor
DESIGN_HD bool design_live(float raw, float I_min) { return raw > I_min; }

// ---- the objective's side --------------------------------------------------------------------------------------------------------
struct DesignConsts {
  double aM, aV, twoE, bend_eps, Gk;      // alpha_moment, alpha_shear, 2 E, bend_eps, G * area_coef
};
// the design's own part of every case's two quotients
DESIGN_HD double design_den_bend(const DesignConsts& k, double I) { return k.twoE * I + k.bend_eps; }
DESIGN_HD double design_den_shear(const DesignConsts& k, double I) { return k.Gk * sqrt(I); }
// what one element of one case adds to its lane's two partial sums
DESIGN_HD void design_case_terms(double M, double V, double den_b, double den_s, double& lsum_b, double& lsum_s) {
  lsum_b += (M * M) / den_b;
  lsum_s += (V * V) / den_s;
}

// The walk over a sample's cases, wave-uniform: every lane holds the same state
struct DesignWalk {
  double loss;        // sum_e I_e, then + sum_c w_c P_c (aggregate 0)
  double top;         // the largest score so far
  double wsum;        // sum_c w_c
  int gov;            // the lowest index that attains `top`
  bool bad;           // a NaN penalty
  DESIGN_HD void start(double sum_I) { loss = sum_I; top = 0.0; wsum = 0.0; gov = 0; bad = sum_I != sum_I; }
  // sb, ss: the case's two sums over the elements.  Returns P_c
  DESIGN_HD double add_case(const DesignConsts& k, int c, double sb, double ss, bool has_extra, double extra, bool has_w, double w,
                            bool sum) {
    double P = k.aM * sb + k.aV * ss;
    if (has_extra) P += extra;
    double score = P;
    if (sum) {
      if (has_w) score = w * P;
      loss += score;
      wsum += w;
    }
    if (P != P) bad = true;
    if (c == 0 || score > top) { top = score; gov = c; }      // ties keep the lowest index
    return P;
  }
  DESIGN_HD double finish(double sum_I, bool sum) const { return sum ? loss : sum_I + top; }
};
// the weighted-sum gradient of one element: acc += w g per case in index order, then the weight term's 1 counted once
DESIGN_HD double design_grad_acc(double acc, double w, double g) { return acc + w * g; }
DESIGN_HD double design_grad_sum(double acc, double wsum) { return acc - (wsum - 1.0); }
// weight / (B ref_b)
DESIGN_HD double design_coef(float weight, int B, double ref) { return (double)weight / ((double)B * ref); }
// d value / d preds[b, e] in float64 (rounded once by the store)
DESIGN_HD double design_dpred(double coef, double g, float scale, bool live) { return live ? (coef * g) * (double)scale : 0.0; }

}  // namespace opsamd
