// Lane-level CPU emulation of the two kernels of openpystruct_amd/csrc/design_loss.hip -- TEST CODE ONLY.
//
// Runs the kernels' per-lane arithmetic (design_loss_math.hpp, shared verbatim) lane by lane: 64 lanes per sample, lane l holding
// elements l, l + 64, ..., the wave's butterfly sums replaced by the same butterfly over an array, the walk over the cases in
// index order.  Nothing under openpystruct_amd/ loads it.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../openpystruct_amd/csrc/design_loss_math.hpp"

using namespace opsamd;

namespace {
// wave_sum of lane_common.hpp: after the butterfly every lane holds the same total
double butterfly(const double* lanes) {
  double v[64], n[64];
  for (int i = 0; i < 64; ++i) v[i] = lanes[i];
  for (int s = 32; s >= 1; s >>= 1) {
    for (int i = 0; i < 64; ++i) n[i] = v[i] + v[i ^ s];
    for (int i = 0; i < 64; ++i) v[i] = n[i];
  }
  return v[0];
}
}  // namespace

// ops_design_loss_prep's inertias: I [B, Ne] float64 (one row per sample; the kernel writes it C times)
extern "C" int emul_design_prep(int B, int Ne, const void* preds, int bf16, long ldp, const float* scale, const float* mean,
                                float I_min, double* I) {
  for (long b = 0; b < B; ++b)
    for (int e = 0; e < Ne; ++e)
      I[b * Ne + e] = design_inertia(design_raw(design_pred(preds, bf16, b * ldp + e), scale[e], mean[e]), I_min);
  return 0;
}

// ops_design_loss_finish on host arrays.  consts[5]: alpha_moment, alpha_shear, 2 E, bend_eps, G * area_coef.  I [B, Ne] (row b*C of
// I_rows); V, M, grad [B*C, Ne]; extra [B*C] or NULL; weights [C] or NULL; status [B*C] or NULL (the OR of the two launches');
// preds / dpreds [B, ldp] (both or neither), ref [B] or NULL (already gathered).  share [B] = L_b / ref_b.
extern "C" int emul_design_finish(int B, int C, int Ne, int aggregate, const double* consts, const double* I, const double* V,
                                  const double* M, const double* grad, const double* extra, const double* weights,
                                  const int32_t* status, const void* preds, int bf16, long ldp, const float* scale, const float* mean,
                                  float I_min, float weight, const double* ref, double* sample_loss, double* gI, double* case_penalty,
                                  int32_t* governing, void* dpreds, double* share) {
  if (Ne > 512 || Ne < 1 || C < 1) return -1;
  const DesignConsts kc{consts[0], consts[1], consts[2], consts[3], consts[4]};
  const bool sum = aggregate == 0;
  const int K = (Ne + 63) / 64;
  for (long b = 0; b < B; ++b) {
    const long row0 = b * C;
    int flag = 0;
    if (status)
      for (int c = 0; c < C; ++c) flag |= status[row0 + c] != 0;
    std::vector<double> den_b(64 * K, 1.0), den_s(64 * K, 1.0), gacc(64 * K, 0.0);
    double lanes[64], lanes2[64];
    for (int l = 0; l < 64; ++l) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) {
        const int e = l + 64 * k;
        if (e < Ne) {
          const double Ie = I[b * Ne + e];
          den_b[e] = design_den_bend(kc, Ie);
          den_s[e] = design_den_shear(kc, Ie);
          s += Ie;
          flag |= Ie != Ie;
        }
      }
      lanes[l] = s;
    }
    const double sum_I = butterfly(lanes);
    DesignWalk walk;
    walk.start(sum_I);
    for (int c = 0; c < C; ++c) {
      const long row = row0 + c;
      const double w = weights ? weights[c] : 1.0;
      for (int l = 0; l < 64; ++l) {
        double sb = 0.0, ss = 0.0;
        for (int k = 0; k < K; ++k) {
          const int e = l + 64 * k;
          if (e < Ne) design_case_terms(M[row * Ne + e], V[row * Ne + e], den_b[e], den_s[e], sb, ss);
        }
        lanes[l] = sb;
        lanes2[l] = ss;
      }
      const double P = walk.add_case(kc, c, butterfly(lanes), butterfly(lanes2), extra != nullptr, extra ? extra[row] : 0.0,
                                     weights != nullptr, w, sum);
      if (sum)
        for (int e = 0; e < Ne; ++e) gacc[e] = design_grad_acc(gacc[e], w, grad[row * Ne + e]);
      if (case_penalty) case_penalty[row] = P;
    }
    const bool bad = flag != 0 || walk.bad;
    const double L = bad ? NAN : walk.finish(sum_I, sum);
    const double r = ref ? ref[b] : 1.0;
    const double coef = design_coef(weight, B, r);
    for (int e = 0; e < Ne; ++e) {
      double g = sum ? design_grad_sum(gacc[e], walk.wsum) : grad[(row0 + walk.gov) * Ne + e];
      if (bad) g = NAN;
      if (gI) gI[b * Ne + e] = g;
      if (dpreds) {
        const long o = b * ldp + e;
        const float raw = design_raw(design_pred(preds, bf16, o), scale[e], mean[e]);
        const double d = bad ? NAN : design_dpred(coef, g, scale[e], design_live(raw, I_min));
        if (bf16) ((uint16_t*)dpreds)[o] = design_f32_to_bf16((float)d);
        else ((float*)dpreds)[o] = (float)d;
      }
    }
    if (sample_loss) sample_loss[b] = L;
    if (governing) governing[b] = walk.gov;
    if (share) share[b] = L / r;
  }
  return 0;
}
