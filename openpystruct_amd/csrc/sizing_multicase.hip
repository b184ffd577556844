// Multi-load-case beam sizing for gfx950 (MI355X): the optimiser step of G designs, each under C load cases, in ONE launch.
// C ABI: include/openpystruct_amd_sizing_multicase.h.  Arithmetic: sizing_multicase_math.hpp over sizing_math.hpp.  Design: DESIGN.md §9j.
//
// The solve and the gradient kernels run unchanged on the G*C beam rows (design-major); this kernel ties the C rows of a design
// together: one set of inertias and one Adam state, the per-case penalties aggregated (weighted sum or worst case), one early-stop
// decision, and the widened inertias written back into all C rows for the next epoch's solve.
//
// Mapping: sizing_step_kernel's -- one 64-lane wavefront per design, four designs per 256-thread block, lane e handles elements
// e, e + 64, ... (Ne <= 512) -- with the elements per lane a template parameter (1, 2, 4, 8: at the workload's Ne = 100 a lane
// holds 2 elements per case, not 8 padded ones).  The wave walks the design's cases in index order with the next case's rows
// loading while this case's two sums are reduced; no atomics, no LDS, plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openpystruct_amd_sizing_multicase.h"
#include "sizing_multicase_math.hpp"

namespace opsamd {

constexpr int kMultiCaseMax = 64;

template <int K>
__global__ __launch_bounds__(256) void sizing_multicase_kernel(int G, int Ne, const MultiCaseArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * 4 + wave;
  if (g >= G) return;
  if (!a.s.active[g]) return;   // wave-uniform
  multicase_design<K>(lane, g, Ne, a);
}

}  // namespace opsamd

using namespace opsamd;

extern "C" int ops_beam_sizing_multicase_max_cases(void) { return kMultiCaseMax; }

extern "C" int ops_beam_sizing_step_multicase_f32(int G, int C, int Ne, float* I, double* I64_rows, const double* V, const double* M,
                                                  const double* grad, const double* loss_extra, const double* weights,
                                                  int aggregate, float* exp_avg, float* exp_avg_sq, float* best_loss,
                                                  int32_t* patience_cnt, int32_t* epochs_run, uint8_t* active,
                                                  uint8_t* active_rows, float* last_loss, float* case_penalty, int32_t* governing,
                                                  const ops_sizing_params* hp, const float* schedule, void* stream) {
  if (G < 0 || C < 1 || Ne < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (aggregate != 0 && aggregate != 1) return OPS_AMD_ERR_INVALID_ARG;
  if (aggregate == 1 && weights) return OPS_AMD_ERR_INVALID_ARG;
  if (Ne > kSizingMaxElems || C > kMultiCaseMax) return OPS_AMD_ERR_UNSUPPORTED;
  if (G == 0) return OPS_AMD_OK;
  if (!I || !I64_rows || !V || !M || !grad || !exp_avg || !exp_avg_sq || !best_loss || !patience_cnt || !epochs_run || !active ||
      !active_rows || !last_loss || !hp)
    return OPS_AMD_ERR_INVALID_ARG;
  MultiCaseArgs a{sizing_args(I, exp_avg, exp_avg_sq, best_loss, patience_cnt, epochs_run, active, last_loss, hp),
                  C, aggregate, V, M, grad, loss_extra, weights, active_rows, case_penalty, governing};
  a.s.I64 = I64_rows; a.s.schedule = schedule;
  return sizing_lane_elems(Ne, [&](auto K) { return launch_wave_rows(sizing_multicase_kernel<K>, G, stream, G, Ne, a); });
}
