/* openpystruct_amd -- C ABI, extension header: the sizing objective of PREDICTED designs as a loss term and a metric.
 *
 * An addition to include/openpystruct_amd.h, include/openpystruct_amd_sizing_grad.h and
 * include/openpystruct_amd_sizing_multicase.h: entry points of the same shared library, the same conventions -- DEVICE pointers
 * owned by the caller, nothing allocated, copied or synchronised inside, work enqueued on `stream` (a hipStream_t passed as
 * void*), return codes OPS_AMD_OK / OPS_AMD_ERR_* -- and no change to any declaration of those headers: OPS_AMD_ABI_VERSION,
 * ops_sizing_params and ops_sizing_objective stay what they are (this header is read before
 * the one that declares ops_sizing_objective, so its two fields travel in the argument struct).
 *
 * B samples, each ONE design of Ne elements under C load cases, carried by C beam rows, sample-major: load case c of sample b is
 * beam row b*C + c.  The term is four launches, the two in the middle unchanged:
 *   ops_design_loss_prep        the designs from the model's standardised predictions, the loads gathered
 *   ops_beam_solve_batched_f64  the response of the B*C rows
 *   ops_beam_sizing_grad_f64    dL/dI of every row through the solve
 *   ops_design_loss_finish      the C rows of a sample tied together: objective, its gradient, the chain to the predictions, the value
 *
 * prep.  For b < B, e < Ne:  raw = (float)preds[b*ldp + e] * I_scale[e] + I_mean[e] in float32, two roundings (preds float32, or
 * bfloat16 with preds_bf16 != 0);  I = raw < I_min ? I_min : raw (a NaN stays NaN), widened to float64 and written into the C
 * rows I_rows[(b*C + c)*Ne + e].  Fy_rows[(b*C + c)*N + n] = Fy_src[(r*C + c)*N + n], N = Ne + 1, r = rows[b] (int64 [B]; NULL:
 * r = b, which needs G >= B) wrapped into [0, G) modulo G: a row outside Fy_src [G, C, N] is never read.
 * Required: preds, I_scale, I_mean, I_rows, Fy_src, Fy_rows; G >= 1; ldp >= Ne.
 *
 * finish.  One 64-lane wavefront per sample, float64 throughout.  I = row b*C of I_rows;
 *   P_c = alpha_moment sum_e M_c,e^2 / (2 E I_e + bend_eps) + alpha_shear sum_e V_c,e^2 / (G area_coef sqrt(I_e))
 *         + loss_extra[b*C + c]                                         (loss_extra == NULL: the last term is absent)
 *   aggregate == 0:  L_b = sum_e I_e + sum_c w_c P_c (index order; w = weights [C] float64, NULL: all 1),
 *                    gI_b = sum_c w_c grad_c - (sum_c w_c - 1), formed in that order;
 *   aggregate == 1:  L_b = sum_e I_e + max_c P_c, the governing case c* the lowest index that attains the maximum,
 *                    gI_b = grad_c*; weights must be NULL.
 * V, M, grad [B*C, Ne] and loss_extra [B*C] are the outputs of the two launches in the middle, status_solve, status_grad [B*C]
 * int32 (each may be NULL) their status outputs.  Outputs, each optional: sample_loss [B], gI [B, Ne], case_penalty [B*C]
 * float64, governing [B] int32 (aggregate 0: the lowest index of the largest w_c P_c),
 *   dpreds[b*ldp + e] = weight / (B ref_b) * gI_b[e] * I_scale[e] * [raw_be > I_min]   for e < Ne, in the dtype of preds,
 * computed in float64 and rounded once, raw recomputed from preds (dpreds needs preds, I_scale, I_mean; columns >= Ne are not
 * touched); ref_b = ref[r] with r as in prep (ref [G] float64; NULL: 1);
 *   value[0] = (float)(weight * (1/B) sum_b L_b / ref_b), float64 partial results in part [ops_design_loss_part_doubles(B)]
 * summed in a fixed order by a second, single-workgroup launch; value_sum[0] += value[0] (optional).  value needs part.
 * A sample with a NaN inertia, a NaN penalty or a non-zero status in any of its C rows gets NaN in sample_loss, gI and the Ne
 * columns of dpreds, and the value is NaN; no other sample's outputs depend on it, on B or on its neighbours in the launch.
 * No atomics, nothing waits on another workgroup.
 *
 * B == 0: OK, nothing enqueued.  NULL args / hp, a negative size, C < 1, Ne < 1, a NULL required pointer, ldp < Ne,
 * aggregate outside {0, 1}, weights with aggregate == 1, alpha_deflection > 0 without deflection_limit > 0 or without
 * loss_extra, rows == NULL with G < B: ERR_INVALID_ARG.  Ne > 512 or C > ops_design_loss_max_cases(): ERR_UNSUPPORTED.
 * All decided on the host before any HIP call, nothing written.  Never throws, never blocks. */
#ifndef OPENPYSTRUCT_AMD_DESIGN_LOSS_H
#define OPENPYSTRUCT_AMD_DESIGN_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "openpystruct_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ops_design_loss_args {
  int B, C, Ne;                 /* samples, load cases per sample, elements per beam */
  int G;                        /* rows of Fy_src and ref */
  int aggregate;                /* 0: weighted sum, 1: worst case */
  int preds_bf16;               /* dtype of preds and dpreds: 0 float32, else bfloat16 */
  long ldp;                     /* row stride of preds and dpreds, in elements */
  const void* preds;            /* [B, ldp] */
  const float* I_scale;         /* [Ne] */
  const float* I_mean;          /* [Ne] */
  float I_min;
  float weight;
  double alpha_deflection;      /* the two fields of ops_sizing_objective (include/openpystruct_amd_sizing_grad.h), as the */
  double deflection_limit;      /* gradient launch was given them */
  const int64_t* rows;          /* [B] or NULL */
  const double* Fy_src;         /* [G, C, N] */
  const double* ref;            /* [G] or NULL */
  const double* weights;        /* [C] or NULL */
  double* I_rows;               /* [B*C, Ne] */
  double* Fy_rows;              /* [B*C, N] */
  const double* V;              /* [B*C, Ne] */
  const double* M;              /* [B*C, Ne] */
  const double* grad;           /* [B*C, Ne] */
  const double* loss_extra;     /* [B*C] or NULL */
  const int32_t* status_solve;  /* [B*C] or NULL */
  const int32_t* status_grad;   /* [B*C] or NULL */
  double* sample_loss;          /* [B] */
  double* gI;                   /* [B, Ne] */
  double* case_penalty;         /* [B*C] */
  int32_t* governing;           /* [B] */
  void* dpreds;                 /* [B, ldp] */
  double* part;                 /* [ops_design_loss_part_doubles(B)] */
  float* value;                 /* [1] */
  float* value_sum;             /* [1] */
} ops_design_loss_args;

int ops_design_loss_prep(const ops_design_loss_args* args, void* stream);
int ops_design_loss_finish(const ops_design_loss_args* args, const ops_sizing_params* hp, void* stream);
int ops_design_loss_max_cases(void);
size_t ops_design_loss_part_doubles(int B);

#ifdef __cplusplus
}
#endif
#endif /* OPENPYSTRUCT_AMD_DESIGN_LOSS_H */
