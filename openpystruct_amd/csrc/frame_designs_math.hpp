// Arithmetic of frame sizing with ONE design under C load cases (csrc/frame_designs.hip; contract:
// include/openpystruct_amd_frame_designs.h).  Two layers:
//
//   per node / per element, plain C++ (device and host): fd_node_rhs and fd_elem_grad are fs_node_rhs and fs_elem_grad of
//   frame_sizing_math.hpp with the inertia's row (the design) named apart from the row of disp, V, M (the design's case) -- the same
//   functions of sizing_grad_math.hpp and frame_adjoint.hpp called in the same order, so with -ffp-contract=off every value rounds
//   as theirs does;
//   per design, device only: frame_design_step is multicase_design of sizing_multicase_math.hpp, statement for statement, with the
//   gradient of a case formed in registers (fd_elem_grad) where that function reads a row of `grad`.  Its parts -- the walk over the
//   cases (fd_design_walk), Adam on one variable, the early stop -- are also those of the group step (csrc/frame_groups.hip).
#pragma once

#include "frame_sizing_math.hpp"

namespace opsamd {

// fs_node_rhs with the inertias of design `d` and the forward of row `b` (= d * C + c)
FA_HD double fd_node_rhs(const FrameSizingObj& o, int n_nodes, int n_elems, const double* elem_geo, const double* elem_EA,
                         const double* elem_E, const int32_t* node_elem_ptr, const int32_t* node_elem_idx, const double* I,
                         const double* disp, const double* V, const double* M, long d, long b, int n, double r[3]) {
  const long node = b * n_nodes + n;
  const double ux = disp[node * 3], uy = disp[node * 3 + 1];
  r[0] = sizing_gv(o.sway, ux);
  r[1] = sizing_gv(o.defl, uy);
  r[2] = 0.0;
  fa_walk(node_elem_ptr, node_elem_idx, n, r, [&](int e, double y[6]) {      // fa_scatter_k, the inertia by design
    const long row = b * n_elems + e;
    const double Ie = I[d * n_elems + e];
    double gf[6];
    fs_fold(o.sway, sizing_quot(o.sway, Ie, V[row], M[row]), gf);
    fa_apply_k(elem_geo[3 * e], elem_geo[3 * e + 1], elem_geo[3 * e + 2], elem_EA[e], elem_E[e] * Ie, gf, y);
  });
  const double h = sizing_defl(o.sway, ux) + sizing_defl(o.defl, uy);
  return (ux != ux || uy != uy) ? ux + uy : h;
}

// what fs_elem_grad reads of one element of one case, as a lane holds it between its loads and its arithmetic
struct FdElemRegs {
  double V, M;
  double u[6], lam[6];      // the end-node values of disp and lambda (fa_gather)
};

// what it reads of the element itself: the same for every case of every design
struct FdElemGeo { double L, c, s, E; };

// fs_elem_grad from registers: the explicit part plus fa_contract's sum, in its order
FA_HD double fd_elem_grad(const SizingObj& o, const FdElemGeo& t, double Ie, const FdElemRegs& q) {
  const SizingQuot sq = sizing_quot(o, Ie, q.V, q.M);
  double gf[6], y[6];
  fs_fold(o, sq, gf);
  fa_apply_k(t.L, t.c, t.s, 0.0, t.E, q.u, y);
  double acc = 0.0;
  for (int k = 0; k < 6; ++k) acc += (gf[k] - q.lam[k]) * y[k];
  return sizing_explicit(o, Ie, q.V, sq) + acc;
}

}  // namespace opsamd

#if defined(__HIPCC__)
#include <type_traits>

#include "sizing_multicase_math.hpp"

namespace opsamd {

struct FrameDesignArgs {
  SizingArgs s;                      // the design's state [G, ...]; s.I64 [G,Ne]: read for the gradient, written by a design that goes on
  int C, aggregate, Nn;
  SizingObj o;                       // the element constants of the objective (the hinges reach the gradient through lambda alone)
  const double* elem_geo; const double* elem_E; const int32_t* conn;
  const double* disp; const double* lambda;            // [G*C, Nn, 3]
  const double* V; const double* M;                    // [G*C, Ne]
  const double* loss_extra;                            // [G*C] or NULL
  const int32_t* status_fwd; const int32_t* status_adj;   // [G*C] or NULL
  const double* weights;                               // [C] or NULL (all 1)
  float* case_penalty;                                 // [G*C] or NULL
  int32_t* governing;                                  // [G] or NULL
  double* grad_out;                                    // [G,Ne] or NULL
};

// The two arrays of the *_dyn step entries (include/openpystruct_amd_frame_frequency.h), both required there: a gradient with respect
// to the element inertias [G,Ne] and a penalty [G] formed outside the step (a frequency floor: DESIGN.md §9r).  They are kernel
// arguments of the DYN instantiations alone, behind the plain arguments: the plain kernels' argument blocks are what they were
struct FrameStepExtras {
  const double* grad_extra;          // [G,Ne]
  const double* penalty_extra;       // [G]
};
struct FrameDesignDynArgs { FrameDesignArgs a; FrameStepExtras x; };
template <bool DYN> using FrameDesignKernelArgs = std::conditional_t<DYN, FrameDesignDynArgs, FrameDesignArgs>;
__device__ __forceinline__ const FrameDesignArgs& fd_plain(const FrameDesignArgs& a) { return a; }
__device__ __forceinline__ const FrameDesignArgs& fd_plain(const FrameDesignDynArgs& a) { return a.a; }
__device__ __forceinline__ const FrameStepExtras* fd_extras(const FrameDesignArgs&) { return nullptr; }
__device__ __forceinline__ const FrameStepExtras* fd_extras(const FrameDesignDynArgs& a) { return &a.x; }

// one load case as the wavefront holds it: the row's scalars and K elements per lane
template <int K>
struct FdCaseRegs {
  FdElemRegs e[K];
  double extra, w;
  bool bad;
};

// issue the loads of row `row` (nothing waits here).  GRAD: with the end-node gathers the gradient needs
template <int K, bool GRAD>
__device__ __forceinline__ void fd_load_case(int lane, long row, int c, int Ne, const FrameDesignArgs& a, const int (&n1)[K],
                                             const int (&n2)[K], FdCaseRegs<K>& q) {
  q.extra = a.loss_extra ? a.loss_extra[row] : 0.0;
  q.w = a.weights ? a.weights[c] : 1.0;
  q.bad = (a.status_fwd && a.status_fwd[row] != 0) || (a.status_adj && a.status_adj[row] != 0);
  // `row` is the same in every lane of the wave: the row's four bases are scalars and a lane's address is one 32-bit offset from one
  const double* Vr = a.V + row * Ne; const double* Mr = a.M + row * Ne;
  const double* ur = a.disp + row * a.Nn * 3; const double* lr = a.lambda + row * a.Nn * 3;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k, ee = e < Ne ? e : 0;
    q.e[k].V = Vr[ee];
    q.e[k].M = Mr[ee];
    if constexpr (GRAD) {
      const int o1 = 3 * n1[k], o2 = 3 * n2[k];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        q.e[k].u[j] = ur[o1 + j];
        q.e[k].u[3 + j] = ur[o2 + j];
        q.e[k].lam[j] = lr[o1 + j];
        q.e[k].lam[3 + j] = lr[o2 + j];
      }
    }
  }
}

// the gradients of the case held in `q`, element by element.  The element's constants (a table shared by every design: cache hits) are
// read here, not held across the walk: at K = 8 the case's end-node values alone are 192 registers of a lane
template <int K, class Put>
__device__ __forceinline__ void fd_case_grad(int lane, int Ne, const FrameDesignArgs& a, const double (&I64)[K], const FdCaseRegs<K>& q,
                                             Put put) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k, ee = e < Ne ? e : 0;
    const FdElemGeo t{a.elem_geo[3 * ee], a.elem_geo[3 * ee + 1], a.elem_geo[3 * ee + 2], a.elem_E[ee]};
    double Ie = I64[k];
    if constexpr (K == 8) __asm__ volatile("" : "+v"(Ie));      // (formed anew in every case: see frame_design_step)
    const double gk = fd_elem_grad(a.o, t, Ie, q.e[k]);
    put(k, q.bad ? __builtin_nan("") : gk);
  }
}

// what the walk over the cases leaves of a design: its loss, governing case and early-stop state, and per lane the float64
// gradient of its K elements, aggregated over the cases, before it is rounded
template <int K>
struct FdWalk {
  int t_ep, cnt, gov;
  float best, loss;
  double g64[K];
};

// The walk of one design over its C cases, shared by the design step (one variable per element) and the group step
// (csrc/frame_groups.hip: one variable per group of elements): penalties, loss, governing case and the per-element gradient.
// SUM: the weighted sum (aggregate 0); else the worst case (aggregate 1).  inertia32(ee): the float32 inertia of element ee, kept in
// I32; after_walk(): the caller's loads that may fly under the last reductions (Adam's moments)
template <int K, bool SUM, class Inertia32, class AfterWalk>
__device__ __forceinline__ void fd_design_walk(int lane, long g, int Ne, const FrameDesignArgs& a, float (&I32)[K], Inertia32 inertia32,
                                               AfterWalk after_walk, FdWalk<K>& w_) {
  const SizingArgs& s = a.s;
  const ops_sizing_params& hp = s.hp;
  const int C = a.C;
  constexpr bool sum = SUM;
  const long row0 = g * C;
  // the design's state: what the walk needs now, Adam's two moments after it (load_case's loads, the moments later)
  w_.t_ep = s.epochs_run[g];
  w_.best = s.best_loss[g];
  w_.cnt = s.patience_cnt[g];
  // the element's end nodes and the design's float64 inertia, once for all cases (a lane past Ne reads element 0 and stores nothing)
  int n1[K], n2[K];
  double I64[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k, ee = e < Ne ? e : 0;
    I32[k] = inertia32(ee);
    n1[k] = a.conn[2 * ee];
    n2[k] = a.conn[2 * ee + 1];
    I64[k] = s.I64[g * Ne + ee];
  }
  FdCaseRegs<K> cur;
  fd_load_case<K, SUM>(lane, row0, 0, Ne, a, n1, n2, cur);

  const float twoE = (float)(2.0 * hp.E), Gf = (float)hp.G;

  // the design's own terms: the two denominators of every element.  At K < 8 the compiler forms them, and what the gradient derives
  // from the inertia alone, once before the walk; at K = 8 those would be some sixty registers of a lane beside the 224 of a case
  // and spill, so there the inertias pass through an empty statement and everything is formed again in every case -- the same
  // expressions on the same numbers either way
  auto inertia = [&](int k) {
    float Ie = I32[k];
    if constexpr (K == 8) __asm__ volatile("" : "+v"(Ie));
    return Ie;
  };
  auto den_b = [&](float Ie) { return twoE * Ie + (float)hp.bend_eps; };
  auto den_s = [&](float Ie) { return Gf * ((float)hp.area_coef * sqrtf(Ie)); };
  float lsum_I = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (lane + 64 * k < Ne) lsum_I += I32[k];
  const float sum_I = wave_sum(lsum_I);

  // the walk over the cases.  Per case: everything a lane forms from its own elements (the two partial sums, the gradient), then
  // the NEXT case's loads are issued into the registers this case has left, then this case's two wave reductions run under them
  float loss = sum_I, top = 0.f;
  int gov = 0;
  double wsum = 0.0;
  double gacc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) gacc[k] = 0.0;
  // (the last case stands apart from the loop: the loop's loads are unconditional and the last turn issues none)
  auto one_case = [&](int c, auto last) {
    float lsum_b = 0.f, lsum_s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = lane + 64 * k;
      if (e < Ne) {
        const float m = (float)cur.e[k].M, v = (float)cur.e[k].V;
        const float Ie = inertia(k);
        lsum_b += (m * m) / den_b(Ie);
        lsum_s += (v * v) / den_s(Ie);
      }
    }
    const double extra = cur.extra, w = cur.w;
    if constexpr (sum) {
      wsum += w;
      fd_case_grad<K>(lane, Ne, a, I64, cur, [&](int k, double gk) { gacc[k] += w * gk; });
      // this case's registers are free: only now the next case's loads.  The empty statements tie the order down -- each needs its
      // sum and no load may be moved across them; left to itself the compiler issues the loads first, keeps two cases in registers
      // (spilling at K = 8) and copies one onto the other at the end of every turn
#pragma unroll
      for (int k = 0; k < K; ++k) __asm__ volatile("" : "+v"(gacc[k]) : : "memory");
    }
    if constexpr (!decltype(last)::value) fd_load_case<K, SUM>(lane, row0 + c + 1, c + 1, Ne, a, n1, n2, cur);
    const float sb = wave_sum(lsum_b), ss = wave_sum(lsum_s);
    float P = (float)hp.alpha_moment * sb + (float)hp.alpha_shear * ss;
    if (a.loss_extra) P += (float)extra;
    float score = P;                              // what the governing case is the largest of
    if constexpr (sum) {
      if (a.weights) {
        score = (float)w * P;
        loss += score;
      } else if (c == 0) {                        // step_case's order: ((sum I + a_M b) + a_S s) + extra
        loss = sum_I + (float)hp.alpha_moment * sb + (float)hp.alpha_shear * ss;
        if (a.loss_extra) loss += (float)extra;
      } else {
        loss += P;
      }
    }
    if (c == 0 || score > top) { top = score; gov = c; }      // ties keep the lowest index
    if (a.case_penalty && lane == 0) a.case_penalty[row0 + c] = P;
  };
#pragma unroll 1
  for (int c = 0; c + 1 < C; ++c) one_case(c, std::false_type{});
  one_case(C - 1, std::true_type{});
  after_walk();                                   // Adam's moments: in flight under the last reductions
  if constexpr (sum) {
    const double once = wsum - 1.0;               // every case's gradient carries the weight term's 1
#pragma unroll
    for (int k = 0; k < K; ++k) w_.g64[k] = gacc[k] - once;
  } else {
    loss = sum_I + top;
    fd_load_case<K, true>(lane, row0 + gov, gov, Ne, a, n1, n2, cur);      // the governing row, read now that it is known
    fd_case_grad<K>(lane, Ne, a, I64, cur, [&](int k, double gk) { w_.g64[k] = gk; });
  }
  w_.loss = loss;
  w_.gov = gov;
}

// Adam's step sizes of epoch t_ep (step_case).  Formed after the walk: pow() in double needs the registers a case occupies
struct FdAdam { float step_size, bc2s, omb1, omb2; };

__device__ __forceinline__ FdAdam fd_adam_sizes(const SizingArgs& s, int t_ep) {
  const ops_sizing_params& hp = s.hp;
  FdAdam z;
  if (s.schedule) {
    z.step_size = s.schedule[2 * t_ep];
    z.bc2s = s.schedule[2 * t_ep + 1];
  } else {
    const float lr_t = (float)(hp.lr * pow(hp.gamma, (double)t_ep));
    const float bc1 = (float)(1.0 - pow(hp.beta1, (double)(t_ep + 1)));
    z.bc2s = (float)sqrt(1.0 - pow(hp.beta2, (double)(t_ep + 1)));
    z.step_size = lr_t / bc1;
  }
  z.omb1 = (float)(1.0 - hp.beta1);
  z.omb2 = (float)(1.0 - hp.beta2);
  return z;
}

// Adam and the clamp on one variable (step_case): x with gradient gk and moments m, v -> its new value; the new moments in ea, es
__device__ __forceinline__ float fd_adam_var(const ops_sizing_params& hp, const FdAdam& z, float x, float gk, float m, float v, float& ea,
                                             float& es) {
  ea = (float)hp.beta1 * m + z.omb1 * gk;
  es = (float)hp.beta2 * v + z.omb2 * gk * gk;
  const float denom = sqrtf(es) / z.bc2s + (float)hp.adam_eps;
  float xn = x - z.step_size * (ea / denom);
  return fmaxf(xn, (float)hp.clamp_min);
}

// early stopping, one decision per design: updates best and cnt of `w`, true when the design stops
template <int K>
__device__ __forceinline__ bool fd_early_stop(const ops_sizing_params& hp, FdWalk<K>& w) {
  if (w.loss < w.best - (float)hp.tolerance) { w.best = w.loss; w.cnt = 0; } else { w.cnt += 1; }
  return (w.cnt >= hp.patience) || (w.t_ep + 1 >= hp.max_epochs);
}

// the design's scalars, by one lane
template <int K>
__device__ __forceinline__ void fd_store_design(int lane, long g, const FrameDesignArgs& a, const FdWalk<K>& w, bool stop) {
  const SizingArgs& s = a.s;
  if (lane == 0) {
    s.best_loss[g] = w.best;
    s.patience_cnt[g] = w.cnt;
    s.epochs_run[g] = w.t_ep + 1;
    s.last_loss[g] = w.loss;
    if (a.governing) a.governing[g] = w.gov;
    if (stop) s.active[g] = 0;
  }
}

// What a DYN step adds once the walk has ended (gx, px: the design's extras as the lane loaded them): one float64 addition per
// element before anything reads the gradient, and the penalty onto the loss, last, in float32
template <int K>
__device__ __forceinline__ void fd_add_extras(const double (&gx)[K], double px, FdWalk<K>& w) {
#pragma unroll
  for (int k = 0; k < K; ++k) w.g64[k] += gx[k];
  w.loss = w.loss + (float)px;
}

template <int K, bool SUM, bool DYN = false>
__device__ __forceinline__ void frame_design_step(int lane, long g, int Ne, const FrameDesignArgs& a, const FrameStepExtras* x = nullptr) {
  const SizingArgs& s = a.s;
  const ops_sizing_params& hp = s.hp;
  float I32[K], m[K], v[K];
  [[maybe_unused]] double gx[K], px;
  FdWalk<K> w;
  fd_design_walk<K, SUM>(lane, g, Ne, a, I32, [&](int ee) { return s.I[g * Ne + ee]; }, [&]() {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = lane + 64 * k;
      const long o = g * Ne + (e < Ne ? e : 0);
      m[k] = s.exp_avg[o];
      v[k] = s.exp_avg_sq[o];
      if constexpr (DYN) gx[k] = x->grad_extra[o];
    }
    if constexpr (DYN) px = x->penalty_extra[g];
  }, w);
  if constexpr (DYN) fd_add_extras<K>(gx, px, w);

  // Adam, clamp (step_case)
  const FdAdam z = fd_adam_sizes(s, w.t_ep);
  float Inew[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = lane + 64 * k;
    Inew[k] = 0.f;
    if (e < Ne) {
      const long o = g * Ne + e;
      if (a.grad_out) a.grad_out[o] = w.g64[k];
      float ea, es;
      const float In = fd_adam_var(hp, z, I32[k], (float)w.g64[k], m[k], v[k], ea, es);
      s.exp_avg[o] = ea;
      s.exp_avg_sq[o] = es;
      s.I[o] = In;
      Inew[k] = In;
    }
  }
  const bool stop = fd_early_stop(hp, w);
  if (!stop) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = lane + 64 * k;
      if (e < Ne) s.I64[g * Ne + e] = (double)Inew[k];   // what the next factorisation reads, once per design
    }
  }
  fd_store_design(lane, g, a, w, stop);
}

// ---- host side: what ops_frame_design_step_f32 and ops_frame_group_step_f32 (csrc/frame_groups.hip) check and fill alike ----

constexpr int kFrameDesignMaxCases = 64;

// The design step's refusals, in its order, and its arguments in *a.  OPS_AMD_OK with G == 0: nothing to launch, *a not filled.
inline int frame_design_args(int G, int C, int n_nodes, int n_elems, const double* elem_geo, const double* elem_E, const int32_t* conn,
                             float* I, double* I64, const double* disp, const double* V, const double* M, const double* lambda,
                             const double* loss_extra, const int32_t* status_fwd, const int32_t* status_adj, const double* weights,
                             int aggregate, float* exp_avg, float* exp_avg_sq, float* best_loss, int32_t* patience_cnt,
                             int32_t* epochs_run, uint8_t* active, float* last_loss, float* case_penalty, int32_t* governing,
                             double* grad_out, const ops_sizing_params* hp, const float* schedule, FrameDesignArgs* a) {
  if (G < 0 || C < 1 || n_nodes < 2 || n_elems < 1) return OPS_AMD_ERR_INVALID_ARG;
  if (aggregate != 0 && aggregate != 1) return OPS_AMD_ERR_INVALID_ARG;
  if (aggregate == 1 && weights) return OPS_AMD_ERR_INVALID_ARG;
  if (n_elems > kSizingMaxElems || C > kFrameDesignMaxCases || (long)G * C > 0x7fffffffL) return OPS_AMD_ERR_UNSUPPORTED;
  if (G == 0) return OPS_AMD_OK;
  if (!elem_geo || !elem_E || !conn || !I || !I64 || !disp || !V || !M || !lambda || !exp_avg || !exp_avg_sq || !best_loss ||
      !patience_cnt || !epochs_run || !active || !last_loss || !hp)
    return OPS_AMD_ERR_INVALID_ARG;
  // the objective without its hinges, as ops_frame_sizing_grad_f64 forms it: they reach the gradient through lambda alone
  *a = FrameDesignArgs{};
  a->s = sizing_args(I, exp_avg, exp_avg_sq, best_loss, patience_cnt, epochs_run, active, last_loss, hp);
  a->s.I64 = I64; a->s.schedule = schedule;
  a->C = C; a->aggregate = aggregate; a->Nn = n_nodes;
  a->o = frame_sizing_obj(hp, 0.0, 0.0, 0.0, 0.0).sway;
  a->elem_geo = elem_geo; a->elem_E = elem_E; a->conn = conn;
  a->disp = disp; a->lambda = lambda; a->V = V; a->M = M; a->loss_extra = loss_extra;
  a->status_fwd = status_fwd; a->status_adj = status_adj; a->weights = weights;
  a->case_penalty = case_penalty; a->governing = governing; a->grad_out = grad_out;
  return OPS_AMD_OK;
}

}  // namespace opsamd
#endif
