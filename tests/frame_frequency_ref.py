"""References of the natural-frequency floor in frame design sizing (test code only, runs on the CPU), over
tests/frame_modes_ref.py (the dense eigenpairs, dlambda/dI, the NumPy restatement of the subspace iteration, the shared CASES) and
tests/frame_designs_ref.py / tests/frame_groups_ref.py (the loop oracles of multi-load-case sizing):

  floor_terms            P_f, dP_f/dI, the m coefficients and the size of the terms a gradient row is a sum of, from given pairs
  dense_floor            the same from `dense_modes`
  difference_quotient    central differences of the dense P_f
  loop_oracle_frequency  `loop_oracle_designs` (with `labels`: `loop_oracle_groups`) with the term added; its eigenpairs from
                         `frame_modes_ref.iterate`, continued across the epochs on the library's schedule (start_iters, then iters)
"""
import functools
import math
import types

import numpy as np
import torch

from tests import frame_designs_ref as dr
from tests import frame_groups_ref as gr
from tests import frame_modes_ref as fr
from tests import frame_sizing_total_ref as ft
from tests import sizing_multicase_ref as mr

EPS = fr.EPS
CASES = fr.CASES

# The constant of the elementwise GPU bound |got - ref| <= c 2^-52 sum_j |coef_j| |phi_j|^T |K_b| |phi_j| of the floor kernel's
# rows: c = 4 x the largest ratio the g++ build of csrc/frame_modes.hpp::fm_elem_floor shows on the inputs below over every key of
# CASES at m = 1 and m = 2 (room for another order of the same sums).  The ratio as measured, written to two decimals rounded up --
# 2.66437, on 10x4n-c at m = 1 and m = 2; tests/test_frame_frequency_host.py holds the build to it from both sides.  Never taken from the device.
FLOOR_RATIO = 2.67
C_FLOOR = 4.0 * FLOOR_RATIO
ALPHA = 3.0               # of the kernel tests


def floor_of(min_frequency):
    """(2 pi f)^2 as openpystruct_amd/frame_frequency.py forms it."""
    return (2.0 * math.pi * np.asarray(min_frequency, dtype=np.float64)) ** 2


def floor_terms(case, lam, phi, floor, alpha, m):
    """From pairs lam [>= m], phi [>= m, 3 Nn] (M-normalised): (P_f, dP_f/dI [Ne], coef [m], scale [Ne])."""
    h = np.maximum(0.0, 1.0 - np.asarray(lam[:m], dtype=np.float64) / floor)
    coef = -2.0 * alpha * h / floor
    return float(alpha * np.sum(h * h)), coef @ fr.dlambda_dI(case, phi[:m]), coef, fr.grad_scale(case, phi[:m], coef)


def dense_floor(case, I, M, floor, alpha, m):
    lam, phi = fr.dense_modes(case, I, M, m)
    return floor_terms(case, lam, phi, floor, alpha, m)


def difference_quotient(case, I, M, floor, alpha, m, e, h):
    up, dn = np.array(I, dtype=np.float64), np.array(I, dtype=np.float64)
    up[e] += h
    dn[e] -= h
    return (dense_floor(case, up, M, floor, alpha, m)[0] - dense_floor(case, dn, M, floor, alpha, m)[0]) / (2.0 * h)


@functools.lru_cache(maxsize=None)
def kernel_inputs(key, m, p=None):
    """The floor kernel's inputs on a shared case with p vectors (None: the case's own count): phi [B,p,3Nn] and lam [B,p] -- the dense
    pairs of every frame --, and a per-design floor [B] chosen so that one batch holds designs with every hinge off (floor =
    lambda_1 / 2), with one on (between lambda_1 and lambda_2) and with m on (2 lambda_m), in turn by frame index; a batch of one
    takes the last."""
    case, I, mbar, nodal, kind, p_case = fr.inputs(key)
    p = p_case if p is None else p
    B = I.shape[0]
    n = 3 * case.coords.shape[0]
    phi, lam, floor = np.zeros((B, p, n)), np.zeros((B, p)), np.zeros(B)
    for b in range(B):
        M = fr.dense_M(case, mbar, kind, fr.nodal_of(nodal, b))
        lam[b], phi[b] = fr.dense_modes(case, I[b], M, p)
        floor[b] = (0.5 * lam[b, 0], math.sqrt(lam[b, 0] * lam[b, 1]) if p > 1 else 2.0 * lam[b, 0], 2.0 * lam[b, m - 1])[b % 3 if B > 1 else 2]
    for a in (phi, lam, floor):
        a.setflags(write=False)
    return phi, lam, floor


def kernel_reference(key, m, p=None, alpha=ALPHA):
    """(penalty [B], rows [B,Ne], scale [B,Ne], hinges on [B]) of `kernel_inputs`."""
    case = fr.inputs(key)[0]
    phi, lam, floor = kernel_inputs(key, m, p)
    out = [floor_terms(case, lam[b], phi[b], floor[b], alpha, m) for b in range(len(floor))]
    return (np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[3] for o in out]),
            np.array([int(np.count_nonzero(o[2])) for o in out]))


def loop_oracle_frequency(case, cfg, obj, V0, loads, w, max_epochs, aggregate, weights, term, labels=None, exact=False):
    """`dr.loop_oracle_designs` (labels None; V0 = I0 [G,Ne]) or `gr.loop_oracle_groups` (labels [Ne]; V0 = X0 [G,Ng]) with the
    frequency term.  `term`: a namespace M (the dense mass matrix, one for all designs or a list per design), floor [G], alpha, m, p,
    iters, start_iters.  Per epoch the eigenpairs of the design's float64 inertias come from `fr.iterate` continued from the Q of the
    epoch before (start_iters iterations from `fr.default_start` in the first epoch, iters after it; exact=True: `fr.dense_modes`
    instead, the loop with exact eigenpairs); the float64 gradient takes dP_f/dI before it is segment-summed and rounded; the float32
    loss, aggregated in the step's order, takes + float32(P_f) last.  Returns the namespace of those oracles plus penalty [G] (P_f at
    the last epoch), lam [G,m] (the last epoch's), hinge_margin [G]: the least |1 - lambda_j / floor| over epochs and tracked modes,
    mode_gap [G]: the least `fr.gap(lambda, j)` over epochs and tracked modes, hinges_on [G, max_epochs]: how many tracked modes are
    below the floor at every epoch (-1 past a design's last epoch)."""
    hp = ft.frame_hp(cfg, max_epochs)
    V0, loads, w = np.asarray(V0), np.asarray(loads, dtype=np.float64), np.asarray(w, dtype=np.float64)
    G, Nv = V0.shape
    C = loads.shape[1]
    idx = None if labels is None else torch.as_tensor(np.asarray(labels).astype(np.int64))
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
    loss_hist = np.full((G, max_epochs), np.nan, dtype=np.float32)
    V_out, epochs, governing = np.zeros((G, Nv), dtype=np.float32), np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    case_penalty = np.zeros((G, C), dtype=np.float32)
    margin, gov_gap, gov_gap_last = np.full(G, np.inf), np.full(G, np.inf), np.full(G, np.inf)
    hinge_margin, mode_gap = np.full(G, np.inf), np.full(G, np.inf)
    penalty, lam_last = np.zeros(G), np.zeros((G, term.m))
    hinges_on = np.full((G, max_epochs), -1, dtype=np.int8)
    hinged = obj.alpha_sway > 0.0 or obj.alpha_deflection > 0.0
    w32 = None if weights is None else f32(np.asarray(weights, dtype=np.float64))
    aM, aV = f32(cfg.alpha_moment), f32(cfg.alpha_shear)
    for g in range(G):
        Mg = term.M[g] if isinstance(term.M, (list, tuple)) else term.M
        floor = float(term.floor[g])
        v_tensor = torch.tensor(V0[g], dtype=torch.float32, requires_grad=True)
        optimizer = torch.optim.Adam([v_tensor], lr=cfg.lr)
        best_loss, no_improve = float("inf"), 0
        X = fr.default_start(case, term.p)
        for epoch in range(max_epochs):
            optimizer.zero_grad()
            I_tensor = v_tensor.detach() if idx is None else v_tensor.detach()[idx]
            I_one = I_tensor.numpy().astype(np.float64)
            r = dr.rows_gradient(case, np.repeat(I_one[None, :], C, axis=0), loads[g], w[g], hp, obj, with_lam=False)
            if exact:
                lam, Q = fr.dense_modes(case, I_one, Mg, term.p)
            else:
                lam, Q = fr.iterate(case, I_one, Mg, X, term.start_iters if epoch == 0 else term.iters)[-1][:2]
                X = Q
            Pf, gf, _, _ = floor_terms(case, lam, Q, floor, term.alpha, term.m)
            hinges_on[g, epoch] = int(np.count_nonzero(lam[:term.m] < floor))
            hinge_margin[g] = min(hinge_margin[g], float(np.abs(1.0 - lam[:term.m] / floor).min()))
            mode_gap[g] = min(mode_gap[g], min(fr.gap(lam, j) for j in range(term.m)))
            with torch.no_grad():
                V32, M32 = f32(r.outs[2]), f32(r.outs[3])
                sb = torch.sum(M32 ** 2 / (2 * cfg.E * I_tensor + 1e-8), dim=1)
                ss = torch.sum(V32 ** 2 / (cfg.G * (cfg.k * I_tensor ** 0.5)), dim=1)
                ex = f32(r.loss_extra) if hinged else None
                P = aM * sb + aV * ss
                if hinged:
                    P = P + ex
                sum_I = torch.sum(I_tensor)
                if aggregate == dr.MAX:
                    score = P
                    gov = int(torch.argmax(score))
                    total = sum_I + P[gov]
                elif w32 is not None:
                    score = w32 * P
                    gov = int(torch.argmax(score))
                    total = sum_I
                    for c in range(C):
                        total = total + score[c]
                else:
                    score = P
                    gov = int(torch.argmax(score))
                    total = sum_I + aM * sb[0] + aV * ss[0]
                    if hinged:
                        total = total + ex[0]
                    for c in range(1, C):
                        total = total + P[c]
                total = total + f32(Pf)                                        # the term: last, in float32
            if C > 1:
                top2 = np.sort(score.numpy().astype(np.float64))[-2:]
                gov_gap_last[g] = (top2[1] - top2[0]) / abs(top2[1])
                gov_gap[g] = min(gov_gap[g], gov_gap_last[g])
            g64 = mr.group_gradient(r.grad, weights, aggregate, gov) + gf      # one float64 addition per element, before any sum
            v_tensor.grad = torch.tensor(g64 if labels is None else gr.segment_sum(g64, labels), dtype=torch.float32)
            optimizer.step()
            with torch.no_grad():
                v_tensor.clamp_(min=1e-8)
            current = total.item()
            loss_hist[g, epoch], epochs[g], governing[g], case_penalty[g] = current, epoch + 1, gov, P.numpy()
            penalty[g], lam_last[g] = Pf, lam[:term.m]
            if np.isfinite(best_loss):
                margin[g] = min(margin[g], abs(current - (best_loss - cfg.tolerance)) / abs(current))
            if current < best_loss - cfg.tolerance:
                best_loss, no_improve = current, 0
            else:
                no_improve += 1
            if no_improve >= cfg.patience:
                break
        V_out[g] = v_tensor.detach().numpy()
    out = types.SimpleNamespace(loss=loss_hist, epochs=epochs, governing=governing, case_penalty=case_penalty, margin=margin, gov_gap=gov_gap,
                                gov_gap_last=gov_gap_last, penalty=penalty, lam=lam_last, hinge_margin=hinge_margin, mode_gap=mode_gap,
                                hinges_on=hinges_on)
    if labels is None:
        out.I = V_out
    else:
        out.X, out.I = V_out, V_out[:, np.asarray(labels)]
    return out
