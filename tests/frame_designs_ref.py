"""References of multi-load-case frame sizing (test code only), all on the CPU -- the frame counterpart of
tests/sizing_multicase_ref.py, over the dense float64 model with per-row loads (tests/frame_dense_w.py):

  rows_gradient         per (design, case) row on its own: dL_row/dI by autograd, the forward, the hinge values, lambda
  design_objective      L [G] in float64 with ONE leaf I per design shared by its C cases (differentiable)
  design_gradient       autograd of design_objective
  loop_oracle_designs   tests.frame_sizing_total_ref.loop_oracle_frames extended to C cases per design: float32 I, torch.optim.Adam
                        without a scheduler, clamp, one early stop per design; the float32 loss aggregated in the step kernel's order;
                        .grad from the float64 aggregated gradient
"""
import types

import numpy as np
import torch

from tests import frame_sizing_total_ref as ft
from tests import sizing_multicase_ref as mr
from tests.frame_dense_w import dense_frame_solve_w

SUM, MAX = mr.SUM, mr.MAX


def case_penalties(I, disp, V, M, hp, obj):
    """P [..., C] in float64 torch (differentiable): I [..., 1, Ne] or [..., C, Ne]; disp [..., C, Nn, 3]; V, M [..., C, Ne]."""
    P = hp.alpha_moment * (M ** 2 / (2.0 * hp.E * I + hp.bend_eps)).sum(-1) + hp.alpha_shear * (V ** 2 / (hp.G * hp.area_coef * torch.sqrt(I))).sum(-1)
    return P + ft._hinge(disp[..., 0], obj.alpha_sway, obj.sway_limit) + ft._hinge(disp[..., 1], obj.alpha_deflection, obj.deflection_limit)


def rows_gradient(case, I_rows, loads_rows, w_rows, hp, obj, with_lam=True):
    """Every row a frame of its own (what ops_frame_sizing_grad_f64 computes on the G * C rows): `ft.objective_gradient`'s namespace
    (grad [R,Ne] = 1 + dP_row/dI, loss_extra [R], outs, cot, explicit) and lam [R,Nn,3], the adjoint displacements."""
    It = torch.tensor(np.asarray(I_rows, dtype=np.float64), requires_grad=True)
    Lt = torch.tensor(np.asarray(loads_rows, dtype=np.float64), requires_grad=with_lam)
    outs = dense_frame_solve_w(case, It, Lt, torch.as_tensor(np.asarray(w_rows, dtype=np.float64)))
    r = ft.objective_gradient((It, outs), hp, obj, retain_graph=with_lam)
    if with_lam:
        base, extra = ft.objective_terms(It, outs[0], outs[2], outs[3], hp, obj)
        (lam,) = torch.autograd.grad((base + extra).sum(), Lt)
        r.lam = lam.numpy()
    return r


def design_objective(case, I, loads, w, hp, obj, aggregate, weights=None):
    """L [G] (float64 torch, differentiable in `I`) of designs I [G,Ne] (a torch tensor: ONE leaf shared by the C cases of a design)
    under loads [G,C,Nn,3] and element loads w [G,C,Ne,2].  Also returns P [G,C]."""
    loads, w = torch.as_tensor(np.asarray(loads, dtype=np.float64)), torch.as_tensor(np.asarray(w, dtype=np.float64))
    G, C, Nn, _ = loads.shape
    Ne = I.shape[1]
    I_rows = I[:, None, :].expand(G, C, Ne).reshape(G * C, Ne)
    disp, _, V, M = dense_frame_solve_w(case, I_rows, loads.reshape(G * C, Nn, 3), w.reshape(G * C, Ne, 2))
    P = case_penalties(I[:, None, :], disp.reshape(G, C, Nn, 3), V.reshape(G, C, Ne), M.reshape(G, C, Ne), hp, obj)
    if aggregate == MAX:
        return I.sum(-1) + P.max(dim=1).values, P
    wt = torch.ones(C, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights, dtype=np.float64))
    return I.sum(-1) + (wt * P).sum(-1), P


def design_gradient(case, I, loads, w, hp, obj, aggregate, weights=None):
    """Autograd of `design_objective`: a namespace grad [G,Ne], loss [G], P [G,C], governing [G] (the largest w_c P_c; P_c for MAX)."""
    It = torch.tensor(np.asarray(I, dtype=np.float64), requires_grad=True)
    L, P = design_objective(case, It, loads, w, hp, obj, aggregate, weights)
    (grad,) = torch.autograd.grad(L.sum(), It)
    P = P.detach().numpy()
    score = P if (aggregate == MAX or weights is None) else P * np.asarray(weights, dtype=np.float64)[None, :]
    return types.SimpleNamespace(grad=grad.numpy(), loss=L.detach().numpy(), P=P, governing=np.argmax(score, axis=1).astype(np.int32))


def loop_oracle_designs(case, cfg, obj, I0, loads, w, max_epochs, aggregate, weights=None):
    """The multi-case frame sizing loop, one design at a time on the CPU.  I0 [G,Ne], loads [G,C,Nn,3], w [G,C,Ne,2].  Returns a
    namespace: loss [G, max_epochs] float32 (NaN past a design's last epoch), I [G,Ne] float32 (after the last Adam step), epochs [G],
    governing [G] and case_penalty [G,C] float32 (last epoch), margin [G]: the least relative distance of a loss from the early-stop
    threshold it was compared with, gov_gap [G]: the least relative gap, over the epochs, between the two largest scores (what
    rounding would have to bridge to change a governing case; inf for C == 1), gov_gap_last [G]: that gap at the last epoch."""
    hp = ft.frame_hp(cfg, max_epochs)
    I0, loads, w = np.asarray(I0), np.asarray(loads, dtype=np.float64), np.asarray(w, dtype=np.float64)
    G, Ne = I0.shape
    C = loads.shape[1]
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
    loss_hist = np.full((G, max_epochs), np.nan, dtype=np.float32)
    I_out, epochs, governing = np.zeros((G, Ne), dtype=np.float32), np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    case_penalty = np.zeros((G, C), dtype=np.float32)
    margin, gov_gap, gov_gap_last = np.full(G, np.inf), np.full(G, np.inf), np.full(G, np.inf)
    hinged = obj.alpha_sway > 0.0 or obj.alpha_deflection > 0.0
    w32 = None if weights is None else f32(np.asarray(weights, dtype=np.float64))
    aM, aV = f32(cfg.alpha_moment), f32(cfg.alpha_shear)
    for g in range(G):
        I_tensor = torch.tensor(I0[g], dtype=torch.float32, requires_grad=True)
        optimizer = torch.optim.Adam([I_tensor], lr=cfg.lr)
        best_loss, no_improve = float("inf"), 0
        for epoch in range(max_epochs):
            optimizer.zero_grad()
            I64 = np.repeat(I_tensor.detach().numpy().astype(np.float64)[None, :], C, axis=0)
            r = rows_gradient(case, I64, loads[g], w[g], hp, obj, with_lam=False)
            with torch.no_grad():
                V32, M32 = f32(r.outs[2]), f32(r.outs[3])
                sb = torch.sum(M32 ** 2 / (2 * cfg.E * I_tensor + 1e-8), dim=1)
                ss = torch.sum(V32 ** 2 / (cfg.G * (cfg.k * I_tensor ** 0.5)), dim=1)
                ex = f32(r.loss_extra) if hinged else None
                P = aM * sb + aV * ss
                if hinged:
                    P = P + ex
                sum_I = torch.sum(I_tensor)
                if aggregate == MAX:
                    score = P
                    gov = int(torch.argmax(score))
                    total = sum_I + P[gov]
                elif w32 is not None:
                    score = w32 * P
                    gov = int(torch.argmax(score))
                    total = sum_I
                    for c in range(C):
                        total = total + score[c]
                else:                                          # the step kernel's order: ((sum I + a_M b_0) + a_S s_0) + extra_0, then + P_c
                    score = P
                    gov = int(torch.argmax(score))
                    total = sum_I + aM * sb[0] + aV * ss[0]
                    if hinged:
                        total = total + ex[0]
                    for c in range(1, C):
                        total = total + P[c]
            if C > 1:
                top2 = np.sort(score.numpy().astype(np.float64))[-2:]
                gov_gap_last[g] = (top2[1] - top2[0]) / abs(top2[1])
                gov_gap[g] = min(gov_gap[g], gov_gap_last[g])
            I_tensor.grad = torch.tensor(mr.group_gradient(r.grad, weights, aggregate, gov), dtype=torch.float32)
            optimizer.step()
            with torch.no_grad():
                I_tensor.clamp_(min=1e-8)
            current = total.item()
            loss_hist[g, epoch], epochs[g], governing[g], case_penalty[g] = current, epoch + 1, gov, P.numpy()
            if np.isfinite(best_loss):
                margin[g] = min(margin[g], abs(current - (best_loss - cfg.tolerance)) / abs(current))
            if current < best_loss - cfg.tolerance:
                best_loss, no_improve = current, 0
            else:
                no_improve += 1
            if no_improve >= cfg.patience:
                break
        I_out[g] = I_tensor.detach().numpy()
    return types.SimpleNamespace(loss=loss_hist, I=I_out, epochs=epochs, governing=governing, case_penalty=case_penalty, margin=margin,
                                 gov_gap=gov_gap, gov_gap_last=gov_gap_last)
