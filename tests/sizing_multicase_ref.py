"""References of the multi-load-case sizing mode (test code only), all on the CPU:

  group_gradient        the design's Adam gradient from the per-row gradients of its C load cases (the identity the kernel uses)
  design_autograd       dL/dI of the design objective by torch autograd through the dense model, I shared by the C rows
  design_step_reference one design step in numpy float64: tests.sizing_total_ref.step_grad_reference with the aggregated loss and gradient
  design_inputs         seeded optimiser states, forces, gradients and penalties of G designs x C cases
  loop_oracle           the whole loop per design: float32 I, torch.optim.Adam + ExponentialLR + clamp, .grad set from the float64
                        group gradient through the dense model, one early stop per design
"""
import types

import numpy as np
import torch
from torch.optim.lr_scheduler import ExponentialLR

from tests import sizing_step_cases as sc
from tests import sizing_total_ref as tr
from tests.beam_dense import dense_solve

SUM, MAX = 0, 1


def group_gradient(grad_rows, weights, aggregate, governing=None):
    """[..., C, Ne] per-row gradients (each 1 + dP_c/dI) -> the design's [..., Ne]: sum_c w_c grad_c - (sum_c w_c - 1) in float64
    (the weight term counted once), or the governing row."""
    grad_rows = np.asarray(grad_rows, dtype=np.float64)
    C = grad_rows.shape[-2]
    if aggregate == MAX:
        return np.take_along_axis(grad_rows, np.asarray(governing)[..., None, None], axis=-2)[..., 0, :]
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float64)
    acc, wsum = np.zeros(grad_rows.shape[:-2] + grad_rows.shape[-1:]), 0.0
    for c in range(C):                   # the kernel's order
        acc = acc + w[c] * grad_rows[..., c, :]
        wsum = wsum + w[c]
    return acc - (wsum - 1.0)


def case_penalties(I, v, V, M, hp, obj):
    """P_c [C] of one design in float64 torch (differentiable): I [Ne] shared, v [C,N], V, M [C,Ne]."""
    P = hp.alpha_moment * (M ** 2 / (2.0 * hp.E * I + hp.bend_eps)).sum(-1) + hp.alpha_shear * (V ** 2 / (hp.G * hp.area_coef * torch.sqrt(I))).sum(-1)
    if obj.alpha_deflection > 0.0:
        ex = torch.clamp(v.abs() - obj.deflection_limit, min=0.0) / obj.deflection_limit
        P = P + obj.alpha_deflection * (ex ** 2).sum(-1)
    return P


def design_autograd(x, E, I, fix, Fy, wy, hp, obj, weights, aggregate):
    """One design: I [Ne] a single leaf expanded to its C rows, L = sum I + sum_c w_c P_c | sum I + max_c P_c through dense_solve.
    Returns a namespace: grad [Ne], loss, P [C], governing."""
    It = torch.tensor(np.asarray(I, dtype=np.float64), requires_grad=True)
    Fy = torch.as_tensor(np.asarray(Fy))
    C = Fy.shape[0]
    v, th, V, M = dense_solve(torch.as_tensor(np.asarray(x)), E, It[None, :].expand(C, -1), fix, Fy, wy)
    P = case_penalties(It, v, V, M, hp, obj)
    if aggregate == MAX:
        L = It.sum() + P.max()
    else:
        w = torch.ones(C, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights, dtype=np.float64))
        L = It.sum() + (w * P).sum()
    (grad,) = torch.autograd.grad(L, It)
    return types.SimpleNamespace(grad=grad.numpy(), loss=float(L.detach()), P=P.detach().numpy(), governing=int(torch.argmax(P)))


def design_step_reference(I32, exp_avg32, exp_avg_sq32, V, M, grad, loss_extra, weights, aggregate, t, best, cnt, hp):
    """ONE design step of G designs in numpy float64: I, exp_avg, exp_avg_sq [G,Ne] float32; V, M, grad [G,C,Ne] float64 (rounded
    to float32 for the loss as the kernel does, grad aggregated in float64 and rounded once); loss_extra [G,C] or None; weights [C]
    or None.  The dict of `tr.step_grad_reference` plus case_penalty [G,C] and governing [G].  With C == 1, the sum and unit weight
    it returns exactly what `tr.step_grad_reference` returns on the one row."""
    f64 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)      # noqa: E731
    I, Vf, Mf = f64(I32), f64(V), f64(M)
    G, C, Ne = Vf.shape
    den_b = 2.0 * hp.E * I + hp.bend_eps
    den_s = hp.G * (hp.area_coef * np.sqrt(I))
    sb = (Mf ** 2 / den_b[:, None, :]).sum(-1)         # [G,C]
    ss = (Vf ** 2 / den_s[:, None, :]).sum(-1)
    ex = None if loss_extra is None else f64(loss_extra)
    P = hp.alpha_moment * sb + hp.alpha_shear * ss
    if ex is not None:
        P = P + ex
    if aggregate == MAX:
        assert weights is None
        gov = np.argmax(P, axis=1)                       # the first index that attains the maximum
        loss = I.sum(-1) + P[np.arange(G), gov]
    else:
        w = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float64)
        gov = np.argmax(w[None, :] * P, axis=1)
        loss = I.sum(-1)
        for c in range(C):                               # step_grad_reference's order, case by case (w == 1: its very expression)
            loss = loss + w[c] * (hp.alpha_moment * sb[:, c]) + w[c] * (hp.alpha_shear * ss[:, c])
            if ex is not None:
                loss = loss + w[c] * ex[:, c]
    g = group_gradient(grad, weights, aggregate, gov)
    out = tr.step_grad_reference(I32, exp_avg32, exp_avg_sq32, V[:, 0], M[:, 0], g, None, t, best, cnt, hp)   # Adam, clamp
    t, cnt = np.asarray(t, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
    best = f64(best)
    improved = loss < best - hp.tolerance
    new_cnt = np.where(improved, 0, cnt + 1)
    out.update(loss=loss, best=np.where(improved, loss, best), cnt=new_cnt,
               stop=(new_cnt >= hp.patience) | (t + 1 >= hp.max_epochs), case_penalty=P, governing=gov.astype(np.int32))
    return out


def design_inputs(G, C, Ne, seed):
    """Seeded inputs of one step of G designs x C cases: the optimiser state of sc.optimiser_state, forces of sc.random_forces per
    row, per-row gradients 1 + N(0,1) * 10^U(-2,2) and deflection terms U(0, 50)."""
    rng = np.random.default_rng([G, C, Ne, seed, 11])
    I, m, v = sc.optimiser_state(rng, G, Ne)
    V, M = sc.random_forces(rng, G * C, Ne)
    grad = 1.0 + rng.standard_normal((G, C, Ne)) * np.exp(rng.uniform(np.log(1e-2), np.log(1e2), size=(G, C, Ne)))
    extra = rng.uniform(0.0, 50.0, size=(G, C))
    return I, m, v, V.reshape(G, C, Ne), M.reshape(G, C, Ne), grad, extra


def design_epoch(I, m, v, V, M, grad, extra, weights, aggregate, hp, shift, group=4):
    """sc.reference_epoch for the design step: early-stop states placed from the reference's loss, then the reference of the epoch."""
    G = I.shape[0]
    z = np.zeros(G, dtype=np.int64)
    loss = design_step_reference(I, m, v, V, M, grad, extra, weights, aggregate, z, np.full(G, np.inf), z, hp)["loss"]
    st = sc.case_states(loss, hp, shift, group)
    ref = design_step_reference(I, m, v, V, M, grad, extra, weights, aggregate, st.t, st.best, st.cnt, hp)
    assert (np.abs(st.best.astype(np.float64) - hp.tolerance - ref["loss"]) >= 1e-3 * np.abs(ref["loss"] + hp.tolerance))[st.kind != "e"].all()
    want_stop = (st.kind == "c") | (st.kind == "d")
    assert (ref["stop"][st.kind != "e"] == want_stop[st.kind != "e"]).all()
    return st, ref


def loop_oracle(cases, cfg, obj, C, aggregate, weights=None):
    """The multi-case sizing loop of every design, one design at a time on the CPU, in the style of `tr.loop_oracle`: float32 I,
    torch.optim.Adam + ExponentialLR + clamp, .grad the float64 group gradient (per-row total gradients through the dense model)
    cast to float32, the loss the float32 expression on the float32-rounded V, M of every case plus float32(deflection term),
    aggregated in float32; one early stop per design.  Returns a namespace: loss [G, max_e] float32 (NaN past the last epoch),
    I [G,Ne] float32, epochs [G], penalties [G, max_e, C] float32 (NaN past the last epoch), governing [G] (last epoch)."""
    hp = cfg.c_params()
    B, N = cases.Fy.shape
    Ne, G = N - 1, B // C
    loss_hist = np.full((G, cfg.max_e), np.nan, dtype=np.float32)
    pen_hist = np.full((G, cfg.max_e, C), np.nan, dtype=np.float32)
    I_out, epochs, governing = np.zeros((G, Ne), dtype=np.float32), np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    w64 = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float64)
    for g in range(G):
        rows = slice(g * C, (g + 1) * C)
        x, fix, Fy = cases.node_positions[g * C].numpy(), cases.fix[g * C].numpy(), cases.Fy[rows].numpy()
        I_tensor = torch.tensor([cfg.I_0] * Ne, dtype=torch.float32, requires_grad=True)
        optimizer = torch.optim.Adam([I_tensor], lr=cfg.lr)
        scheduler = ExponentialLR(optimizer, gamma=cfg.gamma)
        best, cnt = float("inf"), 0
        for epoch in range(cfg.max_e):
            optimizer.zero_grad()
            I64 = np.repeat(I_tensor.detach().numpy().astype(np.float64)[None, :], C, axis=0)
            r = tr.total_gradient_ref(x, cfg.E, I64, fix, Fy, cfg.uniform_udl, hp, obj)
            with torch.no_grad():
                M32, V32 = torch.tensor(r.outs[3], dtype=torch.float32), torch.tensor(r.outs[2], dtype=torch.float32)
                P = cfg.alpha_moment * torch.sum(M32 ** 2 / (2 * cfg.E * I_tensor + 1e-6), dim=1) \
                    + cfg.alpha_shear * torch.sum(V32 ** 2 / (cfg.G * (0.03 * I_tensor ** 0.5)), dim=1)
                if obj.alpha_deflection > 0.0:
                    P = P + torch.tensor(r.loss_extra, dtype=torch.float32)
                if aggregate == MAX:
                    gov = int(torch.argmax(P))
                    total = torch.sum(I_tensor) + P[gov]
                else:
                    wP = torch.tensor(w64, dtype=torch.float32) * P
                    gov = int(torch.argmax(wP))
                    total = torch.sum(I_tensor)
                    for c in range(C):
                        total = total + wP[c]
            I_tensor.grad = torch.tensor(group_gradient(r.grad, weights, aggregate, gov), dtype=torch.float32)
            loss_hist[g, epoch], pen_hist[g, epoch], governing[g] = total.item(), P.numpy(), gov
            optimizer.step()
            scheduler.step()
            with torch.no_grad():
                I_tensor.clamp_(min=1e-8)
            epochs[g] = epoch + 1
            if total.item() < best - cfg.tolerance:
                best, cnt = total.item(), 0
            else:
                cnt += 1
            if cnt >= cfg.patience:
                break
        I_out[g] = I_tensor.detach().numpy()
    return types.SimpleNamespace(loss=loss_hist, I=I_out, epochs=epochs, penalties=pen_hist, governing=governing)


def design_objective(cases, cfg, I, obj, C, aggregate, weights=None):
    """The float64 objective [G] of designs I [G,Ne] under their C cases, by the dense model."""
    hp = cfg.c_params()
    G = I.shape[0]
    out = np.zeros(G)
    for g in range(G):
        rows = slice(g * C, (g + 1) * C)
        out[g] = design_autograd(cases.node_positions[g * C].numpy(), cfg.E, I[g], cases.fix[g * C].numpy(), cases.Fy[rows].numpy(),
                                 cfg.uniform_udl, hp, obj, weights, aggregate).loss
    return out
