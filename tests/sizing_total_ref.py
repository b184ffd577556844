"""References of the exact-gradient ("total") sizing mode (test code only), all on the CPU:

  total_gradient_ref    dL/dI of the float64 objective by torch autograd through the dense model (tests/beam_dense.py);
                        dense_forward + objective_gradient: the same in two steps, for several objectives on one forward
  step_grad_reference   one gradient-fed optimiser epoch in numpy float64 (the style of oracle.sizing_oracle.sizing_step_reference)
  step_grad_float32     the same epoch with every operation rounded to float32: what round-off alone does to it
  loop_oracle           the whole loop per case: float32 I, torch.optim.Adam + ExponentialLR + clamp, .grad set from the float64
                        total gradient, early stop as in the reference's script
"""
import types

import numpy as np
import torch
from torch.optim.lr_scheduler import ExponentialLR

from oracle import sizing_oracle as so
from tests.beam_dense import dense_solve


def objective(alpha_deflection=0.0, deflection_limit=0.0):
    return types.SimpleNamespace(alpha_deflection=float(alpha_deflection), deflection_limit=float(deflection_limit))


def objective_terms(I, v, V, M, hp, obj):
    """(the three terms of the reference's loss summed, the deflection term) per beam, float64 torch, differentiable."""
    base = I.sum(-1) + hp.alpha_moment * (M ** 2 / (2.0 * hp.E * I + hp.bend_eps)).sum(-1) \
        + hp.alpha_shear * (V ** 2 / (hp.G * hp.area_coef * torch.sqrt(I))).sum(-1)
    if obj.alpha_deflection > 0.0:
        ex = torch.clamp(v.abs() - obj.deflection_limit, min=0.0) / obj.deflection_limit
        extra = obj.alpha_deflection * (ex ** 2).sum(-1)
    else:
        extra = torch.zeros_like(base)
    return base, extra


def total_loss(x, E, I, fix, Fy, wy, hp, obj):
    """L [B] in float64 from the dense model, no gradient: what the central differences difference."""
    with torch.no_grad():
        It = torch.as_tensor(np.asarray(I, dtype=np.float64))
        v, th, V, M = dense_solve(torch.as_tensor(np.asarray(x)), E, It, fix, torch.as_tensor(np.asarray(Fy)), wy)
        base, extra = objective_terms(It, v, V, M, hp, obj)
    return (base + extra).numpy()


def dense_forward(x, E, I, fix, Fy, wy):
    """The dense model's forward with I as a leaf: (I as a torch tensor, (v, theta, V, M)), the graph kept for
    `objective_gradient` -- several objectives can share one forward."""
    It = torch.tensor(np.asarray(I, dtype=np.float64), requires_grad=True)
    return It, dense_solve(torch.as_tensor(np.asarray(x)), E, It, fix, torch.as_tensor(np.asarray(Fy)), wy)


def objective_gradient(fwd, hp, obj, retain_graph=False):
    """Autograd of the float64 objective L through a `dense_forward`.  Returns a namespace of numpy arrays: grad [B,Ne] = dL/dI,
    loss [B], loss_extra [B] (the deflection term), outs = (v, theta, V, M), cot = (gv, None, gV, gM): the objective's own
    cotangents (what tests.beam_dense.gI_term_scale sizes the adjoint's rounding error with) and explicit [B,Ne]: dL/dI with M, V,
    v held fixed."""
    It, outs = fwd
    v, th, V, M = outs
    base, extra = objective_terms(It, v, V, M, hp, obj)
    (grad,) = torch.autograd.grad((base + extra).sum(), It, retain_graph=retain_graph)
    with torch.no_grad():
        Id = It.detach()
        den_b, sq = 2.0 * hp.E * Id + hp.bend_eps, torch.sqrt(Id)
        gM = 2.0 * hp.alpha_moment * M / den_b
        gV = 2.0 * hp.alpha_shear * V / (hp.G * hp.area_coef * sq)
        if obj.alpha_deflection > 0.0:
            gv = 2.0 * obj.alpha_deflection * torch.clamp(v.abs() - obj.deflection_limit, min=0.0) * torch.sign(v) / obj.deflection_limit ** 2
        else:
            gv = torch.zeros_like(v)
        explicit = 1.0 - hp.alpha_moment * M ** 2 * 2.0 * hp.E / den_b ** 2 - hp.alpha_shear * V ** 2 * 0.5 / (hp.G * hp.area_coef * Id ** 1.5)
    n = lambda t: t.detach().numpy()      # noqa: E731
    return types.SimpleNamespace(grad=n(grad), loss=n(base + extra), loss_extra=n(extra), outs=tuple(n(o) for o in outs),
                                 cot=(n(gv), None, n(gV), n(gM)), explicit=n(explicit))


def total_gradient_ref(x, E, I, fix, Fy, wy, hp, obj):
    """dense_solve + autograd of the float64 objective L: `objective_gradient` of a fresh `dense_forward`."""
    return objective_gradient(dense_forward(x, E, I, fix, Fy, wy), hp, obj)


def step_grad_reference(I32, exp_avg32, exp_avg_sq32, V, M, grad, loss_extra, t, best, cnt, hp):
    """ONE gradient-fed optimiser epoch of B cases in numpy float64: `sizing_step_reference` with the Adam gradient taken from
    `grad` [B,Ne] (rounded to float32, then widened) and float32(loss_extra) [B] (None: nothing) added to the loss before the
    early-stop decision.  Same arguments otherwise, same dict; mag = |g|: the gradient comes in exactly rounded, so errors of the
    moments scale with it alone."""
    f64 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)      # noqa: E731
    I, m, v, Vf, Mf, g = f64(I32), f64(exp_avg32), f64(exp_avg_sq32), f64(V), f64(M), f64(grad)
    t, cnt = np.asarray(t, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
    best = f64(best)
    den_b = 2.0 * hp.E * I + hp.bend_eps
    den_s = hp.G * (hp.area_coef * np.sqrt(I))
    loss = I.sum(-1) + hp.alpha_moment * (Mf ** 2 / den_b).sum(-1) + hp.alpha_shear * (Vf ** 2 / den_s).sum(-1)
    if loss_extra is not None:
        loss = loss + f64(loss_extra)
    ea = hp.beta1 * m + (1.0 - hp.beta1) * g
    es = hp.beta2 * v + (1.0 - hp.beta2) * g * g
    step_size, bc2s = so._schedule_f64(t, hp)
    upd = step_size[..., None] * (ea / (np.sqrt(es) / bc2s[..., None] + hp.adam_eps))
    I_free = I - upd
    improved = loss < best - hp.tolerance
    new_cnt = np.where(improved, 0, cnt + 1)
    return {"I": np.maximum(I_free, hp.clamp_min), "I_free": I_free, "exp_avg": ea, "exp_avg_sq": es, "loss": loss,
            "best": np.where(improved, loss, best), "cnt": new_cnt,
            "stop": (new_cnt >= hp.patience) | (t + 1 >= hp.max_epochs), "mag": np.abs(g), "upd": upd}


def step_grad_float32(I32, exp_avg32, exp_avg_sq32, V, M, grad, loss_extra, t, hp):
    """The same epoch with every operation rounded to float32 (the order of a plain elementwise implementation, as
    oracle.sizing_oracle.sizing_step_float32).  Returns I, exp_avg, exp_avg_sq [B,Ne] float32 and loss [B] float32."""
    f = np.float32
    I, m, v = (np.asarray(a, dtype=f) for a in (I32, exp_avg32, exp_avg_sq32))
    Vf, Mf, g = (np.asarray(a, dtype=np.float64).astype(f) for a in (V, M, grad))
    twoE, G, ac = f(2.0 * hp.E), f(hp.G), f(hp.area_coef)
    t64 = np.asarray(t, dtype=np.float64)
    step_size = (hp.lr * hp.gamma ** t64).astype(f) / (1.0 - hp.beta1 ** (t64 + 1.0)).astype(f)
    bc2s = np.sqrt(1.0 - hp.beta2 ** (t64 + 1.0)).astype(f)
    den_b = twoE * I + f(hp.bend_eps)
    den_s = G * (ac * np.sqrt(I))
    loss = I.sum(-1, dtype=f) + f(hp.alpha_moment) * ((Mf * Mf) / den_b).sum(-1, dtype=f) + f(hp.alpha_shear) * ((Vf * Vf) / den_s).sum(-1, dtype=f)
    if loss_extra is not None:
        loss = loss + np.asarray(loss_extra, dtype=np.float64).astype(f)
    ea = f(hp.beta1) * m + f(1.0 - hp.beta1) * g
    es = f(hp.beta2) * v + f(1.0 - hp.beta2) * g * g
    In = np.maximum(I - step_size[..., None] * (ea / (np.sqrt(es) / bc2s[..., None] + f(hp.adam_eps))), f(hp.clamp_min))
    assert all(a.dtype == f for a in (In, ea, es, loss))
    return In, ea, es, loss


def loop_oracle(cases, cfg, obj):
    """The "total" sizing loop of every case, one case at a time on the CPU: float32 I, torch.optim.Adam + ExponentialLR + clamp
    (the reference's optimiser objects), .grad set from the float64 total gradient of this epoch cast to float32, the loss the
    float32 expression of the reference's script on the float32-rounded V, M plus float32(deflection term), early stop as there.
    Returns a namespace: loss [B, max_e] float32 (NaN past a case's last epoch), I [B,Ne] float32 (after the last Adam step),
    epochs [B], vmax [B] (max |v| of each case's last solve)."""
    hp = cfg.c_params()
    B, N = cases.Fy.shape
    Ne = N - 1
    loss_hist = np.full((B, cfg.max_e), np.nan, dtype=np.float32)
    I_out, epochs, vmax = np.zeros((B, Ne), dtype=np.float32), np.zeros(B, dtype=np.int32), np.zeros(B)
    for b in range(B):
        x, fix, Fy = cases.node_positions[b].numpy(), cases.fix[b].numpy(), cases.Fy[b:b + 1].numpy()
        I_tensor = torch.tensor([cfg.I_0] * Ne, dtype=torch.float32, requires_grad=True)
        optimizer = torch.optim.Adam([I_tensor], lr=cfg.lr)
        scheduler = ExponentialLR(optimizer, gamma=cfg.gamma)
        best, cnt = float("inf"), 0
        for epoch in range(cfg.max_e):
            optimizer.zero_grad()
            I64 = I_tensor.detach().numpy().astype(np.float64)[None, :]
            r = total_gradient_ref(x, cfg.E, I64, fix, Fy, cfg.uniform_udl, hp, obj)
            vmax[b] = np.abs(r.outs[0]).max()
            with torch.no_grad():
                M32, V32 = torch.tensor(r.outs[3][0], dtype=torch.float32), torch.tensor(r.outs[2][0], dtype=torch.float32)
                total = torch.sum(I_tensor) + cfg.alpha_moment * torch.sum(M32 ** 2 / (2 * cfg.E * I_tensor + 1e-6)) \
                    + cfg.alpha_shear * torch.sum(V32 ** 2 / (cfg.G * (0.03 * I_tensor ** 0.5)))
                if obj.alpha_deflection > 0.0:
                    total = total + torch.tensor(r.loss_extra[0], dtype=torch.float32)
            I_tensor.grad = torch.tensor(r.grad[0], dtype=torch.float32)
            loss_hist[b, epoch] = total.item()
            optimizer.step()
            scheduler.step()
            with torch.no_grad():
                I_tensor.clamp_(min=1e-8)
            epochs[b] = epoch + 1
            if total.item() < best - cfg.tolerance:
                best, cnt = total.item(), 0
            else:
                cnt += 1
            if cnt >= cfg.patience:
                break
        I_out[b] = I_tensor.detach().numpy()
    return types.SimpleNamespace(loss=loss_hist, I=I_out, epochs=epochs, vmax=vmax)
