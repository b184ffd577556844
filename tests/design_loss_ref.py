"""References of the design-objective term (test code only), numpy float64 on the CPU, built on the multi-case
references of tests/sizing_multicase_ref.py (`case_penalties`, `group_gradient`, `design_autograd`):

  prep_reference      the inertias of standardised predictions, the framework's expression
  finish_reference    what ops_design_loss_finish computes from the rows of the two launches in the middle, with the bound every
                      float64 output is held to
  synthetic_rows      seeded inputs of the finish launch for B samples x C cases
  term_autograd       sample by sample: the objective and its gradient by autograd through the dense model, one leaf per design

The bound of a float64 sum of n terms formed in any order: (n + C) 2^-53 sum |terms| -- n - 1 additions of the kernel's order and
of the reference's each lose at most 2^-53 of the running magnitude, the terms themselves are formed by the same correctly
rounded operations on both sides, and C more roundings tie the cases together.
"""
import types

import numpy as np
import torch

from tests import sizing_multicase_ref as mr
from tests import sizing_step_cases as sc
from tests import sizing_total_ref as tr

U = 2.0 ** -53


def prep_reference(preds, scaler):
    """sI.inverse_transform(p.float()).clamp_min(1e-8).double() -- `preds` a torch tensor (float32 or bfloat16), [B, Ne]."""
    return scaler.inverse_transform(preds.float()).clamp_min(1e-8).double()


def raw_reference(preds, scaler):
    return scaler.inverse_transform(preds.float())


def finish_reference(I, V, M, grad, extra, weights, aggregate, hp, *, live=None, scale=None, weight=1.0, ref=None, status=None):
    """I [B,Ne]; V, M, grad [B,C,Ne]; extra [B,C] or None; weights [C] or None; live [B,Ne] bool (raw > I_min) and scale [Ne]
    for dpreds; ref [B] (gathered) or None; status [B,C] or None.  Returns a namespace: sample_loss, gI, case_penalty, governing,
    dpreds (float64, unrounded), value (float64) and the bounds tol_P [B,C], tol_L [B], tol_g [B,Ne], tol_d [B,Ne] (float64 part
    only), tol_value (float64 part only)."""
    I, V, M, grad = (np.asarray(t, dtype=np.float64) for t in (I, V, M, grad))
    B, C, Ne = V.shape
    free = tr.objective()
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float64)
    P = np.zeros((B, C)); tol_P = np.zeros((B, C))
    L = np.zeros(B); tol_L = np.zeros(B)
    gov = np.zeros(B, dtype=np.int32)
    for b in range(B):
        It = torch.as_tensor(I[b])
        P[b] = mr.case_penalties(It, None, torch.as_tensor(V[b]), torch.as_tensor(M[b]), hp, free).numpy()
        tb = hp.alpha_moment * (M[b] ** 2 / (2.0 * hp.E * I[b] + hp.bend_eps))
        ts = hp.alpha_shear * (V[b] ** 2 / (hp.G * hp.area_coef * np.sqrt(I[b])))
        mag = np.abs(tb).sum(-1) + np.abs(ts).sum(-1)
        n = 2 * Ne
        if extra is not None:
            P[b] = P[b] + np.asarray(extra, dtype=np.float64)[b]
            mag = mag + np.abs(extra[b])
            n += 1
        tol_P[b] = (n + C) * U * mag
        if aggregate == mr.MAX:
            gov[b] = int(np.argmax(P[b]))
            L[b] = I[b].sum() + P[b, gov[b]]
            tol_L[b] = (Ne + n + C) * U * (np.abs(I[b]).sum() + mag[gov[b]])
        else:
            gov[b] = int(np.argmax(w * P[b]))
            L[b] = I[b].sum() + (w * P[b]).sum()
            tol_L[b] = (Ne + C * n + C) * U * (np.abs(I[b]).sum() + (w * mag).sum())
    gI = mr.group_gradient(grad, weights, aggregate, gov)
    if aggregate == mr.MAX:
        tol_g = np.zeros((B, Ne))
    else:       # terms: w_c g_c (C of them), w_c (C), the 1
        tol_g = (2 * C + 1 + C) * U * ((np.abs(w[None, :, None] * grad)).sum(1) + w.sum() + 1.0)
    bad = ~np.isfinite(I).all(-1) | ~np.isfinite(P).all(-1)
    if status is not None:
        bad |= (np.asarray(status).reshape(B, C) != 0).any(-1)
    L = np.where(bad, np.nan, L)
    gI = np.where(bad[:, None], np.nan, gI)
    r = np.ones(B) if ref is None else np.asarray(ref, dtype=np.float64)
    out = types.SimpleNamespace(sample_loss=L, gI=gI, case_penalty=P, governing=gov, tol_P=tol_P, tol_L=tol_L, tol_g=tol_g, bad=bad)
    share = L / r
    out.value = float(weight) * share.sum() / B
    out.tol_value = float(weight) / B * ((tol_L / r).sum() + (B + C) * U * np.abs(np.where(bad, 0.0, share)).sum() + 4 * U * np.abs(np.where(bad, 0.0, share)).sum())
    if live is not None:
        coef = float(weight) / (B * r)
        s = np.asarray(scale, dtype=np.float64)
        d = coef[:, None] * gI * s[None, :]
        out.dpreds = np.where(np.asarray(live), d, np.where(bad[:, None], np.nan, 0.0))
        out.tol_d = np.abs(coef[:, None] * s[None, :]) * tol_g + 4 * U * np.abs(np.where(bad[:, None], 0.0, d))
    return out


def well_separated(P, margin=0.05):
    """Every sample's two largest penalties at least `margin` apart (relative to the largest): the governing case of the reference
    is then the kernel's whatever the rounding."""
    P = np.sort(np.asarray(P), axis=-1)
    return P.shape[-1] < 2 or bool(((P[..., -1] - P[..., -2]) >= margin * np.abs(P[..., -1])).all())


def synthetic_rows(B, C, Ne, seed):
    """Seeded inputs of one finish launch: I [B,Ne] (tests.sizing_step_cases.optimiser_state's, widened), V, M [B,C,Ne] of
    random_forces with ONE case per sample scaled by 4 (the §9j fixture's way to a clear worst case: its penalty grows 16-fold),
    per-row gradients 1 + N(0,1) 10^U(-2,2), deflection terms U(0, 1) of the smallest penalty's size."""
    rng = np.random.default_rng([B, C, Ne, seed, 23])
    I32, _, _ = sc.optimiser_state(rng, B, Ne)
    I = I32.astype(np.float64)
    V, M = sc.random_forces(rng, B * C, Ne)
    V, M = V.reshape(B, C, Ne).copy(), M.reshape(B, C, Ne).copy()
    big = rng.integers(0, C, size=B)
    # equalise the cases' penalties first, so that the scaled case governs by a known margin whatever was drawn
    hp = sc.beam_hp()
    for b in range(B):
        P = mr.case_penalties(torch.as_tensor(I[b]), None, torch.as_tensor(V[b]), torch.as_tensor(M[b]), hp, tr.objective()).numpy()
        f = np.sqrt(P.min() / P)
        V[b] *= f[:, None]; M[b] *= f[:, None]
        V[b, big[b]] *= 4.0; M[b, big[b]] *= 4.0
    grad = 1.0 + rng.standard_normal((B, C, Ne)) * np.exp(rng.uniform(np.log(1e-2), np.log(1e2), size=(B, C, Ne)))
    Pmin = np.array([mr.case_penalties(torch.as_tensor(I[b]), None, torch.as_tensor(V[b]), torch.as_tensor(M[b]), hp, tr.objective()).numpy().min()
                     for b in range(B)])
    extra = rng.uniform(0.0, 1.0, size=(B, C)) * Pmin[:, None]
    return types.SimpleNamespace(I=I, V=V, M=M, grad=grad, extra=extra, big=big, hp=hp)


def term_autograd(x, E, I, fix, Fy, wy, hp, obj, weights, aggregate):
    """I [B,Ne], Fy [B,C,N]: `design_autograd` per sample.  Namespace: loss [B], grad [B,Ne], P [B,C], governing [B]."""
    rs = [mr.design_autograd(x, E, I[b], fix, Fy[b], wy, hp, obj, weights, aggregate) for b in range(len(I))]
    return types.SimpleNamespace(loss=np.array([r.loss for r in rs]), grad=np.stack([r.grad for r in rs]),
                                 P=np.stack([r.P for r in rs]), governing=np.array([r.governing for r in rs], dtype=np.int32))
