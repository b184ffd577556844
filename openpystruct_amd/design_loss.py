"""The sizing objective of a PREDICTED design, as a loss term and as a metric.

The surrogates predict one inertia distribution per structure; the sizing loop (sizing.py, multicase.py) minimises

    L(I) = sum_e I_e + agg_c P_c(I)        P_c: moment + shear (+ deflection) penalty of load case c, M, V, v functions of I
                                           through the solve; agg = weighted sum or worst case (§9j)

This module evaluates that objective for ANY designs under their C load cases (`design_objective`: predictions, heuristic labels,
optimiser output) and hangs it on a model's standardised output as a differentiable term (`design_objective_term`): with the
optimiser's own objective of the label as the per-sample divisor the term is the optimality ratio L(I_pred) / L(I_opt).  Rows are
sample-major (load case c of sample b is beam row b*C + c); the term is four launches -- `ops_design_loss_prep`, the float64
`beam_solve`, dL/dI of every row through it (`sizing._beam_sizing_grad_launch`, both exactly as the sizing loop uses them) and
`ops_design_loss_finish` (csrc/design_loss.hip).  Shared geometry only: x [N], fix [N], scalar E and wy.  GPU only.
"""
from __future__ import annotations

import ctypes
import types
from typing import Dict, NamedTuple, Optional, Sequence

import torch

from . import _cabi
from .beam import beam_solve
from .sizing import SizingConfig, _beam_sizing_grad_launch, sizing_tiling
from .sizing_common import _ptr, checked_aggregate, checked_objective

I_MIN = 1e-8        # the floor of a predicted inertia (train.py, physics.py: clamp_min(1e-8))


class DesignObjective(NamedTuple):
    value: torch.Tensor          # [B] float64   L_b
    grad: torch.Tensor           # [B, Ne] float64   dL_b / dI_b
    case_penalty: torch.Tensor   # [B, C] float64   P_c
    governing: torch.Tensor      # [B] int32   the governing case ("sum": the lowest index of the largest w_c P_c)
    status: torch.Tensor         # [B] int32   non-zero: a row of the sample failed in the solve or the gradient (its value, grad: NaN)


def _checked(aggregate, weights, C, alpha_deflection, deflection_limit, dev):
    """(aggregate index, weights on the device or None, alpha_deflection, deflection_limit), refused as the C entry would."""
    agg, _ = checked_aggregate(aggregate, weights)          # its name; the weights' values after the objective and the case count
    _, aD, vlim = checked_objective("total", (("deflection", alpha_deflection, deflection_limit),))
    if C < 1 or C > _cabi.load().ops_design_loss_max_cases():
        raise ValueError(f"n_load_cases must be in [1, {_cabi.load().ops_design_loss_max_cases()}], got {C}")
    _, w = checked_aggregate(aggregate, weights, C)
    return agg, None if w is None else torch.as_tensor(w, dtype=torch.float64, device=dev), aD, vlim


def _shared(x, fix, E, wy, Ne, dev):
    """x [N] float64, fix [N] uint8, E and wy 0-dim float64, all on `dev` (device tensors pass through: nothing is copied inside a
    captured step)."""
    x = torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
    fix = torch.as_tensor(fix, dtype=torch.uint8, device=dev).contiguous()
    for name, t in (("x", x), ("fix", fix)):
        if tuple(t.shape) != (Ne + 1,):
            raise ValueError(f"{name} must be [{Ne + 1}] (shared by the batch), got {tuple(t.shape)}")
    E, wy = (torch.as_tensor(t, dtype=torch.float64, device=dev) for t in (E, wy))
    if E.numel() != 1 or wy.numel() != 1:
        raise ValueError("E and wy must be scalars (shared by the batch)")
    return x, fix, E.reshape(()), wy.reshape(())


def _hp(hp):
    return hp.c_params() if isinstance(hp, SizingConfig) else hp


def _middle(a, x, E, fix, wy, hp, aD, vlim, I_rows, Fy_rows):
    """The two unchanged launches on the B*C rows; their outputs into the argument struct.  Returns what must stay alive."""
    dev = I_rows.device
    R, Ne = I_rows.shape
    sol = beam_solve(x, E, I_rows, fix, Fy_rows, wy, tiling=sizing_tiling(Ne + 1, shared_geometry=False))
    grad = torch.empty((R, Ne), dtype=torch.float64, device=dev)
    extra = torch.empty((R,), dtype=torch.float64, device=dev) if aD > 0.0 else None
    gstatus = torch.empty((R,), dtype=torch.int32, device=dev)
    obj = _cabi.SizingObjective(alpha_deflection=aD, deflection_limit=vlim)
    _beam_sizing_grad_launch(x, E, I_rows, fix, wy, sol, hp, obj, None, grad, extra, gstatus)
    a.V, a.M, a.grad, a.loss_extra = sol.V.data_ptr(), sol.M.data_ptr(), grad.data_ptr(), _ptr(extra)
    a.status_solve, a.status_grad = sol.status.data_ptr(), gstatus.data_ptr()
    a.alpha_deflection, a.deflection_limit = aD, vlim
    return sol, grad, extra, gstatus


def _finish(a, hp, dev):
    with torch.cuda.device(dev):
        rc = _cabi.load().ops_design_loss_finish(ctypes.byref(a), ctypes.byref(hp), torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_design_loss_finish")


def design_objective(I, x, E, fix, Fy, wy, hp, *, n_load_cases: int = 1, aggregate: str = "sum",
                     weights: Optional[Sequence[float]] = None, alpha_deflection: float = 0.0,
                     deflection_limit: Optional[float] = None) -> DesignObjective:
    """The sizing objective of B designs I [B, Ne] float64, each under its C = `n_load_cases` load cases Fy [B, C, N], and its
    gradient through the solve: the solve and the gradient launch on the B*C rows, then `ops_design_loss_finish`.  `hp`: a
    `SizingConfig` or an `ops_sizing_params`; `aggregate`, `weights`, `alpha_deflection`, `deflection_limit` as in
    `optimize_designs`.  x [N], fix [N], scalar E and wy are shared by the batch.  Asynchronous on the current stream."""
    if not torch.is_tensor(I) or not I.is_cuda:
        raise RuntimeError("design_objective needs GPU tensors: openpystruct_amd has no CPU fallback")
    dev = I.device
    if I.dtype != torch.float64 or I.dim() != 2:
        raise ValueError("I must be a float64 [B, Ne] tensor")
    B, Ne = I.shape
    C, N = int(n_load_cases), Ne + 1
    if Ne < 1 or Ne > 512:
        raise ValueError(f"design_objective serves 1 to 512 elements per beam, got {Ne}")
    agg, w, aD, vlim = _checked(aggregate, weights, C, alpha_deflection, deflection_limit, dev)
    Fy = torch.as_tensor(Fy, dtype=torch.float64, device=dev).contiguous()
    if tuple(Fy.shape) != (B, C, N):
        raise ValueError(f"Fy must be [{B}, {C}, {N}], got {tuple(Fy.shape)}")
    x, fix, E, wy = _shared(x, fix, E, wy, Ne, dev)
    hp = _hp(hp)
    f64 = dict(dtype=torch.float64, device=dev)
    out = DesignObjective(torch.empty((B,), **f64), torch.empty((B, Ne), **f64), torch.empty((B, C), **f64),
                          torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))
    if B == 0:
        return out
    I_rows = I.contiguous().repeat_interleave(C, dim=0)
    a = _cabi.DesignLossArgs(B=B, C=C, Ne=Ne, G=B, aggregate=agg, weight=1.0, weights=_ptr(w), I_rows=I_rows.data_ptr(),
                             sample_loss=out.value.data_ptr(), gI=out.grad.data_ptr(), case_penalty=out.case_penalty.data_ptr(),
                             governing=out.governing.data_ptr())
    sol, _grad, _extra, gstatus = _middle(a, x, E, fix, wy, hp, aD, vlim, I_rows, Fy.reshape(B * C, N))
    _finish(a, hp, dev)
    torch.amax(((sol.status != 0) | (gstatus != 0)).to(torch.int32).reshape(B, C), dim=1, out=out.status)
    return out


def _term_launches(preds, spec) -> types.SimpleNamespace:
    """The four launches of the term on the current stream: everything they wrote, and what their pointers refer to."""
    lib = _cabi.load()
    (nel, sI, rows, Fy, x, E, fix, wy, hp, weight, agg, w, aD, vlim, ref, acc) = spec
    dev = preds.device
    if preds.dtype not in (torch.float32, torch.bfloat16) or preds.dim() != 2 or preds.stride(1) != 1:
        raise ValueError("predictions must be a [B, C] float32 or bfloat16 matrix with unit column stride")
    B, Ne, N = int(preds.shape[0]), nel, nel + 1
    if preds.shape[1] < Ne or (B > 1 and preds.stride(0) < Ne):
        raise ValueError(f"predictions must have at least {Ne} columns (and a row stride of at least that), got {tuple(preds.shape)}")
    if Fy.dim() != 3 or Fy.shape[2] != N or Fy.dtype != torch.float64 or Fy.device != dev or not Fy.is_contiguous():
        raise ValueError(f"Fy_cases must be a contiguous float64 [G, C, {N}] tensor on the predictions' device")
    G, C = int(Fy.shape[0]), int(Fy.shape[1])
    if G < 1 or (rows is None and G < B):
        raise ValueError("Fy_cases must have G >= the batch rows (or `rows` given)")
    if rows is not None and (rows.dtype != torch.int64 or rows.device != dev or rows.dim() != 1 or rows.numel() < B or not rows.is_contiguous()):
        raise ValueError("rows must be a contiguous int64 vector on the predictions' device with one entry per sample")
    if ref is not None and (ref.dtype != torch.float64 or ref.device != dev or tuple(ref.shape) != (G,) or not ref.is_contiguous()):
        raise ValueError(f"ref must be a contiguous float64 [{G}] tensor on the predictions' device")
    if acc is not None and (acc.dtype != torch.float32 or acc.device != dev or acc.numel() != 1):
        raise ValueError("acc must be a float32 device scalar")
    f64 = dict(dtype=torch.float64, device=dev)
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
    scale, mean = f32(sI.scale_), f32(sI.mean_)
    if scale.numel() < Ne or mean.numel() < Ne:
        raise ValueError(f"the inertia scaler must have at least {Ne} columns")
    o = types.SimpleNamespace(
        I_rows=torch.empty((B * C, Ne), **f64), Fy_rows=torch.empty((B * C, N), **f64), sample_loss=torch.empty((B,), **f64),
        gI=torch.empty((B, Ne), **f64), case_penalty=torch.empty((B, C), **f64), governing=torch.empty((B,), dtype=torch.int32, device=dev),
        part=torch.empty((int(lib.ops_design_loss_part_doubles(B)),), **f64), value=torch.empty((), dtype=torch.float32, device=dev),
        # (the launch reads the predictions and writes their gradient with ONE row stride: the gradient takes the predictions' strides)
        dpreds=torch.empty_strided(preds.shape, preds.stride(), dtype=preds.dtype, device=dev))
    if preds.shape[1] != Ne:
        o.dpreds.zero_()
    ldp = int(preds.stride(0)) if B > 1 else max(int(preds.stride(0)), Ne)
    a = _cabi.DesignLossArgs(B=B, C=C, Ne=Ne, G=G, aggregate=agg, preds_bf16=int(preds.dtype == torch.bfloat16), ldp=ldp,
                             preds=preds.data_ptr(), I_scale=scale.data_ptr(), I_mean=mean.data_ptr(), I_min=I_MIN, weight=float(weight),
                             rows=_ptr(rows), Fy_src=Fy.data_ptr(), ref=_ptr(ref), weights=_ptr(w), I_rows=o.I_rows.data_ptr(),
                             Fy_rows=o.Fy_rows.data_ptr(), sample_loss=o.sample_loss.data_ptr(), gI=o.gI.data_ptr(),
                             case_penalty=o.case_penalty.data_ptr(), governing=o.governing.data_ptr(), dpreds=o.dpreds.data_ptr(),
                             part=o.part.data_ptr(), value=o.value.data_ptr(), value_sum=_ptr(acc))
    if B == 0:
        o.value.zero_()
        return o
    with torch.cuda.device(dev):
        rc = lib.ops_design_loss_prep(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_design_loss_prep")
    o.keep = _middle(a, x, E, fix, wy, hp, aD, vlim, o.I_rows, o.Fy_rows) + (scale, mean, preds, rows, Fy, ref, w, acc)
    _finish(a, hp, dev)
    return o


class _DesignObjectiveTerm(torch.autograd.Function):
    """The term's value from four launches in `forward`; `backward` hands out the gradient they already wrote."""

    @staticmethod
    def forward(ctx, preds, spec):
        o = _term_launches(preds.detach(), spec)
        ctx.dpreds = o.dpreds
        return o.value

    @staticmethod
    def backward(ctx, go):
        return ctx.dpreds, None


def _term_spec(dev, nel, sI, rows, Fy_cases, x, E, fix, wy, hp, weight, aggregate, weights, alpha_deflection, deflection_limit, ref, acc):
    """The checked, device-resident argument tuple of `_DesignObjectiveTerm` (train._DesignInputs builds it once per run and swaps
    the rows in per step: nothing here runs inside a captured step)."""
    nel = int(nel)
    if nel < 1 or nel > 512:
        raise ValueError(f"design_objective_term serves 1 to 512 elements per beam, got {nel}")
    if not torch.is_tensor(Fy_cases) or Fy_cases.dim() != 3:
        raise ValueError(f"Fy_cases must be a [G, C, {nel + 1}] tensor")
    agg, w, aD, vlim = _checked(aggregate, weights, int(Fy_cases.shape[1]), alpha_deflection, deflection_limit, dev)
    x, fix, E, wy = _shared(x, fix, E, wy, nel, dev)
    return (nel, sI, rows, Fy_cases, x, E, fix, wy, _hp(hp), float(weight), agg, w, aD, vlim, ref, acc)


def design_objective_term(preds, nel, sI, rows, Fy_cases, x, E, fix, wy, hp, weight, *, aggregate: str = "sum",
                          weights: Optional[Sequence[float]] = None, alpha_deflection: float = 0.0,
                          deflection_limit: Optional[float] = None, ref: Optional[torch.Tensor] = None,
                          acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """weight * mean_b L(I_b) / ref_b with I_b = clamp_min(sI^-1(preds[b, :nel]), 1e-8) under the C load cases
    Fy_cases[rows[b]] ([G, C, N] float64; rows int64 [B], None: row b) and ref_b = ref[rows[b]] ([G] float64, None: 1 -- with the
    optimiser's objective of the label the term is the mean optimality ratio): four launches in the forward pass, none in the
    backward pass.  The value enters the total with weight ONE (the gradient ignores the incoming one); `acc`: float32 device scalar
    the value is added to.  A sample with a NaN prediction or a failed solve makes the value NaN and gets a NaN gradient row.
    Shared geometry: x [N], fix [N], scalars E, wy (device tensors inside a captured step).  `hp`: a `SizingConfig` or an
    `ops_sizing_params`."""
    if not torch.is_tensor(preds) or not preds.is_cuda:
        raise RuntimeError("design_objective_term needs GPU tensors: openpystruct_amd has no CPU fallback")
    spec = _term_spec(preds.device, nel, sI, rows, Fy_cases, x, E, fix, wy, hp, weight, aggregate, weights, alpha_deflection,
                      deflection_limit, ref, acc)
    return _DesignObjectiveTerm.apply(preds, spec)


def design_gap(model, data, term, split: str = "val") -> Dict[str, float]:
    """How far the designs a trained surrogate predicts are from its labels IN OBJECTIVE: L(I_pred) / L(I_label) - 1 over the
    samples of `split` ("val" or "train"), both sides through `design_objective` under the sample's load cases
    (`data.Fy_cases_val` / `data.Fy_cases_train`) with the settings of `term` (a `train.DesignTerm`).  Returns mean, median and
    max over the samples that solved, and `failed`: the count of those that did not (either side non-finite or a failed row)."""
    if split not in ("val", "train"):
        raise ValueError(f"split must be 'val' or 'train', got {split!r}")
    X, Y, Fy = (data.X_val, data.Y_val, data.Fy_cases_val) if split == "val" else (data.X_train, data.Y_train, data.Fy_cases_train)
    if Fy is None:
        raise ValueError("design_gap needs the per-case loads (data.Fy_cases_*: records with force_nodes and force_values)")
    dev = next(model.parameters()).device
    sI = data.scalers_Y["I"]
    nel = int(sI.mean_.numel())
    was_training = model.training
    model.eval()
    with torch.no_grad():
        preds = torch.cat([model(X[i:i + 512].to(dev)).float() for i in range(0, X.shape[0], 512)])
    model.train(was_training)
    I_of = lambda t: sI.inverse_transform(t[:, :nel].float()).clamp_min(I_MIN).double()      # noqa: E731
    kw = dict(n_load_cases=int(Fy.shape[1]), aggregate=term.aggregate, weights=term.weights, alpha_deflection=term.alpha_deflection,
              deflection_limit=term.deflection_limit)
    Fy = Fy.to(dev)
    got = design_objective(I_of(preds), term.x, term.E, term.fix, Fy, term.wy, term.hp, **kw)
    want = design_objective(I_of(Y.to(dev)), term.x, term.E, term.fix, Fy, term.wy, term.hp, **kw)
    gap = got.value / want.value - 1.0
    ok = torch.isfinite(gap) & (got.status == 0) & (want.status == 0)
    good = gap[ok]
    nan = float("nan")
    return {"mean": float(good.mean()) if good.numel() else nan, "median": float(good.median()) if good.numel() else nan,
            "max": float(good.max()) if good.numel() else nan, "failed": int((~ok).sum()), "samples": int(gap.numel())}
