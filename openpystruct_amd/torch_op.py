"""`torch.ops.openpystruct_amd.beam_solve`: the batched solve as a registered PyTorch operator (SURVEY.md 8b:
"called from (i) the torch.library custom op and (ii) the ops shim").

Registered for the GPU dispatch key only -- CPU tensors raise NotImplementedError, there is no CPU kernel --
plus a fake (meta) implementation, so the op can sit inside `torch.compile` / FakeTensor shape propagation and
HIP-graph capture without touching the kernel.  E and wy are tensors here (0-dim/1-element = shared scalar).

The op is differentiable: its autograd formula calls a second registered op,
`openpystruct_amd::beam_solve_vjp` (csrc/beam_vjp.hip, with a fake implementation of its own), so forward and backward
both trace under FakeTensor / `torch.compile` and capture into HIP graphs.  Gradients reach I, E, Fy and wy; a shared
scalar E or wy receives the sum over all elements.  status is not differentiable; x and fix get no gradient, and x
requiring one is an error rather than a silent None."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .beam import beam_solve, beam_solve_vjp

T = torch.Tensor


@torch.library.custom_op("openpystruct_amd::beam_solve", mutates_args=(), device_types="cuda")
def beam_solve_op(x: T, E: T, I: T, fix: T, Fy: T, wy: T, tiling: int = 0) -> Tuple[T, T, T, T, T]:
    s = beam_solve(x, E, I, fix, Fy, wy, tiling=tiling)
    return s.v, s.theta, s.V, s.M, s.status


@beam_solve_op.register_fake
def _(x, E, I, fix, Fy, wy, tiling=0):
    B, Ne = I.shape
    return (I.new_empty((B, Ne + 1)), I.new_empty((B, Ne + 1)), I.new_empty((B, Ne)), I.new_empty((B, Ne)),
            I.new_empty((B,), dtype=torch.int32))


@torch.library.custom_op("openpystruct_amd::beam_solve_vjp", mutates_args=(), device_types="cuda")
def beam_solve_vjp_op(x: T, E: T, I: T, fix: T, wy: T, v: T, theta: T, gv: Optional[T], gt: Optional[T],
                      gV: Optional[T], gM: Optional[T]) -> Tuple[T, T, T, T]:
    return beam_solve_vjp(x, E, I, fix, wy, v, theta, gv, gt, gV, gM)


@beam_solve_vjp_op.register_fake
def _(x, E, I, fix, wy, v, theta, gv, gt, gV, gM):
    B, Ne = I.shape
    return I.new_empty((B, Ne)), I.new_empty((B, Ne + 1)), I.new_empty((B, Ne)), I.new_empty((B,), dtype=torch.int32)


def _setup_context(ctx, inputs, output):
    x, E, I, fix, Fy, wy, tiling = inputs
    v, theta, V, M, status = output
    if x.requires_grad:
        raise ValueError("openpystruct_amd::beam_solve: node coordinates are not differentiable (x requires grad); "
                         "gradients flow to I, E, Fy and wy only")
    ctx.mark_non_differentiable(status)
    ctx.save_for_backward(x, E, I, fix, wy, v, theta)


def _backward(ctx, gv, gt, gV, gM, gstatus):
    x, E, I, fix, wy, v, theta = ctx.saved_tensors
    gI, gFy, gwy, _ = torch.ops.openpystruct_amd.beam_solve_vjp(x, E, I, fix, wy, v, theta, gv, gt, gV, gM)
    gE = None
    if ctx.needs_input_grad[1]:   # k_e is linear in E_e I_e: dL/dE_e = gI_e I_e / E_e
        gE = gI * I / E if E.numel() != 1 else ((gI * I).sum() / E.reshape(())).reshape(E.shape)
    if ctx.needs_input_grad[5] and wy.numel() == 1:
        gwy = gwy.sum().reshape(wy.shape)
    return (None, gE, gI if ctx.needs_input_grad[2] else None, None, gFy if ctx.needs_input_grad[4] else None,
            gwy if ctx.needs_input_grad[5] else None, None)


beam_solve_op.register_autograd(_backward, setup_context=_setup_context)
