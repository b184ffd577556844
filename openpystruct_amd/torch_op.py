"""`torch.ops.openpystruct_amd.beam_solve`: the batched solve as a registered PyTorch operator (SURVEY.md 8b:
"called from (i) the torch.library custom op and (ii) the ops shim").

Registered for the GPU dispatch key only -- CPU tensors raise NotImplementedError, there is no CPU kernel --
plus a fake (meta) implementation, so the op can sit inside `torch.compile` / FakeTensor shape propagation and
HIP-graph capture without touching the kernel.  E and wy are tensors here (0-dim/1-element = shared scalar).

The op is differentiable: its autograd formula calls a second registered op,
`openpystruct_amd::beam_solve_vjp` (csrc/beam_vjp.hip, with a fake implementation of its own), so forward and backward
both trace under FakeTensor / `torch.compile` and capture into HIP graphs.  Gradients reach I, E, Fy and wy; a shared
scalar E or wy receives the sum over all elements.  status is not differentiable; x and fix get no gradient, and x
requiring one is an error rather than a silent None.

`torch.ops.openpystruct_amd.frame_solve` / `frame_solve_vjp` are the same pair for the frame solve (DESIGN.md §9f,
csrc/frame_vjp.hip).  Operator arguments are tensors and ints: the inertias, the loads and the
integer under which the `FrameTopology` -- whose arrays and per-stream workspaces the solve uses -- is registered here, and
its node count (the output shapes of the fake implementation); `frame_solve_autograd` (= `frames.differentiable_frame_solve`) fills them
in.  Gradients reach I and loads; status is not differentiable.

`torch.ops.openpystruct_amd.frame_solve_loads` / `frame_solve_loads_vjp` are that pair with the element loads as one more tensor
argument ([Ne,2] shared or [B,Ne,2]: DESIGN.md §9i, csrc/frame_loads.hip); gradients reach them too.

`torch.ops.openpystruct_amd.frame_eigenvalues` / `frame_eigenvalues_vjp` are the lowest eigenvalues of K(I) phi = lambda M phi
(`frame_modes.differentiable_frame_frequencies`); gradients reach I, the mode shapes carry none.

`torch.ops.openpystruct_amd.frame_buckling_factors` / `frame_buckling_factors_vjp` are the lowest critical load factors of
K(I) phi = lambda S(N) phi under the topology's own loads (`frame_buckling.differentiable_frame_buckling`); gradients
reach I through the direct term and one adjoint re-solve on a factorisation of the backward's own."""
from __future__ import annotations

import itertools
import math
import weakref
from typing import Optional, Tuple

import torch

from . import frames
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


# ---- the frame solve ----
# A FrameTopology is host state (numpy arrays, the workspaces per stream): the operators name it by an integer, valid while the object lives.
_topologies = weakref.WeakValueDictionary()
_topology_ids = itertools.count(1)


def _topology_id(topo: frames.FrameTopology) -> int:
    tid = topo.__dict__.get("_op_id")
    if tid is None:
        tid = topo.__dict__["_op_id"] = next(_topology_ids)
        _topologies[tid] = topo
    return tid


def _topology(tid: int) -> frames.FrameTopology:
    topo = _topologies.get(tid)
    if topo is None:
        raise RuntimeError(f"openpystruct_amd::frame_solve: no live FrameTopology is registered as {tid}")
    return topo


# The two forward operators (with and without the element loads as an argument) share their body, their fake implementation,
# their context setup and the core of their backward; their arguments end in (n_nodes, topology).
def _frame_solve(name: str, I: T, loads: T, element_loads: Optional[T], n_nodes: int, topology: int) -> Tuple[T, T, T, T, T]:
    topo = _topology(topology)
    if n_nodes != topo.Nn:
        raise ValueError(f"openpystruct_amd::{name}: n_nodes = {n_nodes}, the topology registered as {topology} has {topo.Nn}")
    s = frames.frame_solve(topo, I, loads, element_loads=element_loads)
    return s.disp, s.forces, s.V, s.M, s.status


def _frame_solve_fake(I, *args):
    B, Ne = I.shape
    return (I.new_empty((B, args[-2], 3)), I.new_empty((B, Ne, 6)), I.new_empty((B, Ne)), I.new_empty((B, Ne)),
            I.new_empty((B,), dtype=torch.int32))


def _frame_setup_context(ctx, inputs, output):
    ctx.mark_non_differentiable(output[4])
    ctx.save_for_backward(inputs[0], output[0], output[4])
    # the operators name the topology by an integer that is valid while the object lives: the graph keeps it alive
    ctx.topo, ctx.topology = _topologies.get(inputs[-1]), inputs[-1]
    ctx.shared = [False] + [t.dim() == 2 for t in inputs[1:-2]]      # per tensor input: one load set for the batch


def _frame_backward(ctx, vjp_op, g_disp, g_forces, gV, gM, gstatus):
    """The VJP operator returns (gI, g_loads[, g_w], status), the load gradients per frame: a shared input receives the sum over the frames."""
    I, disp, status = ctx.saved_tensors
    grads = vjp_op(I, disp, status, g_disp, g_forces, gV, gM, ctx.topology)[:-1]
    return tuple((g.sum(0) if shared else g) if need else None
                 for g, shared, need in zip(grads, ctx.shared, ctx.needs_input_grad)) + (None, None)


@torch.library.custom_op("openpystruct_amd::frame_solve", mutates_args=(), device_types="cuda")
def frame_solve_op(I: T, loads: T, n_nodes: int, topology: int) -> Tuple[T, T, T, T, T]:
    return _frame_solve("frame_solve", I, loads, None, n_nodes, topology)


@torch.library.custom_op("openpystruct_amd::frame_solve_vjp", mutates_args=(), device_types="cuda")
def frame_solve_vjp_op(I: T, disp: T, status: Optional[T], g_disp: Optional[T], g_forces: Optional[T], gV: Optional[T],
                       gM: Optional[T], topology: int) -> Tuple[T, T, T]:
    return frames.frame_solve_vjp(_topology(topology), I, disp, g_disp, g_forces, gV, gM, status)


@frame_solve_vjp_op.register_fake
def _(I, disp, status, g_disp, g_forces, gV, gM, topology):
    return I.new_empty(I.shape), disp.new_empty(disp.shape), I.new_empty((I.shape[0],), dtype=torch.int32)


# ---- the frame solve under per-call element loads ----
@torch.library.custom_op("openpystruct_amd::frame_solve_loads", mutates_args=(), device_types="cuda")
def frame_solve_loads_op(I: T, loads: T, element_loads: T, n_nodes: int, topology: int) -> Tuple[T, T, T, T, T]:
    return _frame_solve("frame_solve_loads", I, loads, element_loads, n_nodes, topology)


@torch.library.custom_op("openpystruct_amd::frame_solve_loads_vjp", mutates_args=(), device_types="cuda")
def frame_solve_loads_vjp_op(I: T, disp: T, status: Optional[T], g_disp: Optional[T], g_forces: Optional[T], gV: Optional[T],
                             gM: Optional[T], topology: int) -> Tuple[T, T, T, T]:
    """(gI, g_loads per frame, g_w per frame, the adjoint solve's status): `frame_solve_vjp` -- neither gI nor g_loads depends on the
    element loads -- and one more launch for g_w."""
    topo = _topology(topology)
    gI, lam, st = frames.frame_solve_vjp(topo, I, disp, g_disp, g_forces, gV, gM, status)
    return gI, lam, frames.frame_element_load_vjp(topo, lam, g_forces, gV, gM, status, st), st


@frame_solve_loads_vjp_op.register_fake
def _(I, disp, status, g_disp, g_forces, gV, gM, topology):
    B, Ne = I.shape
    return I.new_empty(I.shape), disp.new_empty(disp.shape), I.new_empty((B, Ne, 2)), I.new_empty((B,), dtype=torch.int32)


for _op, _vjp in ((frame_solve_op, "frame_solve_vjp"), (frame_solve_loads_op, "frame_solve_loads_vjp")):
    _op.register_fake(_frame_solve_fake)
    _op.register_autograd(lambda ctx, *g, _vjp=_vjp: _frame_backward(ctx, getattr(torch.ops.openpystruct_amd, _vjp), *g),
                          setup_context=_frame_setup_context)


def frame_solve_autograd(topo: frames.FrameTopology, I: T, loads: Optional[T] = None,
                         element_loads: Optional[T] = None) -> frames.FrameSolution:
    if loads is None:
        loads = topo.d_loads
    if element_loads is not None:
        return frames.FrameSolution(*torch.ops.openpystruct_amd.frame_solve_loads(I, loads, element_loads, topo.Nn, _topology_id(topo)))
    return frames.FrameSolution(*torch.ops.openpystruct_amd.frame_solve(I, loads, topo.Nn, _topology_id(topo)))


# ---- eigenvalues of K(I) phi = lambda M phi ----
# A FrameMass is host state as a FrameTopology is: named by an integer, valid while the object lives.
_masses = weakref.WeakValueDictionary()


def _mass_id(mass) -> int:
    mid = mass.__dict__.get("_op_id")
    if mid is None:
        mid = mass.__dict__["_op_id"] = next(_topology_ids)
        _masses[mid] = mass
    return mid


@torch.library.custom_op("openpystruct_amd::frame_eigenvalues", mutates_args=(), device_types="cuda")
def frame_eigenvalues_op(I: T, X0: Optional[T], n_modes: int, n_vectors: int, iters: int, tol: float, max_iters: int, poll_every: int,
                         n_nodes: int, topology: int, mass: int) -> Tuple[T, T, T]:
    """(eigenvalues [B,m], shapes [B,m,Nn,3], status [B]) of `frame_modes.frame_solve_modes`; n_vectors = 0: its default, iters = 0:
    run to `tol`."""
    from .frame_modes import frame_solve_modes
    topo, ms = _topology(topology), _masses.get(mass)
    if ms is None:
        raise RuntimeError(f"openpystruct_amd::frame_eigenvalues: no live FrameMass is registered as {mass}")
    if n_nodes != topo.Nn:
        raise ValueError(f"openpystruct_amd::frame_eigenvalues: n_nodes = {n_nodes}, the topology registered as {topology} has {topo.Nn}")
    r = frame_solve_modes(topo, I.contiguous(), ms, n_modes=n_modes, n_vectors=n_vectors or None, iters=iters or None, tol=tol,
                        max_iters=max_iters, poll_every=poll_every, X0=X0)
    return r.eigenvalues, r.shapes, r.status


@frame_eigenvalues_op.register_fake
def _(I, X0, n_modes, n_vectors, iters, tol, max_iters, poll_every, n_nodes, topology, mass):
    B = I.shape[0]
    return I.new_empty((B, n_modes)), I.new_empty((B, n_modes, n_nodes, 3)), I.new_empty((B,), dtype=torch.int32)


@torch.library.custom_op("openpystruct_amd::frame_eigenvalues_vjp", mutates_args=(), device_types="cuda")
def frame_eigenvalues_vjp_op(shapes: T, status: T, g_eigenvalues: T, topology: int) -> T:
    from .frame_modes import _modes_grad
    return _modes_grad(_topology(topology), shapes, status, g_eigenvalues)


@frame_eigenvalues_vjp_op.register_fake
def _(shapes, status, g_eigenvalues, topology):
    return shapes.new_empty((shapes.shape[0], _topology(topology).Ne))


def _eigenvalues_setup_context(ctx, inputs, output):
    ctx.mark_non_differentiable(output[1], output[2])          # the shapes carry no gradient
    ctx.save_for_backward(output[1], output[2])
    ctx.topo, ctx.mass, ctx.topology = _topologies.get(inputs[-2]), _masses.get(inputs[-1]), inputs[-2]


def _eigenvalues_backward(ctx, g_eig, g_shapes, g_status):
    shapes, status = ctx.saved_tensors
    gI = torch.ops.openpystruct_amd.frame_eigenvalues_vjp(shapes, status, g_eig.contiguous(), ctx.topology) if ctx.needs_input_grad[0] else None
    return (gI,) + (None,) * 10


frame_eigenvalues_op.register_autograd(_eigenvalues_backward, setup_context=_eigenvalues_setup_context)


def frame_frequencies_autograd(topo: frames.FrameTopology, I: T, mass, n_modes: int = 1, n_vectors: Optional[int] = None,
                               iters: Optional[int] = None, tol: float = 1e-10, max_iters: int = 64, poll_every: int = 4,
                               X0: Optional[T] = None):
    from .frame_modes import FrameMass      # (the package's attribute `frame_modes` is the function of that name)
    if not isinstance(mass, FrameMass) or mass.topo is not topo:
        raise ValueError("mass must be a FrameMass of this topology")
    if not torch.is_tensor(I) or I.dtype != torch.float64 or I.dim() != 2 or I.shape[1] != topo.Ne:
        raise ValueError(f"I must be float64 [B, {topo.Ne}]")
    if not I.is_cuda:
        raise RuntimeError("differentiable_frame_frequencies needs GPU tensors: openpystruct_amd has no CPU fallback")
    eig, _, _ = torch.ops.openpystruct_amd.frame_eigenvalues(I, X0, int(n_modes), int(n_vectors or 0), int(iters or 0), float(tol), int(max_iters),
                                                             int(poll_every), topo.Nn, _topology_id(topo), _mass_id(mass))
    return eig, torch.sqrt(eig) / (2.0 * math.pi)


# ---- load factors of K(I) phi = lambda S(N) phi ----
@torch.library.custom_op("openpystruct_amd::frame_buckling_factors", mutates_args=(), device_types="cuda")
def frame_buckling_factors_op(I: T, X0: Optional[T], n_modes: int, consistent: int, n_vectors: int, iters: int, tol: float, max_iters: int,
                              poll_every: int, n_nodes: int, topology: int) -> Tuple[T, T, T]:
    """(load_factors [B,m], shapes [B,m,Nn,3], status [B]) of `frame_buckling.frame_solve_buckling` under the topology's own loads;
    consistent = 0: the P-Delta matrix, n_vectors = 0: its default, iters = 0: run to `tol`."""
    from .frame_buckling import frame_solve_buckling
    topo = _topology(topology)
    if n_nodes != topo.Nn:
        raise ValueError(f"openpystruct_amd::frame_buckling_factors: n_nodes = {n_nodes}, the topology registered as {topology} has {topo.Nn}")
    r = frame_solve_buckling(topo, I.contiguous(), n_modes=n_modes, kind="consistent" if consistent else "pdelta", n_vectors=n_vectors or None,
                             iters=iters or None, tol=tol, max_iters=max_iters, poll_every=poll_every, X0=X0)
    return r.load_factors, r.shapes, r.status


@frame_buckling_factors_op.register_fake
def _(I, X0, n_modes, consistent, n_vectors, iters, tol, max_iters, poll_every, n_nodes, topology):
    B = I.shape[0]
    return I.new_empty((B, n_modes)), I.new_empty((B, n_modes, n_nodes, 3)), I.new_empty((B,), dtype=torch.int32)


@torch.library.custom_op("openpystruct_amd::frame_buckling_factors_vjp", mutates_args=(), device_types="cuda")
def frame_buckling_factors_vjp_op(I: T, load_factors: T, shapes: T, status: T, g_load_factors: T, consistent: int, topology: int) -> T:
    """gI [B,Ne]: the keeping solve once more (the reference state and the factor the adjoint re-solve runs on), then
    `frame_buckling.frame_buckling_vjp`."""
    from .frame_buckling import FrameBuckling, frame_buckling_vjp
    fac = frames.frame_factor(_topology(topology), I.contiguous())
    res = FrameBuckling(load_factors, None, shapes, None, 0, status, fac.solution, "consistent" if consistent else "pdelta")
    return frame_buckling_vjp(fac, res, g_load_factors)[0]


@frame_buckling_factors_vjp_op.register_fake
def _(I, load_factors, shapes, status, g_load_factors, consistent, topology):
    return I.new_empty(I.shape)


def _buckling_setup_context(ctx, inputs, output):
    ctx.mark_non_differentiable(output[1], output[2])          # the shapes carry no gradient
    ctx.save_for_backward(inputs[0], *output)
    ctx.topo, ctx.topology, ctx.consistent = _topologies.get(inputs[-1]), inputs[-1], inputs[3]


def _buckling_backward(ctx, g_lam, g_shapes, g_status):
    I, lam, shapes, status = ctx.saved_tensors
    gI = None
    if ctx.needs_input_grad[0]:
        gI = torch.ops.openpystruct_amd.frame_buckling_factors_vjp(I, lam, shapes, status, g_lam.contiguous(), ctx.consistent, ctx.topology)
    return (gI,) + (None,) * 10


frame_buckling_factors_op.register_autograd(_buckling_backward, setup_context=_buckling_setup_context)


def frame_buckling_autograd(topo: frames.FrameTopology, I: T, n_modes: int = 1, kind: str = "consistent", n_vectors: Optional[int] = None,
                            iters: Optional[int] = None, tol: float = 1e-10, max_iters: int = 64, poll_every: int = 4,
                            X0: Optional[T] = None) -> T:
    from .frame_buckling import KINDS
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}")
    if not torch.is_tensor(I) or I.dtype != torch.float64 or I.dim() != 2 or I.shape[1] != topo.Ne:
        raise ValueError(f"I must be float64 [B, {topo.Ne}]")
    if not I.is_cuda:
        raise RuntimeError("differentiable_frame_buckling needs GPU tensors: openpystruct_amd has no CPU fallback")
    lam, _, _ = torch.ops.openpystruct_amd.frame_buckling_factors(I, X0, int(n_modes), int(kind == "consistent"), int(n_vectors or 0),
                                                                  int(iters or 0), float(tol), int(max_iters), int(poll_every), topo.Nn,
                                                                  _topology_id(topo))
    return lam
