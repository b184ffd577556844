"""Batched 2-D frame analysis and sizing: the host side of SURVEY 8(f1) / BASELINE config 5.

Mirrors /root/reference/OpenPyStruct_FrameOpt_Discrete_Beta.py:
  * grid geometry, element order (columns first, then beams), supports, loads   FR:50-69, :75-139 -> `grid_frame`
  * `setup_frame_model` + `ops.analyze(1)` + `ops.eleResponse(e,'forces')`        FR:75-139, :151, :181-183 -> `frame_solve`
  * loss (bending eps 1e-8, "shear" = global Fy even for columns), Adam without a scheduler, early stop
                                                                                  FR:141-206 -> `optimize_frames`
One topology (coordinates, connectivity, constraints) is prepared once on the host -- equation numbers as
OpenSees' PlainHandler + a node-order numberer would give them, half bandwidth -- and shared by the batch;
frames differ in their inertia vectors (and optionally loads).  The solve is the HIP kernel in
csrc/frame_solve.hip behind `ops_frame_solve_batched_f64`; there is no CPU path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _cabi
from .sizing_common import (GRADIENTS, _ptr, _sizing_step, _StepState, arm_optimiser_state, checked_objective,  # noqa: F401  (GRADIENTS: public here)
                            history_callback, new_optimiser_state, run_epochs)


@dataclass
class FrameConfig:
    """FR:17-44."""
    bay_width: float = 6.0
    story_height: float = 3.0
    E: float = 200e9
    nu: float = 0.3
    A: float = 0.02
    I0: float = 5e-4
    alpha_moment: float = 1e-2
    alpha_shear: float = 1e-2
    k: float = 0.03
    lateral_load: float = 1e4
    vertical_load: float = -1e4
    num_epochs: int = 5000
    lr: float = 0.005
    tolerance: float = 1e-3
    patience: int = 10

    @property
    def G(self):
        return self.E / (2 * (1 + self.nu))


def rcm_node_order(n_nodes: int, conn: np.ndarray, has_eq: np.ndarray) -> np.ndarray:
    """Reverse Cuthill-McKee order of the nodes that carry equations (what `ops.numberer('RCM')`, FR:135 / SC:121, asks OpenSees
    for): breadth-first levels from a pseudo-peripheral node (George-Liu: repeat from a minimum-degree node of the last level
    while the eccentricity grows), neighbours by increasing degree, the whole order reversed; components one after the other.
    Nodes without equations (fully fixed) keep their place at the end -- they number nothing."""
    adj = [set() for _ in range(n_nodes)]
    for a, b in conn:
        a, b = int(a), int(b)
        if a != b and has_eq[a] and has_eq[b]:
            adj[a].add(b); adj[b].add(a)
    deg = np.array([len(s) for s in adj])
    todo = set(int(i) for i in np.nonzero(has_eq)[0])

    def levels(root):
        seen, order, frontier, depth = {root}, [root], [root], 0
        while frontier:
            nxt = []
            for u in frontier:
                for v in sorted(adj[u] - seen, key=lambda w: (deg[w], w)):
                    seen.add(v); nxt.append(v)
            if not nxt:
                break
            order += nxt; frontier = nxt; depth += 1
        return order, frontier, depth

    out = []
    while todo:
        root = min(todo, key=lambda w: (deg[w], w))
        order, last, depth = levels(root)
        while True:
            cand = min(last, key=lambda w: (deg[w], w))
            o2, l2, d2 = levels(cand)
            if d2 <= depth:
                break
            root, order, last, depth = cand, o2, l2, d2
        out += order[::-1]
        todo -= set(order)
    return np.array(out + [int(i) for i in np.nonzero(~has_eq)[0]], dtype=np.int64)


def _number_equations(order: np.ndarray, fix3: np.ndarray, conn: np.ndarray):
    """Equation numbers node by node along `order` (constrained DOFs get none: constraints('Plain')), and the half bandwidth."""
    node_eq = -np.ones(fix3.shape, dtype=np.int32)
    k = 0
    for nd in order:
        for dof in range(3):
            if not fix3[nd, dof]:
                node_eq[nd, dof] = k
                k += 1
    elem_eq = np.concatenate([node_eq[conn[:, 0]], node_eq[conn[:, 1]]], axis=1)
    span = [int(q[q >= 0].max() - q[q >= 0].min()) for q in elem_eq if (q >= 0).any()]
    return node_eq, elem_eq, (max(span) if span else 0)


class FrameTopology:
    """Shared description of a frame: what `setup_frame_model` rebuilds every epoch, minus the inertias.

    `numbering`: "node" = equations in node order (what r01-r04 did: row by row on a grid); "rcm" = reverse Cuthill-McKee (the
    reference's `numberer('RCM')`, FR:135); "auto" (default) = the narrowest of node order, reverse Cuthill-McKee and the two
    coordinate sweeps (`self.numbering` says which), node order on a tie.  The solution does not depend on it beyond rounding; the work does (n kd^2): a 10-bay x 2-story frame of the reference's own
    random range is kd 35 story by story and kd 8 along its column lines, and a 21 x 3 frame (kd 68 in node order: beyond the
    tuned kernels' 63, i.e. on the slow column-by-column fallback) stays on the wave kernel."""

    def __init__(self, coords, conn, fix3, A, E, wy, wx, nodal_loads, device="cuda", numbering: str = "auto"):
        coords = np.asarray(coords, dtype=np.float64)
        conn = np.asarray(conn, dtype=np.int64)
        fix3 = np.asarray(fix3).astype(bool)
        self.Nn, self.Ne = coords.shape[0], conn.shape[0]
        d = coords[conn[:, 1]] - coords[conn[:, 0]]
        L = np.hypot(d[:, 0], d[:, 1])
        geo = np.stack([L, d[:, 0] / L, d[:, 1] / L], axis=1)
        if numbering not in ("auto", "node", "rcm"):
            raise ValueError("numbering must be 'auto', 'node' or 'rcm'")
        node_eq, elem_eq, kd = _number_equations(np.arange(self.Nn), fix3, conn)
        self.numbering = "node"
        if numbering == "rcm":
            node_eq, elem_eq, kd = _number_equations(rcm_node_order(self.Nn, conn, ~fix3.all(axis=1)), fix3, conn)
            self.numbering = "rcm"
        elif numbering == "auto":
            # candidates: reverse Cuthill-McKee, and the two coordinate sweeps (nodes sorted by (x, y) / by (y, x): on a rectangular grid
            # the sweep along the shorter side is the optimum, which the breadth-first levels of RCM -- diagonals of the grid -- miss)
            cands = [("rcm", rcm_node_order(self.Nn, conn, ~fix3.all(axis=1))),
                     ("sweep-x", np.lexsort((coords[:, 1], coords[:, 0]))), ("sweep-y", np.lexsort((coords[:, 0], coords[:, 1])))]
            for name, order in cands:
                c_node_eq, c_elem_eq, c_kd = _number_equations(order, fix3, conn)
                if c_kd < kd:
                    node_eq, elem_eq, kd, self.numbering = c_node_eq, c_elem_eq, c_kd, name
        self.n_eq, self.kd = int((~fix3).sum()), kd
        Ev = np.broadcast_to(np.asarray(E, dtype=np.float64), (self.Ne,))
        Av = np.broadcast_to(np.asarray(A, dtype=np.float64), (self.Ne,))
        w = np.stack([np.broadcast_to(np.asarray(wy, dtype=np.float64), (self.Ne,)),
                      np.broadcast_to(np.asarray(wx, dtype=np.float64), (self.Ne,))], axis=1)
        self.coords, self.conn, self.fix3 = coords, conn, fix3
        self.A, self.E, self.wy, self.wx = Av.copy(), Ev.copy(), w[:, 0].copy(), w[:, 1].copy()
        self.nodal_loads = np.asarray(nodal_loads, dtype=np.float64).reshape(self.Nn, 3)
        dev = torch.device(device)
        t = lambda a, dt: torch.as_tensor(np.array(a), dtype=dt, device=dev)  # noqa: E731
        self.device = dev
        self.d_geo, self.d_EA, self.d_E, self.d_w = t(geo, torch.float64), t(Ev * Av, torch.float64), t(Ev, torch.float64), t(w, torch.float64)
        self.d_elem_eq, self.d_node_eq = t(elem_eq, torch.int32), t(node_eq, torch.int32)
        self.d_loads = t(self.nodal_loads, torch.float64)

    def lds_bytes(self) -> int:
        n3, ld = (self.n_eq + 2) // 3 * 3, (max(self.kd, 3) + 4) & ~1     # csrc/frame_solve.hip: frame_n3, frame_ld
        return (n3 * ld + n3) * 8


def grid_frame(num_bays: int, num_stories: int, cfg: Optional[FrameConfig] = None, device="cuda", numbering: str = "auto") -> FrameTopology:
    """The reference's rectangular frame (FR:50-69, :84-131): nodes row by row from the ground, columns then
    beams, ground row fully fixed, lateral loads on the left column line, beamUniform(w, w) on the beams."""
    cfg = cfg or FrameConfig()
    nb1 = num_bays + 1
    coords = np.array([(j * cfg.bay_width, i * cfg.story_height) for i in range(num_stories + 1) for j in range(nb1)])
    cols = [(i * nb1 + j, (i + 1) * nb1 + j) for i in range(num_stories) for j in range(nb1)]                  # FR:101-107
    beams = [(i * nb1 + j, i * nb1 + j + 1) for i in range(1, num_stories + 1) for j in range(num_bays)]      # FR:110-116
    conn = np.array(cols + beams)
    fix3 = np.zeros((coords.shape[0], 3), dtype=bool)
    fix3[coords[:, 1] == 0.0] = True                                                                           # FR:96-98
    loads = np.zeros((coords.shape[0], 3))
    loads[(coords[:, 0] == 0.0) & (coords[:, 1] != 0.0), 0] = cfg.lateral_load                                 # FR:126-128
    w = np.zeros(len(conn)); w[len(cols):] = cfg.vertical_load                                                 # FR:130-131 (Wy = Wx)
    return FrameTopology(coords, conn, fix3, cfg.A, cfg.E, w, w, loads, device, numbering=numbering)


class FrameSolution(NamedTuple):
    disp: torch.Tensor      # [B, Nn, 3]
    forces: torch.Tensor    # [B, Ne, 6]  eleResponse(e, 'forces')
    V: torch.Tensor         # [B, Ne]     forces[..., 1]  (FR:152)
    M: torch.Tensor         # [B, Ne]     forces[..., 2]  (FR:153)
    status: torch.Tensor    # [B] int32


def _checked(name: str, t, dtype, shape: tuple, dev=None, *, gpu_for: str = "", optional: bool = False, in_place: bool = False):
    """The one tensor check of this module: `t`, contiguous, if it is a `dtype` tensor of `shape` (None: any batch size) on `dev` (None:
    wherever it is), else ValueError.  `gpu_for`: the entry's name -- anything but a GPU tensor is a RuntimeError.  `optional`: None
    passes as None.  `in_place`: the caller uses `t`'s own memory, so a tensor that is not contiguous is refused rather than copied."""
    if t is None and optional:
        return None
    if gpu_for and (not torch.is_tensor(t) or not t.is_cuda):
        raise RuntimeError(f"{gpu_for} needs GPU tensors: openpystruct_amd has no CPU fallback")
    fits = t.dim() == len(shape) and all(want is None or want == have for want, have in zip(shape, t.shape))
    if t.dtype != dtype or (dev is not None and t.device != dev) or not fits or (in_place and not t.is_contiguous()):
        what = f"{str(dtype).split('.')[-1]} [{', '.join('B' if n is None else str(n) for n in shape)}]"
        raise ValueError(f"{name} must be {'contiguous ' if in_place else ''}{what}" + (f" on {dev}" if dev is not None else ""))
    return t.contiguous()


def frame_solve(topo: FrameTopology, I: torch.Tensor, loads: Optional[torch.Tensor] = None,
                out: Optional[FrameSolution] = None, element_loads: Optional[torch.Tensor] = None) -> FrameSolution:
    """`element_loads`: float64 [Ne,2] or [B,Ne,2] (wy, wx) REPLACES the topology's `wy` / `wx` for this call, per frame when it has
    a batch dimension (three launches -- the right-hand side with the consistent loads, the solve without element
    loads on a workspace of its own, the correction of the forces); None: the topology's element loads, one launch."""
    I = _checked("I", I, torch.float64, (None, topo.Ne), gpu_for="frame_solve")
    B = I.shape[0]
    dev = I.device
    if loads is None:
        loads, lbs = topo.d_loads, 0
    else:
        loads = loads.to(torch.float64).contiguous()
        lbs = topo.Nn * 3 if loads.dim() == 3 else 0
    if element_loads is not None:
        w, wbs = _checked_element_loads(topo, element_loads, B, dev)
        _check_nodal_loads(topo, loads, B, dev)
    if out is None:
        out = _empty_solution(topo, B, dev)
    if element_loads is not None:
        _element_load_launches(topo, I, loads, lbs, w, wbs, torch.empty((B, topo.Nn, 3), dtype=torch.float64, device=dev), out)
        return out
    _run_solve(topo, I, loads, lbs, out, topo.d_w, "_ws")
    return out


def _checked_element_loads(topo: FrameTopology, w, B: int, dev) -> tuple:
    """(contiguous element loads, their batch stride) of an `element_loads` argument for B frames on `dev`."""
    if not torch.is_tensor(w) or not w.is_cuda:
        raise RuntimeError("element_loads must be a GPU tensor: openpystruct_amd has no CPU fallback")
    if w.dtype != torch.float64 or w.device != dev or tuple(w.shape) not in ((topo.Ne, 2), (B, topo.Ne, 2)):
        raise ValueError(f"element_loads must be float64 [{topo.Ne}, 2] or [{B}, {topo.Ne}, 2] (wy, wx) on {dev}")
    return w.contiguous(), (2 * topo.Ne if w.dim() == 3 else 0)


def _check_nodal_loads(topo: FrameTopology, loads: torch.Tensor, B: int, dev) -> None:
    if loads.device != dev or tuple(loads.shape) not in ((topo.Nn, 3), (B, topo.Nn, 3)):
        raise ValueError(f"loads must be [{topo.Nn}, 3] or [{B}, {topo.Nn}, 3] on {dev}")


def _element_load_launches(topo: FrameTopology, I: torch.Tensor, loads: torch.Tensor, lbs: int, w: torch.Tensor, wbs: int,
                           rhs: torch.Tensor, out: FrameSolution) -> None:
    """The three launches of a solve under element loads `w` on the current stream (csrc/frame_loads.hip around the solve without
    element loads); no checks, no allocation beyond what `_run_solve` keeps per stream.  The workspaces are this
    path's own (`_ws_loads`): a cached plan holds the consistent loads of the element loads it was built with."""
    lib = _cabi.load()
    dev, B = I.device, I.shape[0]
    adj = _adjoint_tables(topo)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.ops_frame_load_rhs_f64(B, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(),
                                        loads.data_ptr(), lbs, w.data_ptr(), wbs, rhs.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_load_rhs_f64")
    _run_solve(topo, I, rhs, topo.Nn * 3, out, adj.zero_w, "_ws_loads")
    with torch.cuda.device(dev):
        rc = lib.ops_frame_load_forces_f64(B, topo.Ne, topo.d_geo.data_ptr(), w.data_ptr(), wbs, out.status.data_ptr(),
                                           out.forces.data_ptr(), out.V.data_ptr(), out.M.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_load_forces_f64")


def _empty_solution(topo: FrameTopology, B: int, dev) -> FrameSolution:
    f64 = dict(dtype=torch.float64, device=dev)
    return FrameSolution(torch.empty((B, topo.Nn, 3), **f64), torch.empty((B, topo.Ne, 6), **f64),
                         torch.empty((B, topo.Ne), **f64), torch.empty((B, topo.Ne), **f64),
                         torch.empty((B,), dtype=torch.int32, device=dev))


def _run_solve(topo: FrameTopology, I: torch.Tensor, loads: torch.Tensor, lbs: int, out: FrameSolution, d_w: torch.Tensor,
               cache_name: str) -> None:
    """One call of the solve on the current stream, with the workspace and plan bookkeeping.  `cache_name`: the attribute of the
    topology that keeps the workspaces of solves with this `d_w` -- the plan holds the consistent loads of the element loads
    (csrc/frame_wave.hpp frame_plan_kernel: rhs_base), so a plan is kept only for the element loads it was built with."""
    lib = _cabi.load()
    B, dev = I.shape[0], I.device
    ws_bytes = int(lib.ops_frame_workspace_bytes(B, topo.n_eq, topo.kd))
    ws, flags, entry = None, 0, None
    if ws_bytes:       # factor storage + the topology's assembly plan: HBM workspace, cached on the topology PER STREAM (two solves on one
        # topology from different streams or threads must not share factor columns or plan)
        cache = topo.__dict__.setdefault(cache_name, {})
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        entry = cache.get(key)
        if entry is None or entry[0].numel() < ws_bytes:
            entry = cache[key] = [torch.empty(ws_bytes, dtype=torch.uint8, device=dev), 0]
        ws = entry[0]
        # the plan (the topology-only part of the assembly, at the start of the workspace) is built by the first call that uses this buffer and
        # kept: a FrameTopology's arrays never change (include/openpystruct_amd.h OPS_FRAME_REUSE_PLAN)
        sig = int(lib.ops_frame_plan_signature(B, topo.n_eq, topo.kd))
        if sig != 0 and entry[1] == sig:
            flags = _cabi.FRAME_REUSE_PLAN
    with torch.cuda.device(dev):
        rc = lib.ops_frame_solve_batched_f64_ex(
            B, topo.Nn, topo.Ne, topo.n_eq, topo.kd, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(),
            d_w.data_ptr(), topo.d_elem_eq.data_ptr(), topo.d_node_eq.data_ptr(), I.data_ptr(), loads.data_ptr(), lbs,
            out.disp.data_ptr(), out.forces.data_ptr(), out.V.data_ptr(), out.M.data_ptr(), out.status.data_ptr(),
            ws.data_ptr() if ws is not None else None, ws_bytes, torch.cuda.current_stream(dev).cuda_stream, flags)
    if entry is not None:
        entry[1] = sig if rc == _cabi.OK else 0
    if rc == _cabi.ERR_UNSUPPORTED:
        raise NotImplementedError(f"frame too large: n_eq={topo.n_eq}, half bandwidth={topo.kd} (half bandwidth <= 63: a (kd+6)-column ring, one "
                                  f"n_eq vector and two 24-column chunks must fit 160 KB of LDS; beyond 63, up to 1024: one n_eq vector and one column)")
    _cabi.check(rc, "ops_frame_solve_batched_f64")


class _AdjointTables(NamedTuple):
    conn: torch.Tensor         # [Ne,2] int32
    ptr: torch.Tensor          # [Nn+1] int32
    idx: torch.Tensor          # [2 Ne] int32: 2 * element + end, per node in element order
    zero_w: torch.Tensor       # [Ne,2] float64 zeros: the adjoint solve has no element loads


def _adjoint_tables(topo: FrameTopology) -> _AdjointTables:
    """What the VJP needs beyond the forward's arrays, built once per topology and kept on it (as `_ws` is)."""
    t = topo.__dict__.get("_adj")
    if t is None:
        if topo.conn.min() < 0 or topo.conn.max() >= topo.Nn:
            raise ValueError("conn names a node that does not exist")
        ends = np.argsort(topo.conn.reshape(-1), kind="stable")          # entry 2 e + end of conn: sorted by node, element order within
        ptr = np.zeros(topo.Nn + 1, dtype=np.int64)
        np.cumsum(np.bincount(topo.conn.reshape(-1), minlength=topo.Nn), out=ptr[1:])
        mk = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=topo.device)  # noqa: E731
        t = topo.__dict__["_adj"] = _AdjointTables(mk(topo.conn, torch.int32), mk(ptr, torch.int32), mk(ends, torch.int32),
                                                   torch.zeros((topo.Ne, 2), dtype=torch.float64, device=topo.device))
    return t


def frame_solve_vjp(topo: FrameTopology, I: torch.Tensor, disp: torch.Tensor, g_disp: Optional[torch.Tensor] = None,
                    g_forces: Optional[torch.Tensor] = None, gV: Optional[torch.Tensor] = None, gM: Optional[torch.Tensor] = None,
                    status: Optional[torch.Tensor] = None):
    """Vector-Jacobian product of `frame_solve`: given the forward's `disp` [B,Nn,3] and the cotangents of disp
    [B,Nn,3], forces [B,Ne,6], V and M [B,Ne] (None = zero), returns (gI [B,Ne], g_loads [B,Nn,3] per frame, status [B] int32).
    Three launches on the current stream: the adjoint right-hand side, the solve once more (K is symmetric; its own workspace, no
    element loads), the per-element contraction (csrc/frame_vjp.hip).  A frame whose factorisation fails has status != 0 and NaN rows;
    `status` [B] int32: the forward's status, when given a frame that failed there gets a NaN gI row whatever its `disp` holds."""
    lib = _cabi.load()
    I = _checked("I", I, torch.float64, (None, topo.Ne), gpu_for="frame_solve_vjp")
    B, dev = I.shape[0], I.device
    if disp is None:
        raise ValueError("disp: the forward's displacements are needed")
    disp, g_disp = (_checked(k, v, torch.float64, (B, topo.Nn, 3), dev, optional=True) for k, v in (("disp", disp), ("g_disp", g_disp)))
    g_forces, gV, gM = _checked_cotangents(topo, B, dev, g_forces, gV, gM)
    status = _checked("status", status, torch.int32, (B,), dev, optional=True)
    adj = _adjoint_tables(topo)
    rhs = torch.empty((B, topo.Nn, 3), dtype=torch.float64, device=dev)
    gI = torch.empty((B, topo.Ne), dtype=torch.float64, device=dev)
    if B == 0:
        return gI, rhs, torch.empty((0,), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        rc = lib.ops_frame_adjoint_rhs_f64(B, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(),
                                           adj.conn.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(), I.data_ptr(), _ptr(g_disp),
                                           _ptr(g_forces), _ptr(gV), _ptr(gM), rhs.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_adjoint_rhs_f64")
    sol = _empty_solution(topo, B, dev)                     # disp = lambda; the adjoint's forces, V, M are not used
    _run_solve(topo, I, rhs, topo.Nn * 3, sol, adj.zero_w, "_ws_adjoint")
    with torch.cuda.device(dev):
        rc = lib.ops_frame_grad_contract_f64(B, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(),
                                             disp.data_ptr(), sol.disp.data_ptr(), _ptr(g_forces), _ptr(gV), _ptr(gM), _ptr(status),
                                             sol.status.data_ptr(), gI.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_grad_contract_f64")
    return gI, sol.disp, sol.status


def _checked_cotangents(topo: FrameTopology, B: int, dev, g_forces, gV, gM) -> tuple:
    """The optional cotangents of the element results: forces [B,Ne,6], V and M [B,Ne]."""
    return (_checked("g_forces", g_forces, torch.float64, (B, topo.Ne, 6), dev, optional=True),
            _checked("gV", gV, torch.float64, (B, topo.Ne), dev, optional=True),
            _checked("gM", gM, torch.float64, (B, topo.Ne), dev, optional=True))


def frame_element_load_vjp(topo: FrameTopology, lam: torch.Tensor, g_forces: Optional[torch.Tensor] = None,
                           gV: Optional[torch.Tensor] = None, gM: Optional[torch.Tensor] = None,
                           status: Optional[torch.Tensor] = None, status_adj: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of a loss with respect to per-frame element loads: g_w [B,Ne,2] (wy, wx) from `lam` [B,Nn,3], the
    `g_loads` that `frame_solve_vjp` returns for the same cotangents, and the cotangents of forces [B,Ne,6], V and M [B,Ne] (None =
    zero).  One launch on the current stream (csrc/frame_loads.hip).  `status` / `status_adj` [B] int32: the forward's and the
    adjoint solve's; a frame with a non-zero one gets a NaN row.  Element loads shared by the batch take the sum over the frames."""
    lib = _cabi.load()
    lam = _checked("lam", lam, torch.float64, (None, topo.Nn, 3), gpu_for="frame_element_load_vjp")
    B, dev = lam.shape[0], lam.device
    g_forces, gV, gM = _checked_cotangents(topo, B, dev, g_forces, gV, gM)
    status, status_adj = (_checked(k, v, torch.int32, (B,), dev, optional=True) for k, v in (("status", status), ("status_adj", status_adj)))
    adj = _adjoint_tables(topo)
    g_w = torch.empty((B, topo.Ne, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.ops_frame_load_vjp_f64(B, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), adj.conn.data_ptr(), lam.data_ptr(), _ptr(g_forces),
                                        _ptr(gV), _ptr(gM), _ptr(status), _ptr(status_adj), g_w.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_frame_load_vjp_f64")
    return g_w


class FrameCaseSolution(NamedTuple):
    """`FrameSolution` with a case axis behind the batch axis."""
    disp: torch.Tensor      # [B, C, Nn, 3]
    forces: torch.Tensor    # [B, C, Ne, 6]
    V: torch.Tensor         # [B, C, Ne]     forces[..., 1]
    M: torch.Tensor         # [B, C, Ne]     forces[..., 2]
    status: torch.Tensor    # [B, C] int32


class FrameFactor:
    """The factorisation K(I) = L D L^T of B frames, kept on the device by `frame_factor` for `frame_resolve`.
    `topo`; `I` [B,Ne]: the CALLER'S tensor, not a copy -- the force recovery of every re-solve reads it, so it must hold the values
    that were factorised for as long as the factor is used; `workspace`: the kept buffer (uint8); `solution`: the `FrameSolution` of
    the keeping solve, under the topology's own loads; `status` [B] int32 = `solution.status` (non-zero: that frame's factorisation
    failed and every re-solve of it is NaN).  Buffers that re-solves need beyond their outputs are kept here by shape."""

    def __init__(self, topo: FrameTopology, I: torch.Tensor, workspace: torch.Tensor, solution: FrameSolution):
        self.topo, self.I, self.workspace, self.solution, self.status = topo, I, workspace, solution, solution.status
        self._scratch = {}

    def _buffer(self, name: str, shape: tuple, dtype=torch.float64) -> torch.Tensor:
        t = self._scratch.get((name, shape))
        if t is None:
            t = self._scratch[(name, shape)] = torch.empty(shape, dtype=dtype, device=self.I.device)
        return t


def frame_factor(topo: FrameTopology, I: torch.Tensor) -> FrameFactor:
    """Solves the B frames under the topology's own loads, as `frame_solve(topo, I)` does (equal to its tolerances, not bit for bit:
    always the wave-per-frame kernel), and KEEPS every frame's factorisation: (n_eq + 4) * W doubles per frame, W = 36 / 52 / 56 for
    half bandwidths up to 35 / 51 / 55.  Served: half bandwidth <= 55 and frames whose four waves fit the LDS of a compute unit;
    anything else is a ValueError (`frame_solve` serves every shape).  `I` is kept by reference (see `FrameFactor`)."""
    if torch.is_tensor(I) and (I.dtype != torch.float64 or I.dim() != 2 or I.shape[1] != topo.Ne):
        raise ValueError(f"I must be contiguous float64 [B, {topo.Ne}]")
    I = _checked("I", I, torch.float64, (None, topo.Ne), gpu_for="frame_factor", in_place=True)
    lib = _cabi.load()
    B, dev = I.shape[0], I.device
    nbytes = int(lib.ops_frame_factor_workspace_bytes(max(B, 1), topo.n_eq, topo.kd))
    if nbytes == 0:
        raise ValueError(f"frame_factor keeps the factor of the wave-per-frame kernel only: half bandwidth <= 55 (this topology: {topo.kd}) and "
                         f"four waves' LDS within 160 KB (n_eq = {topo.n_eq}); use frame_solve, which serves every shape")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sol = _empty_solution(topo, B, dev)
    with torch.cuda.device(dev):
        rc = lib.ops_frame_factor_solve_f64(
            B, topo.Nn, topo.Ne, topo.n_eq, topo.kd, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(),
            topo.d_w.data_ptr(), topo.d_elem_eq.data_ptr(), topo.d_node_eq.data_ptr(), I.data_ptr(), topo.d_loads.data_ptr(), 0,
            sol.disp.data_ptr(), sol.forces.data_ptr(), sol.V.data_ptr(), sol.M.data_ptr(), sol.status.data_ptr(),
            ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_frame_factor_solve_f64")
    return FrameFactor(topo, I, ws, sol)


def _empty_case_solution(topo: FrameTopology, B: int, C: int, dev) -> FrameCaseSolution:
    f64 = dict(dtype=torch.float64, device=dev)
    return FrameCaseSolution(torch.empty((B, C, topo.Nn, 3), **f64), torch.empty((B, C, topo.Ne, 6), **f64),
                             torch.empty((B, C, topo.Ne), **f64), torch.empty((B, C, topo.Ne), **f64),
                             torch.empty((B, C), dtype=torch.int32, device=dev))


def _checked_cases(name: str, t, B: int, tail: tuple, dev, gpu_for: str, shape_only: bool = False) -> torch.Tensor:
    """A per-case input: float64 [B,C,*tail] or [C,*tail] (shared by the frames) on `dev`, contiguous.  Shape and dtype first
    (ValueError), then where it lives (anything but a GPU tensor: RuntimeError)."""
    dims = ", ".join(str(n) for n in tail)
    ok = torch.is_tensor(t) and t.dtype == torch.float64 and t.dim() in (len(tail) + 1, len(tail) + 2) and tuple(t.shape[-len(tail):]) == tail
    if not ok or (t.dim() == len(tail) + 2 and t.shape[0] != B):
        raise ValueError(f"{name} must be float64 [{B}, C, {dims}] or [C, {dims}]")
    if shape_only:
        return t
    if not t.is_cuda or not dev.type == "cuda":
        raise RuntimeError(f"{gpu_for} needs GPU tensors: openpystruct_amd has no CPU fallback")
    if t.device != dev:
        raise ValueError(f"{name} must be on {dev}, where the factor is")
    return t.contiguous()


def _resolve_launch(factor: FrameFactor, C: int, rhs: torch.Tensor, rhs_bs: int, out: FrameCaseSolution) -> None:
    """ops_frame_resolve_f64 on the current stream: K(I_b) x = rhs[b, c], forces without element loads, into `out`."""
    lib = _cabi.load()
    topo, I = factor.topo, factor.I
    with torch.cuda.device(I.device):
        rc = lib.ops_frame_resolve_f64(
            I.shape[0], C, topo.Nn, topo.Ne, topo.n_eq, topo.kd, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(),
            topo.d_elem_eq.data_ptr(), topo.d_node_eq.data_ptr(), I.data_ptr(), rhs.data_ptr(), rhs_bs, factor.status.data_ptr(),
            out.disp.data_ptr(), out.forces.data_ptr(), out.V.data_ptr(), out.M.data_ptr(), out.status.data_ptr(),
            factor.workspace.data_ptr(), factor.workspace.numel(), torch.cuda.current_stream(I.device).cuda_stream)
    _cabi.check(rc, "ops_frame_resolve_f64")


def frame_resolve(factor: FrameFactor, loads: torch.Tensor, element_loads: Optional[torch.Tensor] = None,
                  out: Optional[FrameCaseSolution] = None) -> FrameCaseSolution:
    """C load cases per frame on the kept factorisation, by substitution alone.  `loads`: float64 [B,C,Nn,3], or
    [C,Nn,3] shared by the frames; `element_loads`: float64 [B,C,Ne,2] or [C,Ne,2] (wy, wx), None = the topology's `wy` / `wx` in
    every case, as in `frame_solve`.  Three launches on the current stream, as `frame_solve(..., element_loads=)`: the right-hand
    sides with the consistent loads, ONE re-solve launch for all B * C rows, the correction of the forces.  Case (b, c) depends on
    frame b's factor and its own loads alone -- not on B, C or its position; a frame whose factorisation failed is NaN with status 1
    in every case.  With `out` (a `FrameCaseSolution` of this shape) nothing is allocated after the first call of a shape: the
    right-hand sides, and the replica of a shared `element_loads` (the correction of the forces runs on all B * C rows) or of
    shared `loads` beside per-frame `element_loads` (one copy launch each), live in buffers kept on the factor."""
    topo, I = factor.topo, factor.I
    B, dev = I.shape[0], I.device
    for name, t, tail in (("loads", loads, (topo.Nn, 3)), ("element_loads", element_loads, (topo.Ne, 2))):      # every shape before any device
        if t is not None:
            _checked_cases(name, t, B, tail, dev, "frame_resolve", shape_only=True)
    if element_loads is not None and element_loads.shape[-3] != loads.shape[-3]:
        raise ValueError(f"element_loads has {element_loads.shape[-3]} cases, loads has {loads.shape[-3]}")
    loads = _checked_cases("loads", loads, B, (topo.Nn, 3), dev, "frame_resolve")
    C = loads.shape[-3]
    w = None if element_loads is None else _checked_cases("element_loads", element_loads, B, (topo.Ne, 2), dev, "frame_resolve")
    if out is None:
        out = _empty_case_solution(topo, B, C, dev)
    else:
        want = _empty_case_solution(topo, 0, C, dev)
        for name, t, ref in zip(FrameCaseSolution._fields, out, want):
            _checked(f"out.{name}", t, ref.dtype, (B,) + tuple(ref.shape[1:]), dev, in_place=True)
    if B == 0 or C == 0:
        return out
    lib = _cabi.load()
    adj = _adjoint_tables(topo)
    # the rows the two streaming kernels work on: all B * C, or the C shared ones where nothing differs between the frames
    shared = loads.dim() == 3 and (w is None or w.dim() == 3)
    if loads.dim() == 3 and not shared:
        loads = factor._buffer("loads_rows", (B, C, topo.Nn, 3)).copy_(loads.expand(B, C, topo.Nn, 3))
    w_rows, wbs = (topo.d_w, 0) if w is None else (w, 2 * topo.Ne)
    if w is not None and w.dim() == 3:            # the correction of the forces runs on all B * C rows
        w_rows = factor._buffer("w_rows", (B, C, topo.Ne, 2)).copy_(w.expand(B, C, topo.Ne, 2))
    rows = C if shared else B * C
    rhs = factor._buffer("rhs", (rows, topo.Nn, 3))
    w_rhs = w if (shared and w is not None) else w_rows
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.ops_frame_load_rhs_f64(rows, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(),
                                        loads.data_ptr(), 3 * topo.Nn, w_rhs.data_ptr(), wbs, rhs.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_load_rhs_f64")
    _resolve_launch(factor, C, rhs, 0 if shared else C * topo.Nn * 3, out)
    with torch.cuda.device(dev):
        rc = lib.ops_frame_load_forces_f64(B * C, topo.Ne, topo.d_geo.data_ptr(), w_rows.data_ptr(), wbs, out.status.data_ptr(),
                                           out.forces.data_ptr(), out.V.data_ptr(), out.M.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_load_forces_f64")
    return out


def frame_solve_cases(topo: FrameTopology, I: torch.Tensor, loads: torch.Tensor,
                      element_loads: Optional[torch.Tensor] = None) -> FrameCaseSolution:
    """`frame_resolve(frame_factor(topo, I), loads, element_loads)`: B designs under C load cases each with ONE factorisation per
    design, where `frame_solve` on the B * C rows (I repeated per case) factorises K(I) C times.
    Measured (one MI355X, medians of three rounds, profiles/frame_cases_timing.json), time of `frame_solve` on the
    rows over the time of this call at C = 1 / 2 / 4 / 8: 15 x 16 x 3072 designs 0.67 / 1.11 / 1.72 / 2.27, 10 x 10 x 4096 0.66 / 1.13 /
    1.59 / 2.22, 5 x 5 x 8192 0.30 / 0.47 / 0.80 / 1.11.  So it LOSES at C = 1 (a factorisation plus a substitution that reads the
    factor back) and on small frames up to C = 4, where `frame_solve` runs the packed kernel and this call the wave-per-frame one;
    nothing here chooses between the two for the caller."""
    return frame_resolve(frame_factor(topo, I), loads, element_loads)


def frame_solve_cases_vjp(factor: FrameFactor, sol: FrameCaseSolution, g_disp: Optional[torch.Tensor] = None,
                          g_forces: Optional[torch.Tensor] = None, gV: Optional[torch.Tensor] = None, gM: Optional[torch.Tensor] = None):
    """Vector-Jacobian product of `frame_resolve`: from its solution `sol` and the cotangents of disp [B,C,Nn,3],
    forces [B,C,Ne,6], V and M [B,C,Ne] (None = zero, bit for bit) returns (gI [B,Ne], g_loads [B,C,Nn,3], g_element_loads
    [B,C,Ne,2]).  The adjoint displacements of all B * C rows come from ONE re-solve launch on the kept factor -- no factorisation:
    the adjoint right-hand side (on the rows, with `I` repeated per case: the one copy this makes), the re-solve, the contraction
    and the element-load VJP on the rows, then gI as the sum over the case axis in index order.  g_loads and g_element_loads are
    per (frame, case): an input shared by the frames takes their sum over the frames.  Rows of failed frames are NaN."""
    topo, I = factor.topo, factor.I
    B, dev = I.shape[0], I.device
    disp = _checked("sol.disp", sol.disp, torch.float64, (B, None, topo.Nn, 3), dev)
    C = disp.shape[1]
    st_fwd = _checked("sol.status", sol.status, torch.int32, (B, C), dev)
    g_disp = _checked("g_disp", g_disp, torch.float64, (B, C, topo.Nn, 3), dev, optional=True)
    g_forces = _checked("g_forces", g_forces, torch.float64, (B, C, topo.Ne, 6), dev, optional=True)
    gV, gM = (_checked(k, v, torch.float64, (B, C, topo.Ne), dev, optional=True) for k, v in (("gV", gV), ("gM", gM)))
    if not I.is_cuda:
        raise RuntimeError("frame_solve_cases_vjp needs GPU tensors: openpystruct_amd has no CPU fallback")
    lib = _cabi.load()
    f64 = dict(dtype=torch.float64, device=dev)
    gI = torch.empty((B, topo.Ne), **f64)
    g_w = torch.empty((B, C, topo.Ne, 2), **f64)
    lam = _empty_case_solution(topo, B, C, dev)               # disp = lambda; the adjoint's forces, V, M are not used
    if B == 0 or C == 0:
        return gI.zero_(), lam.disp, g_w
    adj = _adjoint_tables(topo)
    R = B * C
    I_rows = I.repeat_interleave(C, 0)
    rhs = torch.empty((B, C, topo.Nn, 3), **f64)
    gI_rows = torch.empty((B, C, topo.Ne), **f64)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.ops_frame_adjoint_rhs_f64(R, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(),
                                           adj.conn.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(), I_rows.data_ptr(), _ptr(g_disp),
                                           _ptr(g_forces), _ptr(gV), _ptr(gM), rhs.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_adjoint_rhs_f64")
    _resolve_launch(factor, C, rhs, C * topo.Nn * 3, lam)
    with torch.cuda.device(dev):
        rc = lib.ops_frame_grad_contract_f64(R, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(),
                                             disp.data_ptr(), lam.disp.data_ptr(), _ptr(g_forces), _ptr(gV), _ptr(gM), st_fwd.data_ptr(),
                                             lam.status.data_ptr(), gI_rows.data_ptr(), stream)
        _cabi.check(rc, "ops_frame_grad_contract_f64")
        rc = lib.ops_frame_load_vjp_f64(R, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), adj.conn.data_ptr(), lam.disp.data_ptr(), _ptr(g_forces),
                                        _ptr(gV), _ptr(gM), st_fwd.data_ptr(), lam.status.data_ptr(), g_w.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_load_vjp_f64")
    gI.copy_(gI_rows[:, 0])
    for c in range(1, C):                                      # the case axis in index order
        gI += gI_rows[:, c]
    return gI, lam.disp, g_w


def differentiable_frame_solve(topo: FrameTopology, I: torch.Tensor, loads: Optional[torch.Tensor] = None,
                               element_loads: Optional[torch.Tensor] = None) -> FrameSolution:
    """`frame_solve` through the registered operator `openpystruct_amd::frame_solve` (torch_op.py): gradients reach I and, when
    given, loads ([Nn,3] shared or [B,Nn,3]); status is not differentiable.  The graph keeps `topo` alive until it is freed.
    With `element_loads` ([Ne,2] shared or [B,Ne,2]) it is the operator `openpystruct_amd::frame_solve_loads`, whose gradients reach
    the element loads too; a shared input receives the sum over the frames."""
    from . import torch_op
    return torch_op.frame_solve_autograd(topo, I, loads, element_loads)


def _objective(gradient: str, alpha_sway: float, sway_limit: Optional[float], alpha_deflection: float,
               deflection_limit: Optional[float]) -> tuple:
    """The checked (gradient, alpha_sway, sway_limit, alpha_deflection, deflection_limit) of a frame sizing run.  "explicit": the
    reference's gradient (M and V held fixed), which cannot see a displacement term; "total": the gradient of the loss through the
    solve.  The limits are penalties, not constraints."""
    return checked_objective(gradient, (("sway", alpha_sway, sway_limit), ("deflection", alpha_deflection, deflection_limit)))


def _objective_struct(objective: tuple) -> "_cabi.FrameSizingObjective":
    """The penalties of a checked objective (`_objective`) as the launches read them."""
    _, aS, s_lim, aD, d_lim = objective
    return _cabi.FrameSizingObjective(alpha_sway=aS, sway_limit=s_lim, alpha_deflection=aD, deflection_limit=d_lim)


def _sizing_params(cfg: FrameConfig, max_epochs: Optional[int] = None) -> "_cabi.SizingParams":
    """FR:17-44, :155, :170 as the step kernels read them: no scheduler (gamma = 1), `+ 1e-8` in the bending term."""
    return _cabi.SizingParams(E=cfg.E, G=cfg.G, alpha_moment=cfg.alpha_moment, alpha_shear=cfg.alpha_shear, lr=cfg.lr, gamma=1.0,
                              beta1=0.9, beta2=0.999, adam_eps=1e-8, clamp_min=1e-8, bend_eps=1e-8, area_coef=cfg.k,
                              tolerance=cfg.tolerance, patience=cfg.patience,
                              max_epochs=max_epochs if max_epochs is not None else cfg.num_epochs)


class _SizingGradBuffers(NamedTuple):
    rhs: torch.Tensor                    # [B,Nn,3] the adjoint right-hand side
    adj: FrameSolution                   # the adjoint solve: disp = lambda
    grad: torch.Tensor                   # [B,Ne]
    loss_extra: Optional[torch.Tensor]   # [B], None without a displacement term


def _sizing_grad_buffers(topo: FrameTopology, B: int, dev, with_extra: bool) -> _SizingGradBuffers:
    f64 = dict(dtype=torch.float64, device=dev)
    return _SizingGradBuffers(torch.empty((B, topo.Nn, 3), **f64), _empty_solution(topo, B, dev), torch.empty((B, topo.Ne), **f64),
                              torch.zeros((B,), **f64) if with_extra else None)


def _sizing_grad_launches(topo: FrameTopology, I: torch.Tensor, sol: FrameSolution, hp, obj, active: Optional[torch.Tensor],
                          buf: _SizingGradBuffers) -> None:
    """The three launches of dL/dI on the current stream (csrc/frame_sizing_grad.hip around the adjoint solve of §9f); no checks, no
    allocation beyond what `_run_solve` keeps per stream."""
    lib = _cabi.load()
    dev, B = I.device, I.shape[0]
    adj = _adjoint_tables(topo)
    act, extra = _ptr(active), _ptr(buf.loss_extra)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.ops_frame_sizing_rhs_f64(B, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(),
                                          adj.ptr.data_ptr(), adj.idx.data_ptr(), I.data_ptr(), sol.disp.data_ptr(), sol.V.data_ptr(),
                                          sol.M.data_ptr(), ctypes.byref(hp), ctypes.byref(obj), act, buf.rhs.data_ptr(), extra, stream)
    _cabi.check(rc, "ops_frame_sizing_rhs_f64")
    _run_solve(topo, I, buf.rhs, topo.Nn * 3, buf.adj, adj.zero_w, "_ws_adjoint")
    with torch.cuda.device(dev):
        rc = lib.ops_frame_sizing_grad_f64(B, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(),
                                           I.data_ptr(), sol.disp.data_ptr(), sol.V.data_ptr(), sol.M.data_ptr(),
                                           buf.adj.disp.data_ptr(), ctypes.byref(hp), act, sol.status.data_ptr(),
                                           buf.adj.status.data_ptr(), buf.grad.data_ptr(), stream)
    _cabi.check(rc, "ops_frame_sizing_grad_f64")


def frame_sizing_gradient(topo: FrameTopology, I: torch.Tensor, sol: FrameSolution, hp, *, alpha_sway: float = 0.0,
                          sway_limit: Optional[float] = None, alpha_deflection: float = 0.0,
                          deflection_limit: Optional[float] = None, active: Optional[torch.Tensor] = None):
    """dL/dI [B,Ne] of the frame sizing objective (float64, with M, V and the nodal displacements as functions of I)
    from the forward solution `sol` of `frame_solve(topo, I)`: three launches on the current stream -- the adjoint right-hand side,
    the adjoint solve, the gradient (csrc/frame_sizing_grad.hip).  `hp`: a `FrameConfig` or an `ops_sizing_params`.  The objective may
    add `alpha_sway * sum_n (max(0, |ux_n| - sway_limit) / sway_limit)^2` and the same in uy with `alpha_deflection`,
    `deflection_limit`: penalties, not constraints.  Returns (grad, loss_extra, status): loss_extra [B] is the value of the two
    displacement terms (None when both alphas are 0), status [B] the adjoint solve's (non-zero: the frame's row is NaN, as it is for
    a frame with sol.status != 0).  Rows of frames with active[b] == 0 are not written."""
    I = _checked("I", I, torch.float64, (None, topo.Ne), gpu_for="frame_sizing_gradient", in_place=True)
    B, dev = I.shape[0], I.device
    obj = _objective_struct(_objective("total", alpha_sway, sway_limit, alpha_deflection, deflection_limit))
    hp = _sizing_params(hp) if isinstance(hp, FrameConfig) else hp
    for name, t, shape in (("sol.disp", sol.disp, (B, topo.Nn, 3)), ("sol.V", sol.V, (B, topo.Ne)), ("sol.M", sol.M, (B, topo.Ne))):
        _checked(name, t, torch.float64, shape, dev, in_place=True)
    sol = sol._replace(status=_checked("sol.status", sol.status, torch.int32, (B,), dev))
    active = _checked("active", active, torch.uint8, (B,), dev, optional=True)
    buf = _sizing_grad_buffers(topo, B, dev, obj.alpha_sway + obj.alpha_deflection > 0.0)
    if B:
        _sizing_grad_launches(topo, I, sol, hp, obj, active, buf)
    return buf.grad, buf.loss_extra, buf.adj.status


def optimize_frames(topo: FrameTopology, B: int, cfg: Optional[FrameConfig] = None, I0: Optional[torch.Tensor] = None,
                    max_epochs: Optional[int] = None, poll_every: int = 25, loss_history: Optional[list] = None,
                    gradient: str = "explicit", alpha_sway: float = 0.0, sway_limit: Optional[float] = None,
                    alpha_deflection: float = 0.0, deflection_limit: Optional[float] = None, loads: Optional[torch.Tensor] = None,
                    element_loads: Optional[torch.Tensor] = None):
    """FR:163-206 for B frames at once (same topology; `I0` [B,Ne] lets them start from different designs).
    `loads` ([Nn,3] or [B,Nn,3]) and `element_loads` (float64 [Ne,2] or [B,Ne,2]: wy, wx) replace the topology's nodal and element
    loads, per frame when they have a batch dimension; only the forward solve of an epoch changes.
    Adam(lr) with NO scheduler (gamma = 1), loss with `+1e-8` in the bending term (FR:155), early stop
    tolerance 1e-3 / patience 10.  Returns (I float32 [B,Ne], solution of the last solve, epochs_run).
    `loss_history`: a list that receives every epoch's `total_loss` [B] (FR:190; a stopped frame repeats its last value).
    `gradient`: "explicit" steps on the reference's gradient (M and V held fixed: its loop); "total" on the exact gradient of the
    loss through the solve (five launches per epoch, two factorisations) and may add the penalties
    `alpha_sway * sum_n (max(0, |ux_n| - sway_limit) / sway_limit)^2` and, in uy, `alpha_deflection` / `deflection_limit` to the loss."""
    cfg = cfg or FrameConfig()
    obj = _objective_struct(_objective(gradient, alpha_sway, sway_limit, alpha_deflection, deflection_limit))
    if gradient == "total" and topo.Ne > 512:
        raise ValueError(f'gradient="total" serves up to 512 elements per frame (the optimiser step kernel), got {topo.Ne}')
    dev, Ne = topo.device, topo.Ne
    f32 = dict(dtype=torch.float32, device=dev)
    I = (I0.to(**f32).clone() if I0 is not None else torch.full((B, Ne), cfg.I0, **f32))
    st = _StepState(I, I.double(), *arm_optimiser_state(new_optimiser_state(B, Ne, dev)), torch.zeros((B, Ne), **f32), torch.zeros((B, Ne), **f32))
    n_max = max_epochs if max_epochs is not None else cfg.num_epochs
    hp = _sizing_params(cfg, n_max)
    if loads is not None:
        if not torch.is_tensor(loads) or not loads.is_cuda:
            raise RuntimeError("loads must be a GPU tensor: openpystruct_amd has no CPU fallback")
        loads = loads.to(torch.float64).contiguous()
        _check_nodal_loads(topo, loads, B, I.device)
    # every buffer of the loop, before it (the one-launch forward with the explicit step allocates its solution in the first epoch);
    # the forward is one callable that fills and returns its solution
    sol = _empty_solution(topo, B, dev) if element_loads is not None or gradient == "total" else None
    if element_loads is not None:      # the three-launch forward
        w, wbs = _checked_element_loads(topo, element_loads, B, I.device)
        fwd_loads = topo.d_loads if loads is None else loads
        lbs = topo.Nn * 3 if fwd_loads.dim() == 3 else 0
        fwd_rhs = torch.empty((B, topo.Nn, 3), dtype=torch.float64, device=dev)

        def forward(out):
            _element_load_launches(topo, st.I64, fwd_loads, lbs, w, wbs, fwd_rhs, out)
            return out
    else:
        forward = lambda out: frame_solve(topo, st.I64, loads, out=out)  # noqa: E731
    buf = grad = loss_extra = None      # the explicit step forms its gradient from (V, M)
    if gradient == "total":
        buf = _sizing_grad_buffers(topo, B, dev, obj.alpha_sway + obj.alpha_deflection > 0.0)
        grad, loss_extra = buf.grad, buf.loss_extra

    def epoch():
        nonlocal sol
        sol = forward(sol)
        if buf is not None:
            _sizing_grad_launches(topo, st.I64, sol, hp, obj, st.active, buf)
        _sizing_step(st, sol.V, sol.M, hp, grad, loss_extra)

    run_epochs(epoch, n_max, poll_every, st.active, history_callback(loss_history, st.last))
    torch.cuda.synchronize(dev)
    return I, sol, st.epochs


def grid_load_cases(topo: FrameTopology, lateral, vertical):
    """The reference's load pattern (FR:120-131) with per-frame magnitudes: `lateral` [B] and `vertical` [B] (array-likes or
    tensors) -> (loads [B,Nn,3], element_loads [B,Ne,2]) float64 on `topo.device`: (lateral_b, 0, 0) on the nodes of the left column
    line that are not fully fixed, beamUniform(vertical_b, vertical_b) on the horizontal elements.  With a `FrameConfig`'s two
    scalars it is `grid_frame`'s own `nodal_loads`, `wy` and `wx`."""
    f64 = dict(dtype=torch.float64, device=topo.device)
    lateral, vertical = torch.as_tensor(lateral, **f64).reshape(-1), torch.as_tensor(vertical, **f64).reshape(-1)
    if lateral.shape != vertical.shape:
        raise ValueError("lateral and vertical must have one value per frame each")
    left = (topo.coords[:, 0] == topo.coords[:, 0].min()) & ~topo.fix3.all(axis=1)
    horizontal = topo.coords[topo.conn[:, 0], 1] == topo.coords[topo.conn[:, 1], 1]
    loads = torch.zeros((lateral.shape[0], topo.Nn, 3), **f64)
    loads[:, torch.as_tensor(np.nonzero(left)[0], device=topo.device), 0] = lateral[:, None]
    w = torch.zeros((lateral.shape[0], topo.Ne, 2), **f64)
    w[:, torch.as_tensor(np.nonzero(horizontal)[0], device=topo.device), :] = vertical[:, None, None]
    return loads, w


def frame_dataset_draws(n_cases: int, lateral_range=(0.5e4, 2e4), vertical_range=(-2e4, -0.5e4), seed: int = 0):
    """The load magnitudes of `generate_frame_dataset`: (lateral [n_cases], vertical [n_cases]) float64 numpy, uniform over the two
    ranges from `np.random.default_rng(seed)` -- all lateral values first, then all vertical ones."""
    if n_cases < 0:
        raise ValueError("n_cases must be >= 0")
    rng = np.random.default_rng(seed)
    lateral = rng.uniform(lateral_range[0], lateral_range[1], size=n_cases)
    vertical = rng.uniform(vertical_range[0], vertical_range[1], size=n_cases)
    return lateral, vertical


def generate_frame_dataset(num_bays: int, num_stories: int, n_cases: int, cfg: Optional[FrameConfig] = None,
                           lateral_range=(0.5e4, 2e4), vertical_range=(-2e4, -0.5e4), seed: int = 0, gradient: str = "explicit",
                           max_epochs: Optional[int] = None, **objective) -> dict:
    """`n_cases` sized designs of the reference's num_bays x num_stories frame, each under its own wind and gravity load
    (`frame_dataset_draws`, `grid_load_cases`), sized in one batch by `optimize_frames` (`objective`: its penalty keywords).
    Returns CPU tensors: I [n,Ne] float32, lateral, vertical [n] float64, V, M [n,Ne] and disp [n,Nn,3] float64 (the last solve's),
    epochs [n] int32, status [n] int32."""
    cfg = cfg or FrameConfig()
    topo = grid_frame(num_bays, num_stories, cfg)
    lateral, vertical = frame_dataset_draws(n_cases, lateral_range, vertical_range, seed)
    loads, w = grid_load_cases(topo, lateral, vertical)
    I, sol, ep = optimize_frames(topo, n_cases, cfg, max_epochs=max_epochs, gradient=gradient, loads=loads, element_loads=w, **objective)
    return dict(I=I.cpu(), lateral=torch.as_tensor(lateral), vertical=torch.as_tensor(vertical), V=sol.V.cpu(), M=sol.M.cpu(),
                disp=sol.disp.cpu(), epochs=ep.cpu(), status=sol.status.cpu())
