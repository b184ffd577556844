"""Multi-load-case frame sizing: ONE design (one set of element inertias) under C load cases, on the exact gradient, with ONE
factorisation per design and epoch.

`optimize_frames(gradient="total")` sizes every (frame, load) row on its own: two factorisations per row and epoch, and C different
designs for what is one structure under wind from either side, gravity alone and their combinations.  Here the C cases share a
design and the factorisation of §9k (`frame_factor`, `frame_resolve`):

    L(I) = sum_e I_e + sum_c w_c P_c(I)        (aggregate="sum")         P_c: moment + shear (+ sway, deflection) penalty of case c,
    L(I) = sum_e I_e + max_c P_c(I)            (aggregate="max")         M, V, ux, uy functions of I through the solve

Rows are design-major: case c of design g is row g*C + c of every [G,C,...] array; the inertias exist once per design.  An epoch is
six launches -- the keeping solve on I64, the forward re-solve of all G*C rows, the correction of their forces for the element loads,
the adjoint right-hand sides (csrc/frame_designs.hip), the adjoint re-solve, the design step (same file: the gradient of every case
formed in registers, aggregated, Adam, one early stop per design).
"""
from __future__ import annotations

import ctypes
import types
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _cabi
from . import frames
from .frame_frequency import FrequencyFloor
from .frames import FrameCaseSolution, FrameConfig, FrameFactor, FrameTopology
from .sizing_common import _ptr, arm_optimiser_state, checked_aggregate, history_callback, new_optimiser_state, run_epochs, step_schedule


class FrameDesigns(NamedTuple):
    I: torch.Tensor                  # [G, Ne] float32: the designs after their last step
    solution: FrameCaseSolution      # [G, C, ...]: every design's LAST solve (on the inertias that step started from)
    epochs: torch.Tensor             # [G] int32
    governing: torch.Tensor          # [G] int32: the case with the largest (weighted) penalty at the last epoch
    case_penalty: torch.Tensor       # [G, C] float32: P_c at the last epoch


def _penalties(alpha_sway, sway_limit, alpha_deflection, deflection_limit) -> "_cabi.FrameSizingObjective":
    return frames._objective_struct(frames._objective("total", alpha_sway, sway_limit, alpha_deflection, deflection_limit))


def _checked_limits(topo: FrameTopology, C: int) -> None:
    most = _cabi.load().ops_frame_design_max_cases()
    if C < 1 or C > most:
        raise ValueError(f"{C} load cases: the design step serves 1 to {most}")
    if topo.Ne > 512:
        raise ValueError(f"frame design sizing serves up to 512 elements per frame (the design step kernel), got {topo.Ne}")


def _factor_bytes(topo: FrameTopology, G: int) -> int:
    nbytes = int(_cabi.load().ops_frame_factor_workspace_bytes(max(G, 1), topo.n_eq, topo.kd))
    if nbytes == 0:
        raise ValueError(f"frame_factor does not serve this topology: it keeps the factor of the wave-per-frame kernel only, half bandwidth <= 55 "
                         f"(this topology: {topo.kd}) and four waves' LDS within 160 KB (n_eq = {topo.n_eq})")
    return nbytes


def _factor_launch(factor: FrameFactor) -> None:
    """ops_frame_factor_solve_f64 on the current stream into the factor's own buffers (`frame_factor` without its allocations)."""
    topo, I, sol = factor.topo, factor.I, factor.solution
    with torch.cuda.device(I.device):
        rc = _cabi.load().ops_frame_factor_solve_f64(
            I.shape[0], topo.Nn, topo.Ne, topo.n_eq, topo.kd, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(),
            topo.d_w.data_ptr(), topo.d_elem_eq.data_ptr(), topo.d_node_eq.data_ptr(), I.data_ptr(), topo.d_loads.data_ptr(), 0,
            sol.disp.data_ptr(), sol.forces.data_ptr(), sol.V.data_ptr(), sol.M.data_ptr(), sol.status.data_ptr(),
            factor.workspace.data_ptr(), factor.workspace.numel(), torch.cuda.current_stream(I.device).cuda_stream)
    _cabi.check(rc, "ops_frame_factor_solve_f64")


class _DesignState:
    """What the design step updates in place [G, ...] and what steps 4 to 6 of an epoch pass between them [G, C, ...]."""

    def __init__(self, topo: FrameTopology, I: torch.Tensor, I64: torch.Tensor, C: int, hp, obj, aggregate: int, weights, with_grad: bool,
                 n_vars: Optional[int] = None):
        G, Ne = I.shape
        Nv = Ne if n_vars is None else n_vars         # the variables Adam steps on: the elements, or their groups (frame_groups.py)
        dev = I.device
        f64, f32, i32 = (dict(dtype=t, device=dev) for t in (torch.float64, torch.float32, torch.int32))
        self.topo, self.C, self.hp, self.obj, self.aggregate = topo, C, hp, obj, aggregate
        self.I, self.I64 = I, I64
        (self.exp_avg, self.exp_avg_sq, self.best, self.patience_cnt, self.epochs, self.active,
         self.last) = arm_optimiser_state(new_optimiser_state(G, Nv, dev))
        self.case_penalty, self.governing = torch.zeros((G, C), **f32), torch.zeros((G,), **i32)
        self.weights = None if weights is None else torch.as_tensor(weights, **f64)
        self.rhs = torch.empty((G, C, topo.Nn, 3), **f64)
        self.lam = frames._empty_case_solution(topo, G, C, dev)           # disp = lambda; the adjoint's forces, V, M are not used
        self.loss_extra = torch.zeros((G, C), **f64) if obj.alpha_sway + obj.alpha_deflection > 0.0 else None
        self.grad = torch.empty((G, Nv), **f64) if with_grad else None
        self.schedule = step_schedule(hp, dev)
        self.extras = None                        # (grad_extra [G,Ne], penalty_extra [G]) of a term formed outside the step: the dyn entry

    def adjoint_rhs(self, fwd: FrameCaseSolution) -> None:
        """Step 4 of an epoch on the current stream: the adjoint right-hand sides (and the hinge values) of all G*C rows."""
        topo, C, I = self.topo, self.C, self.I
        dev = I.device
        adj = frames._adjoint_tables(topo)
        with torch.cuda.device(dev):
            rc = _cabi.load().ops_frame_design_rhs_f64(
                I.shape[0], C, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(), adj.ptr.data_ptr(),
                adj.idx.data_ptr(), self.I64.data_ptr(), fwd.disp.data_ptr(), fwd.V.data_ptr(), fwd.M.data_ptr(), ctypes.byref(self.hp),
                ctypes.byref(self.obj), self.active.data_ptr(), self.rhs.data_ptr(), _ptr(self.loss_extra),
                torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(rc, "ops_frame_design_rhs_f64")

    def gradient_and_step(self, factor: FrameFactor, fwd: FrameCaseSolution) -> None:
        """Steps 4 to 6 of an epoch on the current stream: the adjoint right-hand sides of all G*C rows, their re-solve on the kept
        factor, the design step.  No checks, no allocation."""
        self.adjoint_rhs(fwd)
        frames._resolve_launch(factor, self.C, self.rhs, self.C * self.topo.Nn * 3, self.lam)
        self.step(fwd, self.lam.disp, self.lam.status)

    def _step_entry(self, name: str):
        """(the step entry `ops_frame_<name>_step[_dyn]_f32`, its name): the dyn one when a term's `extras` are set."""
        name = f"ops_frame_{name}_step_dyn_f32" if self.extras is not None else f"ops_frame_{name}_step_f32"
        return getattr(_cabi.load(), name), name

    def _step_tail(self, fwd: FrameCaseSolution, lam: torch.Tensor, status_adj: Optional[torch.Tensor]) -> tuple:
        """The arguments of a step entry from `disp` on: the same in ops_frame_design_step_f32 and ops_frame_group_step_f32, and in
        their dyn forms with the two extras before the stream."""
        tail = self._plain_tail(fwd, lam, status_adj)
        return tail if self.extras is None else tail[:-1] + tuple(t.data_ptr() for t in self.extras) + tail[-1:]

    def _plain_tail(self, fwd: FrameCaseSolution, lam: torch.Tensor, status_adj: Optional[torch.Tensor]) -> tuple:
        return (fwd.disp.data_ptr(), fwd.V.data_ptr(), fwd.M.data_ptr(), lam.data_ptr(), _ptr(self.loss_extra), fwd.status.data_ptr(),
                _ptr(status_adj), _ptr(self.weights), self.aggregate,
                *(t.data_ptr() for t in (self.exp_avg, self.exp_avg_sq, self.best, self.patience_cnt, self.epochs, self.active, self.last,
                                         self.case_penalty, self.governing)),
                _ptr(self.grad), ctypes.byref(self.hp), self.schedule.data_ptr(), torch.cuda.current_stream(self.I.device).cuda_stream)

    def step(self, fwd: FrameCaseSolution, lam: torch.Tensor, status_adj: Optional[torch.Tensor]) -> None:
        """The design step on the current stream (`lam` [G,C,Nn,3]: the adjoint displacements)."""
        topo, I = self.topo, self.I
        entry, name = self._step_entry("design")
        with torch.cuda.device(I.device):
            rc = entry(I.shape[0], self.C, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), frames._adjoint_tables(topo).conn.data_ptr(),
                       I.data_ptr(), self.I64.data_ptr(), *self._step_tail(fwd, lam, status_adj))
        _cabi.check(rc, name)


def _checked_problem(topo: FrameTopology, loads, element_loads, n_designs, V0, v_name: str, n_vars: int, aggregate: str, weights,
                     who: str, frequency=None) -> types.SimpleNamespace:
    """The arguments of a designs run, checked in the order every entry keeps: every shape before any device, then where everything
    lives (with the loads, on the topology's device); a `frequency` term is checked against the problem with the shapes.  `V0`: the optional start [G, n_vars] (I0, or X0 of the grouped loop).
    -> G, C, dev, loads, w (the checked tensors), agg, w_c (`checked_aggregate`), nbytes (`_factor_bytes`)."""
    if torch.is_tensor(loads) and loads.dim() == 4:
        G = int(loads.shape[0])
    elif V0 is not None and torch.is_tensor(V0) and V0.dim() == 2:
        G = int(V0.shape[0])
    elif n_designs is not None:
        G = int(n_designs)
    else:
        raise ValueError(f"loads shared by the designs ([C, Nn, 3]) need n_designs or {v_name} to say how many designs there are")
    if n_designs is not None and int(n_designs) != G:
        raise ValueError(f"n_designs = {n_designs}, but loads / {v_name} are for {G} designs")
    dev = topo.device
    frames._checked_cases("loads", loads, G, (topo.Nn, 3), dev, who, shape_only=True)
    C = int(loads.shape[-3])
    if element_loads is not None:
        frames._checked_cases("element_loads", element_loads, G, (topo.Ne, 2), dev, who, shape_only=True)
        if element_loads.shape[-3] != C:
            raise ValueError(f"element_loads has {element_loads.shape[-3]} cases, loads has {C}")
    if V0 is not None and (not torch.is_tensor(V0) or tuple(V0.shape) != (G, n_vars)):
        raise ValueError(f"{v_name} must be [{G}, {n_vars}]")
    _checked_limits(topo, C)
    agg, w_c = checked_aggregate(aggregate, weights, C)
    nbytes = _factor_bytes(topo, G)
    _checked_frequency(frequency, topo, G)
    if loads.is_cuda and topo.device.type == "cuda" and topo.device.index in (None, loads.device.index):
        dev = loads.device
    loads = frames._checked_cases("loads", loads, G, (topo.Nn, 3), dev, who)
    w = None if element_loads is None else frames._checked_cases("element_loads", element_loads, G, (topo.Ne, 2), dev, who)
    if V0 is not None and not V0.is_cuda:
        raise RuntimeError(f"{who} needs GPU tensors: openpystruct_amd has no CPU fallback")
    return types.SimpleNamespace(G=G, C=C, dev=dev, loads=loads, w=w, agg=agg, w_c=w_c, nbytes=nbytes)


class _Forward:
    """Steps 1 to 3 of an epoch -- the keeping solve on I64, the forward re-solve of all G*C rows, the correction of their forces for
    the element loads -- with every buffer allocated here, once: `factor`, `fwd`, and the cases' right-hand sides with the consistent
    element loads, which do not depend on I (frame_resolve's rows, formed once).  Calling it launches the three on the current stream."""

    def __init__(self, topo: FrameTopology, I64: torch.Tensor, q: types.SimpleNamespace):
        lib = _cabi.load()
        G, C, dev, loads, w = q.G, q.C, q.dev, q.loads, q.w
        Nn, Ne = topo.Nn, topo.Ne
        self.topo, self.G, self.C, self.dev = topo, G, C, dev
        self.factor = FrameFactor(topo, I64, torch.empty(q.nbytes, dtype=torch.uint8, device=dev), frames._empty_solution(topo, G, dev))
        self.fwd = frames._empty_case_solution(topo, G, C, dev)
        if G == 0:
            return
        adj = frames._adjoint_tables(topo)
        shared = loads.dim() == 3 and (w is None or w.dim() == 3)
        if loads.dim() == 3 and not shared:
            loads = loads.expand(G, C, Nn, 3).contiguous()
        self.w_rows, self.wbs = (topo.d_w, 0) if w is None else (w, 2 * Ne)
        if w is not None and w.dim() == 3:            # the correction of the forces runs on all G * C rows
            self.w_rows = w.expand(G, C, Ne, 2).contiguous()
        rows = C if shared else G * C
        self.fwd_rhs = torch.empty((rows, Nn, 3), dtype=torch.float64, device=dev)
        w_rhs = w if (shared and w is not None) else self.w_rows
        with torch.cuda.device(dev):
            rc = lib.ops_frame_load_rhs_f64(rows, Nn, Ne, topo.d_geo.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(), loads.data_ptr(),
                                            3 * Nn, w_rhs.data_ptr(), self.wbs, self.fwd_rhs.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(rc, "ops_frame_load_rhs_f64")
        self.rbs = 0 if shared else C * Nn * 3
        self.has_w = w is not None or bool(np.any(topo.wy != 0.0) or np.any(topo.wx != 0.0))

    def __call__(self) -> None:
        topo, fwd, dev = self.topo, self.fwd, self.dev
        _factor_launch(self.factor)               # its own solution (the topology's loads) is not used
        frames._resolve_launch(self.factor, self.C, self.fwd_rhs, self.rbs, fwd)
        if self.has_w:
            with torch.cuda.device(dev):
                rc = _cabi.load().ops_frame_load_forces_f64(self.G * self.C, topo.Ne, topo.d_geo.data_ptr(), self.w_rows.data_ptr(), self.wbs,
                                                            fwd.status.data_ptr(), fwd.forces.data_ptr(), fwd.V.data_ptr(), fwd.M.data_ptr(),
                                                            torch.cuda.current_stream(dev).cuda_stream)
            _cabi.check(rc, "ops_frame_load_forces_f64")


def _start_values(V0: Optional[torch.Tensor], G: int, n_vars: int, cfg: FrameConfig, dev) -> torch.Tensor:
    """The variables a designs loop starts from, float32 [G, n_vars] on `dev`: a copy of `V0`, or cfg.I0 everywhere."""
    return V0.to(dtype=torch.float32, device=dev).clone() if V0 is not None else torch.full((G, n_vars), cfg.I0, dtype=torch.float32, device=dev)


def _checked_frequency(frequency: Optional[FrequencyFloor], topo: FrameTopology, G: int) -> Optional[FrequencyFloor]:
    """The `frequency=` of an entry, checked against its problem before any device call."""
    if frequency is not None:
        if not isinstance(frequency, FrequencyFloor):
            raise ValueError("frequency must be a FrequencyFloor or None")
        frequency.check(topo, G)
    return frequency


def _run_design_loop(st: _DesignState, q: types.SimpleNamespace, n_max: int, poll_every: int, loss_history: Optional[list],
                     frequency: Optional[FrequencyFloor] = None) -> _Forward:
    """The loop of a designs run on the state `st` (its `step` is the design's or the groups'): up to `n_max` epochs of the forward
    and `st.gradient_and_step`, then the forward once more -- I64 froze when a design stopped: every design's last solve, all C cases
    -- and a device synchronise.  Returns the forward, whose `fwd` is that solve; with no designs nothing is launched.
    With `frequency` the step is the dyn one, and between the forward and the step the term's iteration advances on the epoch's
    factor (`start_iters` in the first epoch, `iters` after it, continuing from the last Ritz step's R) and the floor kernel runs on
    the active designs; after the last forward it advances once more and the floor kernel fills `.modes` / `.penalty` for all.  The
    term's buffers are allocated before the loop."""
    fw = _Forward(st.topo, st.I64, q)
    if q.G:
        if frequency is not None:
            frequency.bind(q.G, q.dev)
            frequency.start()
            st.extras = frequency.extras

        def epoch():
            fw()
            if frequency is not None:
                frequency.advance(fw.factor)
                frequency.floor_launch(st.active)
            st.gradient_and_step(fw.factor, fw.fwd)

        run_epochs(epoch, n_max, poll_every, st.active, history_callback(loss_history, st.last))
        fw()
        if frequency is not None:
            frequency.advance(fw.factor)
            frequency.floor_launch(None)
        torch.cuda.synchronize(q.dev)
        if frequency is not None:
            frequency.finish()
    return fw


def optimize_frame_designs(topo: FrameTopology, loads: torch.Tensor, element_loads: Optional[torch.Tensor] = None, *,
                           n_designs: Optional[int] = None, cfg: Optional[FrameConfig] = None, I0: Optional[torch.Tensor] = None,
                           aggregate: str = "sum", weights: Optional[Sequence[float]] = None, alpha_sway: float = 0.0,
                           sway_limit: Optional[float] = None, alpha_deflection: float = 0.0, deflection_limit: Optional[float] = None,
                           max_epochs: Optional[int] = None, poll_every: int = 25, loss_history: Optional[list] = None,
                           frequency: Optional[FrequencyFloor] = None) -> FrameDesigns:
    """Size G frame designs, each under its C load cases, on the exact gradient of the aggregated loss.
    `loads`: float64 [G,C,Nn,3], or [C,Nn,3] shared by the designs (then `n_designs` or `I0` [G,Ne] says how many there are);
    `element_loads`: float64 [G,C,Ne,2] or [C,Ne,2] (wy, wx), None = the topology's `wy` / `wx` in every case, as in `frame_resolve`.
    `aggregate`: "sum" (`weights` w_c, default all 1) or "max" (the worst case governs; no weights).  The penalties are those of
    `optimize_frames(gradient="total")`, per load case.  Adam without a scheduler, the clamp and the early stop of `optimize_frames`,
    once per design on its aggregated loss.  Six launches and ONE factorisation per epoch (the rows path: five launches and two
    factorisations per ROW); every buffer is allocated before the loop; `poll_every` as in `optimize_frames`.  `loss_history`: a
    list that receives every epoch's design loss [G].  Served: half bandwidth <= 55 (`frame_factor`), C <= 64, Ne <= 512.
    `frequency`: a `FrequencyFloor` adds its penalty on the lowest natural frequencies (frame_frequency.py) -- a
    penalty, not a constraint; with None every launch is the one made without the keyword.
    Returns `FrameDesigns` (I, the last solve of every design and case, epochs, governing case, case penalties)."""
    cfg = cfg or FrameConfig()
    obj = _penalties(alpha_sway, sway_limit, alpha_deflection, deflection_limit)
    q = _checked_problem(topo, loads, element_loads, n_designs, I0, "I0", topo.Ne, aggregate, weights, "optimize_frame_designs", frequency)
    n_max = max_epochs if max_epochs is not None else cfg.num_epochs
    I = _start_values(I0, q.G, topo.Ne, cfg, q.dev)
    st = _DesignState(topo, I, I.double(), q.C, frames._sizing_params(cfg, n_max), obj, q.agg, q.w_c, with_grad=False)
    fw = _run_design_loop(st, q, n_max, poll_every, loss_history, frequency)
    return FrameDesigns(I, fw.fwd, st.epochs, st.governing, st.case_penalty)


def _checked_gradient_inputs(factor: FrameFactor, sol: FrameCaseSolution, hp, aggregate: str, weights, who: str, frequency=None,
                             modes=None) -> types.SimpleNamespace:
    """The arguments of a gradient entry `who`, checked in the order both keep: the factor's inertias, the solution's shapes, the
    limits, the aggregate, then where everything lives.  -> topo, I64 (factor.I), G, C, agg, w_c (`checked_aggregate`), hp (an
    `ops_sizing_params`)."""
    topo, I64 = factor.topo, factor.I
    if not torch.is_tensor(I64) or I64.dtype != torch.float64 or I64.dim() != 2 or I64.shape[1] != topo.Ne:
        raise ValueError(f"factor.I must be float64 [G, {topo.Ne}]")
    G = I64.shape[0]
    for name, t, tail, dt in (("sol.disp", sol.disp, (topo.Nn, 3), torch.float64), ("sol.V", sol.V, (topo.Ne,), torch.float64),
                              ("sol.M", sol.M, (topo.Ne,), torch.float64), ("sol.status", sol.status, (), torch.int32)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 2 + len(tail) or t.shape[0] != G or tuple(t.shape[2:]) != tail or \
                t.shape[1] != sol.disp.shape[1] or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous {str(dt).split('.')[-1]} [{G}, C{''.join(', ' + str(n) for n in tail)}]")
    C = int(sol.disp.shape[1])
    _checked_limits(topo, C)
    agg, w_c = checked_aggregate(aggregate, weights, C)
    _checked_frequency(frequency, topo, G)
    if modes is not None and frequency is None:
        raise ValueError("modes= is for a frequency= term")
    if not I64.is_cuda or any(not t.is_cuda for t in (sol.disp, sol.V, sol.M, sol.status)):
        raise RuntimeError(f"{who} needs GPU tensors: openpystruct_amd has no CPU fallback")
    hp = frames._sizing_params(hp) if isinstance(hp, FrameConfig) else hp
    return types.SimpleNamespace(topo=topo, I64=I64, G=G, C=C, agg=agg, w_c=w_c, hp=hp)


def frame_design_gradient(factor: FrameFactor, sol: FrameCaseSolution, hp, *, aggregate: str = "sum",
                          weights: Optional[Sequence[float]] = None, alpha_sway: float = 0.0, sway_limit: Optional[float] = None,
                          alpha_deflection: float = 0.0, deflection_limit: Optional[float] = None,
                          frequency: Optional[FrequencyFloor] = None, modes=None):
    """dL/dI [G,Ne] (float64) of the aggregated design objective from a caller's `frame_factor(topo, I)` and the solution `sol` of
    `frame_resolve(factor, ...)`: steps 4 to 6 of an epoch of `optimize_frame_designs` -- the adjoint right-hand sides, ONE re-solve
    on the kept factor, the design step -- with the step's state in scratch tensors: nothing of the caller's is written.  `hp`: a
    `FrameConfig` or an `ops_sizing_params`.  Returns (grad, loss_extra [G,C] -- the value of the displacement terms per case, None
    when both alphas are 0 --, governing [G] int32).  "sum": grad = 1 + sum_c w_c dP_c/dI; "max": 1 + dP_c*/dI of the governing
    case.  Rows of a design with a failed factorisation (or, under "sum", any failed case) are NaN.  `frequency`: a `FrequencyFloor`
    adds dP_f/dI from a cold iteration of its `start_iters` on `factor`, or, with `modes` (a `FrameModes` of the caller for these
    inertias, at least the term's n_modes), from those and no iteration; a design whose mode status is non-zero gets a NaN row."""
    obj = _penalties(alpha_sway, sway_limit, alpha_deflection, deflection_limit)
    q = _checked_gradient_inputs(factor, sol, hp, aggregate, weights, "frame_design_gradient", frequency, modes)
    st = _DesignState(q.topo, q.I64.float(), q.I64.clone(), q.C, q.hp, obj, q.agg, q.w_c, with_grad=True)
    if q.G:
        _frequency_extras(st, frequency, factor, modes)
        st.gradient_and_step(factor, sol)
        if frequency is not None and modes is None:
            frequency.finish()
    return st.grad, st.loss_extra, st.governing


def _frequency_extras(st: _DesignState, frequency: Optional[FrequencyFloor], factor: FrameFactor, modes=None) -> None:
    """The term of a one-shot entry on the current stream, into the state's `extras`: a cold iteration on `factor`, or the caller's modes."""
    if frequency is None:
        return
    G, dev = st.I.shape[0], st.I.device
    if modes is not None:
        frequency.from_modes(modes, G, dev)
    else:
        frequency.bind(G, dev)
        frequency.cold(factor)
    st.extras = frequency.extras


def _dataset_fields(r, lateral: np.ndarray, vertical: np.ndarray, G: int, C: int) -> dict:
    """The CPU tensors both dataset generators return, from a designs result `r` and the draws of its G * C load cases."""
    sol = r.solution
    return dict(I=r.I.cpu(), lateral=torch.as_tensor(lateral).reshape(G, C), vertical=torch.as_tensor(vertical).reshape(G, C),
                V=sol.V.cpu(), M=sol.M.cpu(), disp=sol.disp.cpu(), epochs=r.epochs.cpu(), status=sol.status.cpu(),
                governing=r.governing.cpu(), case_penalty=r.case_penalty.cpu())


def generate_frame_design_dataset(num_bays: int, num_stories: int, n_designs: int, n_load_cases: int, cfg: Optional[FrameConfig] = None,
                                  lateral_range=(0.5e4, 2e4), vertical_range=(-2e4, -0.5e4), seed: int = 0, aggregate: str = "sum",
                                  weights: Optional[Sequence[float]] = None, max_epochs: Optional[int] = None, **objective) -> dict:
    """`generate_frame_dataset` for designs under several load cases: `n_designs` designs of the reference's num_bays x num_stories
    frame, each under `n_load_cases` wind and gravity loads -- `frame_dataset_draws(n_designs * n_load_cases)` through
    `grid_load_cases`, design-major -- sized in one batch by `optimize_frame_designs` (`objective`: its penalty keywords).  Returns
    CPU tensors: I [G,Ne] float32, lateral, vertical [G,C] float64, V, M [G,C,Ne] and disp [G,C,Nn,3] float64 (the last solve's),
    epochs [G] int32, status [G,C] int32, governing [G] int32, case_penalty [G,C] float32."""
    cfg = cfg or FrameConfig()
    G, C = int(n_designs), int(n_load_cases)
    topo = frames.grid_frame(num_bays, num_stories, cfg)
    lateral, vertical = frames.frame_dataset_draws(G * C, lateral_range, vertical_range, seed)
    loads, w = frames.grid_load_cases(topo, lateral, vertical)
    r = optimize_frame_designs(topo, loads.reshape(G, C, topo.Nn, 3), w.reshape(G, C, topo.Ne, 2), n_designs=G, cfg=cfg, aggregate=aggregate,
                               weights=weights, max_epochs=max_epochs, **objective)
    return _dataset_fields(r, lateral, vertical, G, C)
