"""Multi-load-case beam sizing: ONE design (one set of element inertias) under C load cases.

The reference sizes every load case on its own; its MultiCase surrogates then group `n_cases` consecutive samples and take
mean + 0.5 std of their separately optimal inertias as the label (`dataprep.unify_label_with_c`, PINN:79-92).  Here the C cases
of a group share one design, optimised under all of them together:

    L(I) = sum_e I_e + sum_c w_c P_c(I)        (aggregate="sum")         P_c: moment + shear (+ deflection) penalty of load case c,
    L(I) = sum_e I_e + max_c P_c(I)            (aggregate="max")         M, V, v functions of I through the solve

Rows are design-major: load case c of design g is beam row g*C + c.  The epoch is three launches on the G*C rows -- the float64
`beam_solve`, dL/dI of every row through it (`sizing._beam_sizing_grad_launch`, both exactly as the single-case "total" mode uses
them) and the design step (csrc/sizing_multicase.hip), which ties the C rows of a design together: one Adam state, the penalties
aggregated, one early stop, the new inertias written back into all C rows.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _cabi
from .beam import BeamSolution, beam_solve
from .sizing import (RECORD_KEYS, Cases, SizingConfig, _beam_sizing_grad_launch, _case_record_fields, _shared_rows, make_cases,  # noqa: F401
                     sizing_tiling)
from .sizing_common import (AGGREGATES, _ptr, arm_optimiser_state, checked_aggregate, checked_objective, new_optimiser_state,  # noqa: F401  (AGGREGATES: public here)
                            run_sizing_loop, step_schedule)


def check_design_groups(cases: Cases, n_load_cases: int) -> int:
    """The number of designs G of a design-major batch: len(cases) == G * n_load_cases, and the rows of a group share
    `node_positions` and `fix` (one design has one geometry and one set of supports).  ValueError names the first offending design."""
    C = int(n_load_cases)
    if C < 1:
        raise ValueError(f"n_load_cases must be >= 1, got {n_load_cases}")
    B = len(cases)
    if B % C:
        raise ValueError(f"{B} cases are not a whole number of designs of {C} load cases: design {B // C} is incomplete")
    G = B // C
    if G == 0:
        return 0
    N = cases.node_positions.shape[1]
    xs, fx = cases.node_positions.reshape(G, C, N), cases.fix.reshape(G, C, N)
    bad = ((xs != xs[:, :1]).any(dim=2) | (fx != fx[:, :1]).any(dim=2)).any(dim=1)
    if bool(bad.any()):
        g = int(torch.nonzero(bad)[0])
        what = "node_positions" if bool((xs[g] != xs[g, :1]).any()) else "fix"
        raise ValueError(f"design {g}: its {C} load cases do not share {what}")
    return G


def make_design_cases(n_designs: int, n_load_cases: int, cfg: SizingConfig, seed: int = 20250307, device="cpu") -> Cases:
    """`make_cases(n_designs * n_load_cases, ...)` as design-major groups.  The fixed bridge: as drawn (every case already shares
    geometry and supports).  random_bridge == 1: every group takes `node_positions`, `L`, `roller_nodes_t`, `n_rollers` and `fix` of
    its first row; a drawn force that lands on a support of the design stays in the record and loads nothing (OpenSees ignores a
    load on a constrained degree of freedom; the solve does the same)."""
    G, C = int(n_designs), int(n_load_cases)
    cases = make_cases(G * C, cfg, seed, device=device)
    if cfg.random_bridge == 1 and G > 0:
        first = lambda t: t.reshape(G, C, *t.shape[1:])[:, :1].expand(G, C, *t.shape[1:]).reshape(t.shape).contiguous()   # noqa: E731
        xs = first(cases.node_positions)
        # the force positions of the records follow the design's geometry (generate_multicase_dataset gathers them from xs)
        cases = Cases(xs, first(cases.L), first(cases.roller_nodes_t), first(cases.n_rollers), cases.force_nodes_t, cases.n_forces,
                      cases.force_values_t, first(cases.fix), cases.Fy)
    check_design_groups(cases, C)
    return cases


class MultiCaseState:
    """Device-resident state of G designs under C load cases each: the design's optimiser state [G, ...] and the beam rows [G*C, ...]
    the solve and the gradient launches work on.  The tiling of every solve is fixed when the state is built."""

    def __init__(self, cases: Cases, cfg: SizingConfig, device: torch.device, n_load_cases: int, aggregate: str = "sum",
                 weights: Optional[Sequence[float]] = None, alpha_deflection: float = 0.0, deflection_limit: Optional[float] = None):
        self.aggregate, _ = checked_aggregate(aggregate, weights)          # its name; the weights' values after the device and the shapes
        self.objective = checked_objective("total", (("deflection", alpha_deflection, deflection_limit),))
        device = torch.device(device)
        if device.type != "cuda" or cases.Fy.device.type != "cuda":
            raise RuntimeError("optimize_designs needs GPU tensors: openpystruct_amd has no CPU fallback")
        C = int(n_load_cases)
        G = check_design_groups(cases, C)
        if C > _cabi.load().ops_beam_sizing_multicase_max_cases():
            raise ValueError(f"n_load_cases = {C} exceeds the {_cabi.load().ops_beam_sizing_multicase_max_cases()} the step kernel serves")
        B, N = cases.Fy.shape
        Ne = N - 1
        if Ne > 512:
            raise ValueError(f"multi-case sizing serves up to 512 elements per beam (the optimiser step kernel), got {Ne}")
        _, w = checked_aggregate(aggregate, weights, C)
        f64 = dict(dtype=torch.float64, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.G, self.C, self.B, self.N, self.Ne, self.device, self.cfg = G, C, B, N, Ne, device, cfg
        self.weights = None if w is None else torch.as_tensor(w, **f64)
        shared_geom, shared_fix = _shared_rows(cases) if B else (True, True)
        self._solve_tiling = sizing_tiling(N, shared_geometry=False)      # the "total" mode's: beam_solve.hip's 16 lanes while they fit
        self.x = (cases.node_positions[0] if shared_geom else cases.node_positions).to(device).contiguous()
        self.fix = (cases.fix[0] if shared_fix else cases.fix).to(device).contiguous()
        self.Fy = cases.Fy.to(device).contiguous()
        self.E, self.wy = torch.full((), cfg.E, **f64), torch.full((), cfg.uniform_udl, **f64)
        # the design [G, ...]
        self.I = torch.full((G, Ne), cfg.I_0, **f32)
        (self.exp_avg, self.exp_avg_sq, self.best_loss, self.patience_cnt, self.epochs_run, self.active,
         self.last_loss) = arm_optimiser_state(new_optimiser_state(G, Ne, device))
        self.case_penalty = torch.zeros((G, C), **f32)
        self.governing = torch.zeros((G,), **i32)
        # its beam rows [G*C, ...]
        self.I64_rows = torch.full((B, Ne), float(np.float32(cfg.I_0)), **f64)
        self.active_rows = torch.ones((B,), dtype=torch.uint8, device=device)
        self._grad = torch.empty((B, Ne), **f64)
        self._loss_extra = torch.zeros((B,), **f64) if self.objective[1] > 0.0 else None
        self._obj = _cabi.SizingObjective(alpha_deflection=self.objective[1], deflection_limit=self.objective[2])
        self._grad_status = torch.zeros((B,), **i32)
        self._hp = cfg.c_params()
        self._schedule = step_schedule(self._hp, device)
        self.sol: Optional[BeamSolution] = None
        self.V32 = self.M32 = None

    def _step(self) -> None:
        """The design step, one launch on the current stream; no checks, no allocation."""
        with torch.cuda.device(self.device):
            rc = _cabi.load().ops_beam_sizing_step_multicase_f32(
                self.G, self.C, self.Ne, self.I.data_ptr(), self.I64_rows.data_ptr(), self.sol.V.data_ptr(), self.sol.M.data_ptr(),
                self._grad.data_ptr(), _ptr(self._loss_extra), _ptr(self.weights), self.aggregate,
                *(t.data_ptr() for t in (self.exp_avg, self.exp_avg_sq, self.best_loss, self.patience_cnt, self.epochs_run, self.active,
                                         self.active_rows, self.last_loss, self.case_penalty, self.governing)),
                ctypes.byref(self._hp), self._schedule.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        _cabi.check(rc, "ops_beam_sizing_step_multicase_f32")

    def epoch(self) -> None:
        """Three launches: the float64 solve of the G*C rows on I64_rows, dL/dI of every row through it, the design step."""
        self.sol = beam_solve(self.x, self.E, self.I64_rows, self.fix, self.Fy, self.wy, tiling=self._solve_tiling, out=self.sol)
        _beam_sizing_grad_launch(self.x, self.E, self.I64_rows, self.fix, self.wy, self.sol, self._hp, self._obj, self.active_rows,
                                 self._grad, self._loss_extra, self._grad_status)
        self._step()

    def finalize(self) -> None:
        """The state of every design's LAST solve: `I64_rows` froze when the design stopped, so one full solve with the epochs'
        tiling reproduces it for all C load cases; the float32 roundings of shear / moment are taken from it."""
        self.sol = beam_solve(self.x, self.E, self.I64_rows, self.fix, self.Fy, self.wy, tiling=self._solve_tiling, out=self.sol)
        self.V32, self.M32 = self.sol.V.float(), self.sol.M.float()


def optimize_designs(cases: Cases, cfg: SizingConfig, device, n_load_cases: int, aggregate: str = "sum",
                     weights: Optional[Sequence[float]] = None, alpha_deflection: float = 0.0,
                     deflection_limit: Optional[float] = None, poll_every: int = 25, use_graph: bool = True,
                     record_loss: bool = False) -> MultiCaseState:
    """Size G = len(cases) / n_load_cases designs, each under its `n_load_cases` consecutive cases (design-major), to the early stop
    (or max_e) of the design's aggregated loss; the gradient is the exact one through the solve.  `aggregate`: "sum" (weights w_c,
    default all 1) or "max" (the worst case governs; no weights).  `alpha_deflection`, `deflection_limit`: the serviceability term
    of `optimize_cases(gradient="total")`, per load case.  `poll_every` epochs are replayed as one captured graph; `record_loss`
    keeps every epoch's design loss in `state.loss_history` [epochs, G] and runs the loop launch by launch.  Returns the final
    device state; no state or graph is kept between calls."""
    device = torch.device(device)
    st = MultiCaseState(cases, cfg, device, n_load_cases, aggregate, weights, alpha_deflection, deflection_limit)
    if st.G == 0:
        return st
    _, history = run_sizing_loop(st.epoch, cfg.max_e, poll_every, st.active, st.last_loss, device,
                                 use_graph=use_graph and poll_every > 1 and not record_loss, record=record_loss)
    if record_loss:
        st.loss_history = history
    st.finalize()
    torch.cuda.synchronize(device)
    return st


def generate_multicase_dataset(n_designs: int, n_load_cases: int, cfg: Optional[SizingConfig] = None, device="cuda",
                               seed: int = 20250307, aggregate: str = "sum", weights: Optional[Sequence[float]] = None,
                               alpha_deflection: float = 0.0, deflection_limit: Optional[float] = None,
                               poll_every: int = 25) -> Dict[str, object]:
    """`generate_dataset` for designs under several load cases: the 13 record fields with G*C rows in design-major order, `I_values`
    identical in the C rows of a design -- `dataprep.prepare(records, n_cases=C)` then labels every group with exactly its optimised
    design (mean = I, std = 0) in place of the `unify_label_with_c` heuristic.  Also `design_ids` [G*C], `governing_case` [G],
    `case_penalty` [G, C], `epochs_run` [G], `status` [G*C] and `I_solved` [G*C, Ne]."""
    cfg = cfg or SizingConfig()
    G, C = int(n_designs), int(n_load_cases)
    cases = make_design_cases(G, C, cfg, seed, device=device)
    st = optimize_designs(cases, cfg, device, C, aggregate=aggregate, weights=weights, alpha_deflection=alpha_deflection,
                          deflection_limit=deflection_limit, poll_every=poll_every)
    return {
        **_case_record_fields(cases, cfg, st.sol),
        "I_values": st.I.repeat_interleave(C, dim=0),      # one design, C rows
        "shear_forces": st.V32,
        "bending_moments": st.M32,
        "epochs_run": st.epochs_run,
        "status": st.sol.status,
        "I_solved": st.I64_rows,
        "design_ids": torch.from_numpy(np.repeat(np.arange(G, dtype=np.int64), C)),
        "governing_case": st.governing,
        "case_penalty": st.case_penalty,
    }
