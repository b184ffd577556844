"""Frame design sizing with LINKED member groups and a section catalogue.

`optimize_frame_designs` gives every element an inertia of its own.  Here several elements share one section -- all columns of a
story, all beams of a floor, or any grouping the caller gives -- and the loop owns Ng <= Ne variables X [G,Ng]; the element
inertias are their expansion I[e] = X[group[e]]:

    L(X) = sum_e X_group(e) + sum_c w_c P_c(I(X))      ("sum";  "max": the worst case)      dL/dX_j = sum over the elements e of group j
                                                                                            of dL/dI_e  (a float64 sum in a fixed order)

An epoch is the six launches of `optimize_frame_designs` with the group step (csrc/frame_groups.hip) in place of the design step.
After the loop a catalogue of available inertias may be applied: every variable is snapped to an entry (`snap_to_catalogue`) and
both the continuous and the discrete design are evaluated by one forward pass each (`evaluate_frame_designs`).  That is all the
discrete part does: no search beyond snapping.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _cabi
from . import frames
from .frame_designs import (_checked_gradient_inputs, _checked_problem, _dataset_fields, _DesignState, _Forward,
                            _frequency_extras, _penalties, _run_design_loop, _start_values)
from .frame_frequency import FrequencyFloor
from .frames import FrameCaseSolution, FrameConfig, FrameFactor, FrameTopology


class MemberGroups:
    """Which elements share a design variable: `groups` [Ne], the label (0 .. Ng-1, every label used) of every element.  Keeps the
    three int32 device tables of ops_frame_group_step_f32 -- `elem_group` [Ne], and the same map in CSR form, `group_ptr` [Ng+1] and
    `group_elems` [Ne] with the elements of a group in ascending order.  The C entry cannot validate device tables: the checks here,
    all before any device call, are what stands between a bad table and an out-of-range index in the kernel."""

    def __init__(self, topo: FrameTopology, groups):
        g = groups.detach().cpu().numpy() if torch.is_tensor(groups) else np.asarray(groups)
        if g.dtype.kind not in "iu":
            raise ValueError(f"groups must be an integer array, got dtype {g.dtype}")
        if g.shape != (topo.Ne,):
            raise ValueError(f"groups must be [{topo.Ne}] (one label per element), got {list(g.shape)}")
        g = g.astype(np.int64)
        if (g < 0).any():
            raise ValueError("groups: negative label")
        Ng = int(g.max()) + 1
        counts = np.bincount(g, minlength=Ng)
        if (counts == 0).any():
            raise ValueError(f"groups: labels must be 0 .. Ng-1 without a gap; label {int(np.flatnonzero(counts == 0)[0])} is not used")
        self.topo, self.Ng, self.Ne = topo, Ng, topo.Ne
        self.labels = g.astype(np.int32)
        self.ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.elems = np.argsort(g, kind="stable").astype(np.int32)        # stable: ascending inside a group
        t = lambda a: torch.as_tensor(a, dtype=torch.int32, device=topo.device)      # noqa: E731
        self.d_elem_group, self.d_group_ptr, self.d_group_elems = t(self.labels), t(self.ptr), t(self.elems)
        self._index = {}

    def index(self, dev) -> torch.Tensor:
        """`elem_group` as an int64 index on `dev`: I = X[:, index]."""
        dev = torch.device(dev)
        if dev not in self._index:
            self._index[dev] = torch.as_tensor(self.labels, dtype=torch.int64, device=dev)
        return self._index[dev]

    def expand(self, X: torch.Tensor) -> torch.Tensor:
        """I [G,Ne] = X[:, group[e]]."""
        return X[:, self.index(X.device)].contiguous()


def member_groups(topo: FrameTopology, groups) -> MemberGroups:
    """`MemberGroups` of `groups` (an int array [Ne], or a `MemberGroups` of this topology, passed through).  ValueError for a wrong
    length, a negative label, a gap in the labels or a dtype that is not an integer."""
    if isinstance(groups, MemberGroups):
        if groups.topo is not topo:
            raise ValueError("groups: a MemberGroups of another topology")
        return groups
    return MemberGroups(topo, groups)


def story_groups(topo: FrameTopology) -> np.ndarray:
    """Labels [Ne] int32 from geometry alone: vertical elements are columns, grouped by the rank of their lower end's y; horizontal
    elements are beams, grouped by the rank of their y; the column groups come first.  `grid_frame(b, s)`: 2 s groups.  An element
    that is neither vertical nor horizontal: ValueError."""
    a, b = topo.coords[topo.conn[:, 0]], topo.coords[topo.conn[:, 1]]
    vertical, horizontal = a[:, 0] == b[:, 0], a[:, 1] == b[:, 1]
    if not (vertical ^ horizontal).all():
        raise ValueError(f"story_groups: element {int(np.flatnonzero(~(vertical ^ horizontal))[0])} is neither vertical nor horizontal")
    y = np.where(vertical, np.minimum(a[:, 1], b[:, 1]), a[:, 1])
    labels = np.zeros(topo.Ne, dtype=np.int32)
    n_col = 0
    if vertical.any():
        levels = np.unique(y[vertical])
        labels[vertical] = np.searchsorted(levels, y[vertical])
        n_col = len(levels)
    if horizontal.any():
        levels = np.unique(y[horizontal])
        labels[horizontal] = n_col + np.searchsorted(levels, y[horizontal])
    return labels


def _checked_catalogue(catalogue) -> torch.Tensor:
    c = np.asarray(catalogue.detach().cpu().numpy() if torch.is_tensor(catalogue) else catalogue, dtype=np.float64).reshape(-1)
    if c.size < 1 or not np.isfinite(c).all() or (c <= 0).any() or (np.diff(c) <= 0).any():
        raise ValueError("catalogue must be a strictly ascending sequence of positive inertias")
    c32 = c.astype(np.float32)
    if (np.diff(c32) <= 0).any() or (c32 <= 0).any():
        raise ValueError("catalogue: entries must stay positive and strictly ascending in float32")
    return torch.as_tensor(c32)


def snap_to_catalogue(X: torch.Tensor, catalogue, mode: str = "up"):
    """Every variable to a catalogue entry -> (X_snapped float32, section int32: the entry's index, clipped bool), shaped as X.
    `catalogue`: a strictly ascending sequence of positive inertias (anything else: ValueError), taken in float32 as X is.  "up": the
    smallest entry >= x; "nearest": the closest entry, a tie goes up.  An x above the largest entry takes the largest and sets
    `clipped`.  Plain torch, on X's device."""
    if mode not in ("up", "nearest"):
        raise ValueError(f'mode must be "up" or "nearest", got {mode!r}')
    cat = _checked_catalogue(catalogue)
    if not torch.is_tensor(X) or not X.is_floating_point():
        raise ValueError("X must be a floating-point tensor")
    cat = cat.to(X.device)
    x = X.detach().to(torch.float32).contiguous()
    n = cat.numel()
    up = torch.searchsorted(cat, x)                        # the first entry >= x (n: none)
    clipped = up >= n
    up = up.clamp(max=n - 1)
    section = up
    if mode == "nearest":
        lo = (up - 1).clamp(min=0)
        d_lo, d_up = (x.double() - cat[lo].double()).abs(), (cat[up].double() - x.double()).abs()
        section = torch.where(d_lo < d_up, lo, up)          # a tie goes up
    return cat[section], section.to(torch.int32), clipped


class DiscreteDesigns(NamedTuple):
    X: torch.Tensor                  # [G, Ng] float32: the variables on the catalogue
    section: torch.Tensor            # [G, Ng] int32: the catalogue entry of every variable
    I: torch.Tensor                  # [G, Ne] float32: X expanded
    value: torch.Tensor              # [G] float32: the objective of the discrete design (`evaluate_frame_designs`)
    value_continuous: torch.Tensor   # [G] float32: the objective of the continuous design the loop returned
    clipped: torch.Tensor            # [G, Ng] bool: the variable was above the largest entry


class GroupedFrameDesigns(NamedTuple):
    X: torch.Tensor                  # [G, Ng] float32: the variables after their last step
    I: torch.Tensor                  # [G, Ne] float32: X expanded
    solution: FrameCaseSolution      # [G, C, ...]: every design's LAST solve (on the inertias that step started from)
    epochs: torch.Tensor             # [G] int32
    governing: torch.Tensor          # [G] int32
    case_penalty: torch.Tensor       # [G, C] float32
    discrete: Optional[DiscreteDesigns]      # None without a catalogue


class FrameDesignValues(NamedTuple):
    value: torch.Tensor              # [G] float32: the step's loss, sum I + the aggregated penalties
    case_penalty: torch.Tensor       # [G, C] float32
    governing: torch.Tensor          # [G] int32
    solution: FrameCaseSolution      # [G, C, ...]
    status: torch.Tensor             # [G, C] int32: the solve's


class _GroupState(_DesignState):
    """`_DesignState` whose step owns the groups' variables X [G,Ng]: Adam's moments and the optional gradient are [G,Ng]; I and I64
    are the expansion the step writes."""

    def __init__(self, groups: MemberGroups, X: torch.Tensor, I: torch.Tensor, I64: torch.Tensor, C: int, hp, obj, aggregate: int, weights,
                 with_grad: bool):
        super().__init__(groups.topo, I, I64, C, hp, obj, aggregate, weights, with_grad, n_vars=groups.Ng)
        self.groups, self.X = groups, X
        dev = I.device
        self.tables = tuple(t if t.device == dev else t.to(dev) for t in (groups.d_elem_group, groups.d_group_ptr, groups.d_group_elems))

    def step(self, fwd: FrameCaseSolution, lam: torch.Tensor, status_adj: Optional[torch.Tensor]) -> None:
        topo, I = self.topo, self.I
        entry, name = self._step_entry("group")
        with torch.cuda.device(I.device):
            rc = entry(I.shape[0], self.C, topo.Nn, topo.Ne, self.groups.Ng, topo.d_geo.data_ptr(), topo.d_E.data_ptr(),
                       frames._adjoint_tables(topo).conn.data_ptr(), *(t.data_ptr() for t in self.tables), self.X.data_ptr(), I.data_ptr(),
                       self.I64.data_ptr(), *self._step_tail(fwd, lam, status_adj))
        _cabi.check(rc, name)


def evaluate_frame_designs(topo: FrameTopology, I: torch.Tensor, loads: torch.Tensor, element_loads: Optional[torch.Tensor] = None, *,
                           cfg: Optional[FrameConfig] = None, aggregate: str = "sum", weights: Optional[Sequence[float]] = None,
                           alpha_sway: float = 0.0, sway_limit: Optional[float] = None, alpha_deflection: float = 0.0,
                           deflection_limit: Optional[float] = None, frequency: Optional[FrequencyFloor] = None) -> FrameDesignValues:
    """The objective of `optimize_frame_designs` for any designs I [G,Ne] (float32 or float64) under `loads` / `element_loads` (as
    there): one forward pass -- the keeping solve, the re-solve of the G*C rows, the correction for the element loads -- the hinge
    values when a displacement term is on, and the design step's loss on scratch state (the step is given no adjoint: its loss,
    penalties and governing case do not depend on one).  The existing launches, nothing of the caller's written.  The penalties are
    formed in float32 on I.float(), the solve runs on I.double().  `frequency`: a `FrequencyFloor`; the value then is the plain value
    + (float)P_f of a cold iteration of the term's `start_iters` on this forward's factor, and the term's `.modes` / `.penalty` are
    those.  Returns `FrameDesignValues`."""
    cfg = cfg or FrameConfig()
    obj = _penalties(alpha_sway, sway_limit, alpha_deflection, deflection_limit)
    if not torch.is_tensor(I) or I.dim() != 2 or I.shape[1] != topo.Ne or I.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"I must be float32 or float64 [G, {topo.Ne}]")
    q = _checked_problem(topo, loads, element_loads, None, I, "I", topo.Ne, aggregate, weights, "evaluate_frame_designs", frequency)
    dev = q.dev
    hp = frames._sizing_params(cfg, 1)
    st = _DesignState(topo, I.to(dtype=torch.float32, device=dev).clone(), I.to(dtype=torch.float64, device=dev).clone(), q.C, hp, obj,
                      q.agg, q.w_c, with_grad=False)
    fw = _Forward(topo, st.I64, q)
    if q.G:
        fw()
        if st.loss_extra is not None:
            st.adjoint_rhs(fw.fwd)
        st.rhs.zero_()                            # no adjoint: the step's loss does not read it
        _frequency_extras(st, frequency, fw.factor)
        st.step(fw.fwd, st.rhs, None)
        torch.cuda.synchronize(dev)
        if frequency is not None:
            frequency.finish()
    return FrameDesignValues(st.last, st.case_penalty, st.governing, fw.fwd, fw.fwd.status)


def optimize_grouped_frame_designs(topo: FrameTopology, groups, loads: torch.Tensor, element_loads: Optional[torch.Tensor] = None, *,
                                   X0: Optional[torch.Tensor] = None, catalogue=None, snap: str = "up", n_designs: Optional[int] = None,
                                   cfg: Optional[FrameConfig] = None, aggregate: str = "sum", weights: Optional[Sequence[float]] = None,
                                   alpha_sway: float = 0.0, sway_limit: Optional[float] = None, alpha_deflection: float = 0.0,
                                   deflection_limit: Optional[float] = None, max_epochs: Optional[int] = None, poll_every: int = 25,
                                   loss_history: Optional[list] = None, frequency: Optional[FrequencyFloor] = None) -> GroupedFrameDesigns:
    """`optimize_frame_designs` with linked design variables.  `groups`: int [Ne], the label 0 .. Ng-1 of every
    element (`story_groups(topo)`: columns by story, beams by floor), or a `MemberGroups`.  `X0` [G,Ng] float32: the start (default
    cfg.I0).  The loop steps on X [G,Ng]; the element inertias are X[:, groups].  Six launches and one factorisation per epoch, as
    there, with ops_frame_group_step_f32 as the step; the other keywords, the limits (half bandwidth <= 55, C <= 64, Ne <= 512) and
    `loss_history` are those of `optimize_frame_designs`.  `catalogue`: a strictly ascending sequence of positive inertias; after the
    loop X is snapped to it (`snap`: "up" or "nearest"), expanded, and both designs are evaluated (`evaluate_frame_designs`) into
    `discrete`.  `frequency`: a `FrequencyFloor`, as in `optimize_frame_designs`; its gradient joins the element gradients before
    the per-group sum, and with a `catalogue` both evaluations carry the term (its `.modes` / `.penalty` are then the continuous
    design's, evaluated last).  Returns `GroupedFrameDesigns`."""
    cfg = cfg or FrameConfig()
    penalties = dict(alpha_sway=alpha_sway, sway_limit=sway_limit, alpha_deflection=alpha_deflection, deflection_limit=deflection_limit)
    obj = _penalties(**penalties)
    mg = member_groups(topo, groups)              # the tables' checks: before any device call
    if snap not in ("up", "nearest"):
        raise ValueError(f'snap must be "up" or "nearest", got {snap!r}')
    if catalogue is not None:
        _checked_catalogue(catalogue)
    q = _checked_problem(topo, loads, element_loads, n_designs, X0, "X0", mg.Ng, aggregate, weights, "optimize_grouped_frame_designs", frequency)
    n_max = max_epochs if max_epochs is not None else cfg.num_epochs
    X = _start_values(X0, q.G, mg.Ng, cfg, q.dev)
    I = mg.expand(X)
    st = _GroupState(mg, X, I, I.double(), q.C, frames._sizing_params(cfg, n_max), obj, q.agg, q.w_c, with_grad=False)
    fw = _run_design_loop(st, q, n_max, poll_every, loss_history, frequency)
    discrete = None
    if catalogue is not None:
        Xd, section, clipped = snap_to_catalogue(X, catalogue, snap)
        Id = mg.expand(Xd)
        ev = dict(cfg=cfg, aggregate=aggregate, weights=weights, frequency=frequency, **penalties)
        discrete = DiscreteDesigns(Xd, section, Id, evaluate_frame_designs(topo, Id, q.loads, q.w, **ev).value,
                                   evaluate_frame_designs(topo, I, q.loads, q.w, **ev).value, clipped)
    return GroupedFrameDesigns(X, I, fw.fwd, st.epochs, st.governing, st.case_penalty, discrete)


def frame_group_gradient(factor: FrameFactor, sol: FrameCaseSolution, groups, hp, *, aggregate: str = "sum",
                         weights: Optional[Sequence[float]] = None, alpha_sway: float = 0.0, sway_limit: Optional[float] = None,
                         alpha_deflection: float = 0.0, deflection_limit: Optional[float] = None,
                         frequency: Optional[FrequencyFloor] = None, modes=None):
    """`frame_design_gradient` by group: dL/dX [G,Ng] (float64) of the aggregated design objective with X the groups' variables, from a
    caller's `frame_factor(topo, I)` with I = X[:, groups] and the solution `sol` of `frame_resolve(factor, ...)`.  The adjoint
    right-hand sides, one re-solve on the kept factor and the group step with its state in scratch tensors: nothing of the caller's
    is written.  `frequency`, `modes`: as there; the term's element gradient joins before the per-group sum.  Returns (grad,
    loss_extra [G,C] or None, governing [G] int32)."""
    obj = _penalties(alpha_sway, sway_limit, alpha_deflection, deflection_limit)
    mg = member_groups(factor.topo, groups)
    q = _checked_gradient_inputs(factor, sol, hp, aggregate, weights, "frame_group_gradient", frequency, modes)
    I64 = q.I64
    # the variables as the step reads them: a group's first element speaks for it (I = X[:, groups] is the caller's promise)
    first = torch.as_tensor(mg.elems[mg.ptr[:-1]].astype(np.int64), device=I64.device)
    X = I64[:, first].float().contiguous()
    st = _GroupState(mg, X, I64.float(), I64.clone(), q.C, q.hp, obj, q.agg, q.w_c, with_grad=True)
    if q.G:
        _frequency_extras(st, frequency, factor, modes)
        st.gradient_and_step(factor, sol)
        if frequency is not None and modes is None:
            frequency.finish()
    return st.grad, st.loss_extra, st.governing


def generate_grouped_frame_design_dataset(num_bays: int, num_stories: int, n_designs: int, n_load_cases: int,
                                          groups: Union[str, Sequence[int], np.ndarray] = "story", catalogue=None, snap: str = "up",
                                          cfg: Optional[FrameConfig] = None, lateral_range=(0.5e4, 2e4), vertical_range=(-2e4, -0.5e4),
                                          seed: int = 0, aggregate: str = "sum", weights: Optional[Sequence[float]] = None,
                                          max_epochs: Optional[int] = None, **objective) -> dict:
    """`generate_frame_design_dataset` with linked member groups (`groups`: "story" = `story_groups`, or labels [Ne]) and an optional
    catalogue: the same draws, sized in one batch by `optimize_grouped_frame_designs`.  Returns its CPU tensors plus X [G,Ng] float32
    and groups [Ne] int32, and with a catalogue the discrete fields: discrete_X, discrete_section, discrete_I, discrete_value,
    discrete_value_continuous, discrete_clipped."""
    cfg = cfg or FrameConfig()
    G, C = int(n_designs), int(n_load_cases)
    if isinstance(groups, str) and groups != "story":
        raise ValueError(f'groups must be "story" or an array of labels, got {groups!r}')
    topo = frames.grid_frame(num_bays, num_stories, cfg)
    if isinstance(groups, str):
        groups = story_groups(topo)
    mg = member_groups(topo, groups)
    lateral, vertical = frames.frame_dataset_draws(G * C, lateral_range, vertical_range, seed)
    loads, w = frames.grid_load_cases(topo, lateral, vertical)
    r = optimize_grouped_frame_designs(topo, mg, loads.reshape(G, C, topo.Nn, 3), w.reshape(G, C, topo.Ne, 2), n_designs=G, cfg=cfg,
                                       catalogue=catalogue, snap=snap, aggregate=aggregate, weights=weights, max_epochs=max_epochs, **objective)
    out = dict(X=r.X.cpu(), groups=torch.as_tensor(mg.labels), **_dataset_fields(r, lateral, vertical, G, C))
    if r.discrete is not None:
        out.update({"discrete_" + k: v.cpu() for k, v in r.discrete._asdict().items()})
    return out
