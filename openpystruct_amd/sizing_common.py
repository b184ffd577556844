"""What the sizing loops share on the host (beams: sizing.py, multicase.py; frames: frames.py, frame_designs.py, frame_groups.py; the
design loss beside them): the checks of the objective's and the aggregate's arguments, the optimiser state every loop starts from and
its step-size table, the one launch of the optimiser step (csrc/sizing_step.hip, csrc/sizing_grad.hip: one step-kernel family), the
eager "run epochs, poll `active` every k" loop, the replay loop of a captured poll interval with its lagging poll, and the driver
that chooses between the two.  Nothing here knows a beam from a frame."""
from __future__ import annotations

import collections
import ctypes
from typing import Callable, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _cabi

GRADIENTS = ("explicit", "total")
AGGREGATES = ("sum", "max")


def checked_objective(gradient: str, terms: Sequence[Tuple[str, float, Optional[float]]]) -> tuple:
    """(gradient, alpha_1, limit_1, ...) of a sizing run from its (name, alpha, limit) penalty terms, checked.  "explicit": the
    reference's gradient (M and V held fixed), which cannot see a displacement term; "total": the gradient of the loss through the
    solve.  The limits are penalties, not constraints; a term with alpha == 0 is absent and its limit is stored as 0.0."""
    if gradient not in GRADIENTS:
        raise ValueError(f"gradient must be one of {GRADIENTS}, got {gradient!r}")
    out = [gradient]
    for name, alpha, limit in terms:
        alpha = float(alpha)
        if not alpha >= 0.0:
            raise ValueError(f"alpha_{name} must be >= 0")
        if alpha > 0.0:
            if gradient == "explicit":
                raise ValueError(f'alpha_{name} > 0 needs gradient="total": the {name} term depends on I only through the solve, '
                                 "the explicit gradient is blind to it")
            if limit is None or not float(limit) > 0.0:
                raise ValueError(f"alpha_{name} > 0 needs a {name}_limit > 0")
        out += [alpha, float(limit) if alpha > 0.0 else 0.0]
    return tuple(out)


def checked_aggregate(aggregate: str, weights, C: Optional[int] = None) -> tuple:
    """(the aggregate's index, `weights` -- a sequence, an array or a tensor -- as a float64 numpy [C] or None), checked.  C None: the
    name alone, for a caller that has other refusals to make before the weights' values, and calls again with C."""
    if aggregate not in AGGREGATES:
        raise ValueError(f"aggregate must be one of {AGGREGATES}, got {aggregate!r}")
    if aggregate == "max" and weights is not None:
        raise ValueError('aggregate="max" takes no weights: the governing case is the largest unweighted penalty')
    if weights is not None and C is not None:
        weights = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64).reshape(-1)
        if weights.shape != (C,) or not np.isfinite(weights).all() or (weights < 0).any():
            raise ValueError(f"weights must be {C} finite non-negative numbers")
    return AGGREGATES.index(aggregate), weights


def step_schedule(hp, device) -> torch.Tensor:
    """The tabulated Adam step sizes of `hp` (an `ops_sizing_params`) on `device`: [max(max_epochs, 1), 2] float32, per epoch the
    step size and the bias correction."""
    sched = np.zeros((max(int(hp.max_epochs), 1), 2), dtype=np.float32)
    _cabi.load().ops_sizing_schedule_f32(ctypes.byref(hp), sched.ctypes.data)
    return torch.as_tensor(sched, device=device)


class _StepState(NamedTuple):
    """The tensors the optimiser step kernels update in place, one row per case (beam or frame)."""
    I: torch.Tensor                 # [B,Ne] float32: the design
    I64: torch.Tensor               # [B,Ne] float64: the design as the solve reads it
    exp_avg: torch.Tensor           # [B,Ne] float32 (Adam)
    exp_avg_sq: torch.Tensor        # [B,Ne] float32
    best: torch.Tensor              # [B] float32: early stopping
    patience_cnt: torch.Tensor      # [B] int32
    epochs: torch.Tensor            # [B] int32
    active: torch.Tensor            # [B] uint8
    last: torch.Tensor              # [B] float32: the epoch's total_loss
    V32: Optional[torch.Tensor]     # [B,Ne] float32 records of the step's rounded forces; both None: not recorded
    M32: Optional[torch.Tensor]


# what Adam and the early stop keep per row (a case, a frame or a design -- [rows, n_vars] and [rows]), in the step entry points' order
OptimiserState = collections.namedtuple("OptimiserState", _StepState._fields[2:9])


def new_optimiser_state(rows: int, n_vars: int, device) -> OptimiserState:
    """The tensors of an `OptimiserState`, allocated and not yet armed."""
    f32, i32 = dict(dtype=torch.float32, device=device), dict(dtype=torch.int32, device=device)
    return OptimiserState(torch.empty((rows, n_vars), **f32), torch.empty((rows, n_vars), **f32), torch.empty((rows,), **f32),
                          torch.empty((rows,), **i32), torch.empty((rows,), **i32), torch.empty((rows,), dtype=torch.uint8, device=device),
                          torch.empty((rows,), **f32))


def arm_optimiser_state(s: OptimiserState) -> OptimiserState:
    """The state before the first epoch, written IN PLACE (a captured graph may point at these tensors): the one statement of it."""
    for t in (s.exp_avg, s.exp_avg_sq, s.patience_cnt, s.epochs, s.last):
        t.zero_()
    s.best.fill_(float("inf"))
    s.active.fill_(1)
    return s


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _sizing_step(st: _StepState, V: torch.Tensor, M: torch.Tensor, hp, grad: Optional[torch.Tensor] = None,
                 loss_extra: Optional[torch.Tensor] = None, schedule: Optional[torch.Tensor] = None) -> None:
    """One optimiser step with the early-stop bookkeeping, on the current stream; the only caller of the three step entry points.
    `grad` [B,Ne] float64: step on it (and add `loss_extra` [B] to the loss); None: on the explicit gradient formed from the forces
    (V, M) [B,Ne] of the epoch's solve -- float64, rounded by the kernel, or the float32 rows of a forces-only solve.  `schedule`:
    the tabulated Adam step sizes (the float64 explicit entry point takes none).  No checks, no allocation."""
    lib = _cabi.load()
    B, Ne = st.I.shape
    dev = st.I.device
    design = (B, Ne, st.I.data_ptr(), st.I64.data_ptr(), V.data_ptr(), M.data_ptr())
    state = (*(t.data_ptr() for t in st[2:9]), _ptr(st.V32), _ptr(st.M32))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if grad is not None:
            name, rc = "ops_beam_sizing_step_grad_f32", lib.ops_beam_sizing_step_grad_f32(
                *design, grad.data_ptr(), _ptr(loss_extra), *state, ctypes.byref(hp), _ptr(schedule), stream)
        elif V.dtype == torch.float32:       # (V, M) are the V32 / M32 records themselves: the entry point writes none
            name, rc = "ops_beam_sizing_step_vm32_f32", lib.ops_beam_sizing_step_vm32_f32(
                *design, *state[:-2], ctypes.byref(hp), _ptr(schedule), stream)
        else:
            name, rc = "ops_beam_sizing_step_f32", lib.ops_beam_sizing_step_f32(*design, *state, ctypes.byref(hp), stream)
    _cabi.check(rc, name)


def run_epochs(epoch: Callable[[], None], n_max: int, poll_every: int, active, after_epoch: Optional[Callable[[], None]] = None) -> int:
    """The eager loop: `epoch()` up to `n_max` times, `after_epoch()` after each; once per `poll_every` epochs the host reads
    `active` (one sync) and stops when no row is active.  Returns the number of epochs run."""
    done = 0
    while done < n_max:
        epoch()
        done += 1
        if after_epoch is not None:
            after_epoch()
        if done % poll_every == 0 and not bool(active.any()):
            break
    return done


def replay_epochs(graph, n_max: int, poll_every: int, done: int, active: torch.Tensor, flags: torch.Tensor, events, lag: int = 1) -> int:
    """The captured loop: replay `graph` (`poll_every` epochs) until `n_max` epochs are queued or no row is active; `done` epochs
    ran before.  The "any row still active?" poll lags `lag` replays: its answer travels through a pinned flag (`flags`, 2 x uint8)
    behind an event (`events`, 2), and the host reads the flag of replay k - lag after it has queued replay k -- the device never
    waits for the host (a blocking poll drained the queue 13 times per 50 000-case shard, ~40 us each); the price is one replay of
    skipped wavefronts.  Returns the number of epochs queued."""
    flags.zero_()
    k = 0
    while done < n_max:
        graph.replay()
        done += poll_every
        flags[k & 1: (k & 1) + 1].copy_(active.any().to(torch.uint8).reshape(1), non_blocking=True)
        events[k & 1].record()
        if k >= lag:
            events[(k - lag) & 1].synchronize()
            if int(flags[(k - lag) & 1]) == 0:
                break
        k += 1
    return done


def poll_flags() -> tuple:
    """The (pinned flag pair, two events) `replay_epochs` polls through.  Pinned allocations are slow: a caller that runs many loops
    keeps one."""
    return torch.zeros(2, dtype=torch.uint8).pin_memory(), [torch.cuda.Event(), torch.cuda.Event()]


def history_callback(history: Optional[list], last: torch.Tensor) -> Optional[Callable[[], None]]:
    """The `after_epoch` that appends a copy of `last` (the epoch's loss per row) to `history`; None without a list."""
    return None if history is None else lambda: history.append(last.clone())


def run_sizing_loop(epoch: Callable[[], None], n_max: int, poll_every: int, active: torch.Tensor, last: torch.Tensor, device, *,
                    use_graph: bool, record: bool = False, graph=None, poll: Optional[tuple] = None, lag: int = 1) -> tuple:
    """The beam loops' driver.  `use_graph`: `poll_every` epochs replayed as one HIP graph (the epoch body is launch-bound) through
    `replay_epochs` with `poll` (None: a new `poll_flags()`) and `lag` -- `graph` when the caller kept one of this very `epoch`, else
    captured here after one eager epoch, the warm-up outside capture (it allocates the solution buffers).  Otherwise `run_epochs`,
    with `record` keeping every epoch's `last`.  Returns (the graph used or None, the history [epochs, rows] or None)."""
    if use_graph:
        done = 0
        if graph is None:
            from .runtime import capture_graph
            graph, _ = capture_graph(torch.cuda.Stream(device=device), device, lambda: [epoch() for _ in range(poll_every)], 1, warm=epoch)
            done = 1
        replay_epochs(graph, n_max, poll_every, done, active, *(poll or poll_flags()), lag=lag)
        return graph, None
    history = [] if record else None
    run_epochs(epoch, n_max, poll_every, active, history_callback(history, last))
    return None, (torch.stack(history) if history else last.new_zeros((0, last.shape[0]))) if record else None
