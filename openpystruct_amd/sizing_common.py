"""What the two sizing loops share on the host (beams: sizing.py, frames: frames.py): the check of the objective's arguments, the one
launch of the optimiser step (csrc/sizing_step.hip, csrc/sizing_grad.hip: both loops use one step-kernel family), the eager
"run epochs, poll `active` every k" loop and the replay loop of a captured poll interval with its lagging poll.  Nothing here knows
a beam from a frame."""
from __future__ import annotations

import ctypes
from typing import Callable, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _cabi

GRADIENTS = ("explicit", "total")


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
