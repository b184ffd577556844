"""Data-parallel training loops of the two surrogates (one process per GPU, RCCL all-reduce over xGMI).

Restates the reference's single-device loops
(/root/reference/OpenPyStruct_PINN_MultiCase.py:741-852,
 /root/reference/OpenPyStruct_TransformerDiffusionModule_MultiCase.py:722-829):
per epoch: decaying input noise, shuffled batches, in-batch permutation, autocast forward, loss,
backward, clip_grad_norm_(1.0), Adam step; then a validation pass, ExponentialLR step, early stopping on
the validation loss with best-state checkpointing; finally R^2 of the un-standardised inertias.

What is different, and why (DESIGN.md "Training loops"):
  * bf16 autocast without a GradScaler instead of fp16 + GradScaler (BASELINE config 4; MI355X bf16 MFMA) by default; the reference's own
    mode -- `autocast(float16)` + `GradScaler` (PINN:706, :759-768) -- is `train_surrogate(..., autocast_dtype=torch.float16)` (r06): framework
    modules under fp16 autocast, loss scaling with the GradScaler's rule (skip the step and halve the scale on a non-finite gradient, double it
    after 2 000 clean steps), eager steps (the scale and the skip decision change from step to step);
  * the dataset is resident on the GPU: no per-batch host-to-device copies (PINN:749-750) and no per-step
    `.item()` (PINN:770) -- losses are accumulated on the device and reduced once per epoch;
  * data parallelism by hand instead of the DistributedDataParallel wrapper: every parameter's .grad is a
    view into ONE flat float32 buffer (the models are 1.4 - 2.4 MB), which is all-reduced with a single
    RCCL call per step (latency-bound over xGMI; nothing to bucket or overlap at this size).  That keeps the
    step capturable: [noise, forward, loss, backward] and [scale, clip, Adam] are two HIP graphs with the one
    collective between them, so the multi-GPU step costs three launches, like the single-GPU one costs one.
    Weak scaling: every rank trains on its own shard with the reference's per-GPU batch size;
  * early-stop decisions are taken on all-reduced losses, so every rank stops at the same epoch.
BatchNorm batch statistics are per rank (as per process in the reference; pass sync_bn=True for SyncBatchNorm);
the running statistics are averaged over ranks at the end of every epoch so that the replicas stay identical.
"""
from __future__ import annotations

import copy
import os
import sys
import time
import types
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Union

import torch
import torch.distributed as dist
import torch.nn as nn
from torch.optim.lr_scheduler import ExponentialLR

from . import _cabi, switches
from .dataprep import SurrogateData
from .flat_adam import FlatClipAdam, flat_grads
from .shadow import disable_shadow_linears, enable_shadow_linears, grouped_wgrads      # (functions only: shadow's two rebound globals have no copy here)
from .surrogates import fused_loss, BayesianTransformerWithDiffusion, ChainGNN, CompositeLoss, FNO1dModel, FNNPlain, FNNWithResidual, ModelOnePassTransformerWithDiffusion, TrainableL1L2Loss


@dataclass
class PinnConfig:
    """PINN:35-56."""
    n_cases: int = 6
    nelem: int = 100
    box_constraint_coeff: float = 1e-1
    hidden_units: int = 350
    dropout_rate: float = 0.5
    num_blocks: int = 2
    num_epochs: int = 500
    batch_size: int = 128
    patience: int = 10
    learning_rate: float = 5e-4
    weight_decay: float = 1e-3
    train_split: float = 0.8
    sigma_0: float = 0.01
    gamma_noise: float = 0.99
    gamma: float = 0.98
    initial_alpha: float = 0.5
    c: float = 0.5
    penalty_pinn: float = 1.5e-6


@dataclass
class TfdConfig:
    """TFD:36-60."""
    n_cases: int = 6
    nelem: int = 100
    box_constraint_coeff: float = 5e-1
    hidden_units: int = 256
    dropout_rate: float = 0.1
    num_epochs: int = 500
    batch_size: int = 512
    patience: int = 10
    learning_rate: float = 3e-3
    weight_decay: float = 1e-4
    train_split: float = 0.8
    sigma_0: float = 0.01
    gamma_noise: float = 0.90
    gamma: float = 0.95
    initial_alpha: float = 0.5
    c: float = 0.5
    num_transformer_layers: int = 2
    dim_feedforward: int = 256
    num_heads: int = 8
    max_len: int = 512
    diffusion_hidden_dim: int = 256
    diffusion_T: int = 512


@dataclass
class BtfdConfig:
    """OpenPyStruct_Bayesian_TFDModule_MultiCase_Beta.py:36-66.  kl: "none" reproduces the script as it runs (its KL sum
    is over modules with a `kl_loss` method: none); "gaussian" adds bnn_kl_scale * bayes.bayesian_kl(model)."""
    n_cases: int = 6
    nelem: int = 100
    box_constraint_coeff: float = 5e-1
    hidden_units: int = 512
    dropout_rate: float = 0.1
    num_epochs: int = 500
    batch_size: int = 512
    patience: int = 10
    learning_rate: float = 3e-4
    weight_decay: float = 1e-6
    train_split: float = 0.8
    sigma_0: float = 0.01
    gamma_noise: float = 0.95
    gamma: float = 0.99
    initial_alpha: float = 0.5
    c: float = 0.5
    bnn_kl_scale: float = 1e-6
    num_transformer_layers: int = 4
    dim_feedforward: int = 512
    num_heads: int = 24
    max_len: int = 512
    diffusion_hidden_dim: int = 512
    diffusion_T: int = 512
    kl: str = "none"


@dataclass
class BtfdmConfig(BtfdConfig):
    """The _Meta_ script: n_cases 8, dropout 0.01, c 1 (and the model's trainable output_scales)."""
    n_cases: int = 8
    dropout_rate: float = 0.01
    c: float = 1.0


@dataclass
class FnnConfig:
    """/root/reference/OpenPyStruct_FNN_MultiCase.py:35-52 (num_blocks = 3 is unused there: the model is built with 4)."""
    n_cases: int = 6
    nelem: int = 100
    box_constraint_coeff: float = 5e-1
    hidden_units: int = 128
    dropout_rate: float = 0.5
    num_residual_blocks: int = 4
    num_epochs: int = 500
    batch_size: int = 128
    patience: int = 10
    learning_rate: float = 2e-4
    weight_decay: float = 1e-2
    train_split: float = 0.8
    sigma_0: float = 0.03
    gamma_noise: float = 0.97
    gamma: float = 0.99
    initial_alpha: float = 0.5
    c: float = 1.0


@dataclass
class GnnConfig:
    """/root/reference/OpenPyStruct_GNN_MultiCase_Beta.py:38-55 (AdamW, no alpha term, :394, :437-446)."""
    n_cases: int = 6
    nelem: int = 100
    box_constraint_coeff: float = 5e-1
    encoder_hidden_dim: int = 128
    gnn_hidden_dim: int = 128
    num_gnn_layers: int = 2
    dropout_rate: float = 0.5
    num_epochs: int = 500
    batch_size: int = 512
    patience: int = 10
    learning_rate: float = 3e-3
    weight_decay: float = 1e-2
    train_split: float = 0.8
    sigma_0: float = 0.01
    gamma_noise: float = 0.99
    gamma: float = 0.975
    initial_alpha: float = 0.5
    c: float = 0.5


@dataclass
class FnoConfig:
    """/root/reference/OpenPyStruct_FNO_MultiCase_Beta.py:34-58 (Adam, autocast disabled, alpha term, :561, :613-617)."""
    n_cases: int = 6
    nelem: int = 100
    box_constraint_coeff: float = 5e-1
    hidden_units: int = 512
    dropout_rate: float = 0.1
    num_fno_layers: int = 4
    num_epochs: int = 500
    batch_size: int = 512
    patience: int = 10
    learning_rate: float = 3e-3
    weight_decay: float = 1e-6
    train_split: float = 0.8
    sigma_0: float = 0.01
    gamma_noise: float = 0.95
    gamma: float = 0.975
    initial_alpha: float = 0.5
    c: float = 0.5
    fno_modes: int = 4
    fno_width: int = 128


_FUSED_LOSS = switches.get("fused_loss") == "1"      # A/B switch: 0 = the nn.Module losses
_SHADOW_LINEAR = switches.get("shadow_linear") == "1"   # A/B switch: 0 = nn.Linear under autocast
_GROUP_WGRAD = switches.get("group_wgrad") == "1"    # A/B switch: 0 = one launch per product, inside backward
_EXPLICIT_ROOT = switches.get("explicit_root") == "1"      # A/B switch: 0 = loss.backward() with its implicit ones_like() fill node
_DEBUG_NAN = os.environ.get("OPS_AMD_DEBUG_NAN", "0") == "1"
# data-parallel step (world > 1).  Default: [graph A: noise, forward, loss, backward] -> gradient all-reduce -> [graph B: average, clip,
# Adam], the collective enqueued asynchronously (the host never blocks on it: `wait()` only orders the compute stream behind the
# collective's) -- OPS_AMD_DP_ASYNC=0 is the plain blocking-call form, bit for bit the same arithmetic (tests/test_surrogates.py).
# r06: under `nccl` the collective is captured too -- the whole step is ONE graph, one replay per step and no host work between its segments
# (one-rank RCCL timing, profiles/r05_notes.md 6: PINN 137.5 us against 169.1 us for two graphs around an eager collective, TFD 191.3 / 219.8;
# the same bits as the plain run).  A failure while capturing falls back to the two-graph form; a captured collective that goes wrong on
# N > 1 ranks would hang at REPLAY, past every fallback, so the first replay runs under a timer that ends the rank with exit code 17
# (OPS_AMD_DP_STALL_S seconds, default 120: the launcher then takes the job down; a fresh job may set OPS_AMD_DP_ONE_GRAPH=0 -- never a re-exec
# from a process that holds the GPU).  OPS_AMD_DP_ONE_GRAPH=0: [graph A | all-reduce | graph B].
_DP_ASYNC = os.environ.get("OPS_AMD_DP_ASYNC", "1") == "1"
_DP_ONE_GRAPH = os.environ.get("OPS_AMD_DP_ONE_GRAPH", "1") == "1"
_DP_STALL_S = float(os.environ.get("OPS_AMD_DP_STALL_S", "120"))
_FORCE_DP = os.environ.get("OPS_AMD_FORCE_DP", "0") == "1"           # run the data-parallel branch with a one-rank process group too
_DP_PROFILE = os.environ.get("OPS_AMD_DP_PROFILE", "0") == "1"       # HIP events around the step's segments, reported as out["dp_segments"]

stall_hook = None     # callable(what) run by a firing _StallGuard just before the process ends


class _StallGuard:
    """`with _StallGuard(seconds, what):` -- if the block has not finished after `seconds`, the process ends with exit code 17 and a line on
    stderr saying what stalled (a hung graph replay of a captured collective cannot be recovered inside the process)."""

    def __init__(self, seconds: float, what: str):
        self.seconds, self.what, self.timer = seconds, what, None

    def _fire(self):
        if stall_hook is not None:       # the caller's last words (bench.py: the FE record measured before the training part)
            try:
                stall_hook(self.what)
            except Exception:
                pass
        sys.stderr.write(f"openpystruct_amd: {self.what} did not finish within {self.seconds:.0f} s -- ending this rank (exit 17); "
                         f"run again with OPS_AMD_DP_ONE_GRAPH=0 for the two-graph step\n")
        sys.stderr.flush()
        os._exit(17)

    def __enter__(self):
        import threading
        self.timer = threading.Timer(self.seconds, self._fire)
        self.timer.daemon = True
        self.timer.start()
        return self

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


_ROOT_ONES = {}


def _root_ones(device):
    key = (device.type, device.index)
    if key not in _ROOT_ONES:
        _ROOT_ONES[key] = torch.ones((), dtype=torch.float32, device=device)
    return _ROOT_ONES[key]


def clear_blas_workspaces() -> None:
    """Drop the framework's cached BLAS workspaces at the END of a training run (the caller has synchronised).  One that was allocated
    while a HIP graph was being captured lives in that graph's private pool but stays cached per (handle, stream): a later run whose
    side stream gets the same id would hand the freed memory to its GEMMs as scratch space.  (Calling this at the START of a run as
    well made things worse -- 4 NaN runs of 12 against 0 of 12, profiles/r03_notes.md 8 -- so it is not.)"""
    clear = getattr(torch._C, "_cuda_clearCublasWorkspaces", None)
    if clear is not None:
        clear()


class _TieTerms(torch.autograd.Function):
    """Two scalar loss terms as one backward root without a launch: forward = a view of the first, backward = the root gradient to both."""

    @staticmethod
    def forward(ctx, a, b):
        return a.view_as(a)

    @staticmethod
    def backward(ctx, g):
        return g, g


def _debug_nan(model, opt, flat, s_loss, epoch, b, sX, sY):
    """Diagnostics (OPS_AMD_DEBUG_NAN=1; run with OPS_AMD_ADAM_ZERO=0 to keep the gradients): first step with a non-finite value."""
    torch.cuda.synchronize()
    bad_p = [n for n, q in model.named_parameters() if not bool(torch.isfinite(q).all())]
    bad_g = [n for n, q in model.named_parameters() if q.grad is not None and not bool(torch.isfinite(q.grad).all())]
    if bad_p or bad_g or not bool(torch.isfinite(s_loss)):
        print("DEBUG_NAN epoch", epoch, "batch", b, "loss", float(s_loss), "inputs finite", bool(torch.isfinite(sX.float()).all()), bool(torch.isfinite(sY).all()),
              "gradnorm", float(flat.norm()), "\n  bad grads", bad_g[:12], "\n  bad params", bad_p[:6], flush=True)
        for n, q in model.named_parameters():
            if n in bad_g:
                idx = (~torch.isfinite(q.grad)).nonzero().flatten()[:40].tolist()
                print("   ", n, tuple(q.shape), "non-finite at", idx, "values", q.grad.flatten()[idx[:6]].tolist(), flush=True)
        raise RuntimeError("non-finite value in the training step")


def build_model_and_loss(kind: str, cfg, data: SurrogateData, device):
    if kind == "pinn":
        out_dim = cfg.nelem + 2 * (cfg.nelem + 1)
        model = FNNWithResidual(data.X_train.shape[1], cfg.hidden_units, cfg.num_blocks, out_dim, cfg.dropout_rate)   # PINN:687-693
        crit = CompositeLoss(cfg.nelem, cfg.nelem + 1, cfg.nelem + 1, cfg.initial_alpha, cfg.box_constraint_coeff,
                             data.min_constraint, data.max_constraint, cfg.penalty_pinn)                              # PINN:698-699
    elif kind == "tfd":
        model = ModelOnePassTransformerWithDiffusion(cfg.n_cases, data.feat_dim, cfg.nelem, cfg.hidden_units,
                                                     cfg.num_transformer_layers, cfg.num_heads, cfg.dim_feedforward,
                                                     cfg.dropout_rate, cfg.max_len, cfg.diffusion_hidden_dim, cfg.diffusion_T)  # TFD:664-676
        crit = TrainableL1L2Loss(cfg.initial_alpha, data.min_constraint, data.max_constraint, cfg.box_constraint_coeff)       # TFD:680
    elif kind in ("btfd", "btfdm"):
        model = BayesianTransformerWithDiffusion(cfg.n_cases, data.feat_dim, cfg.nelem, cfg.hidden_units, cfg.num_transformer_layers,
                                                 cfg.num_heads, cfg.dim_feedforward, cfg.dropout_rate, cfg.max_len, cfg.diffusion_hidden_dim,
                                                 cfg.diffusion_T, output_scales=kind == "btfdm")                # BTFD:640-653
        crit = TrainableL1L2Loss(cfg.initial_alpha, data.min_constraint, data.max_constraint, cfg.box_constraint_coeff)
    elif kind == "gnn":
        model = ChainGNN(data.X_train.shape[1], cfg.nelem, cfg.encoder_hidden_dim, cfg.gnn_hidden_dim, cfg.num_gnn_layers, cfg.dropout_rate)
        crit = TrainableL1L2Loss(cfg.initial_alpha, data.min_constraint, data.max_constraint, cfg.box_constraint_coeff)
    elif kind == "fno":
        model = FNO1dModel(cfg.n_cases, data.feat_dim, cfg.nelem, cfg.fno_modes, cfg.fno_width, cfg.num_fno_layers, cfg.hidden_units,
                           cfg.dropout_rate)
        crit = TrainableL1L2Loss(cfg.initial_alpha, data.min_constraint, data.max_constraint, cfg.box_constraint_coeff)
    elif kind == "fnn":
        model = FNNPlain(data.X_train.shape[1], cfg.hidden_units, cfg.num_residual_blocks, cfg.nelem, cfg.dropout_rate)
        crit = TrainableL1L2Loss(cfg.initial_alpha, data.min_constraint, data.max_constraint, cfg.box_constraint_coeff)
    else:
        raise ValueError(kind)
    return model.to(device), crit.to(device)


@dataclass
class PhysicsTerm:
    """Optional FE-residual term (physics.py; BASELINE configs 3-4).  Needs per-case targets (cfg.n_cases == 1, so that
    inertias and displacements belong to ONE load case) and `data.Fy_train`.
    PINN: r = K(I_pred) u_pred - f on the model's own (I, v, theta) outputs.
    TFD / FNN (I-only outputs): r = K(I_pred) u_rec - f with the displacement field recorded in the dataset
    (`data.v_train`, `data.theta_train`): zero when the predicted inertias reproduce the recorded response.  The
    records must keep the last node's values (SizingConfig.zero_last_node = False: MultiCore.py:222-223 zeroes them)."""
    weight: float
    x: torch.Tensor        # [N] node coordinates
    E: float
    fix: torch.Tensor      # [N] uint8
    wy: float


@dataclass
class DesignTerm:
    """Optional design-objective term (design_loss.py), given to `train_surrogate(..., physics=...)` in place of a
    `PhysicsTerm`: weight * mean over the batch of L(I_pred) / ref, the sizing objective of the predicted design under the sample's
    `cfg.n_cases` load cases (`data.Fy_cases_train`), differentiated through the solve.  `normalise`: ref is the objective of the
    sample's own label (computed once at setup), so the term is the mean optimality ratio; otherwise ref = 1.  `hp`: a
    `SizingConfig` or an `ops_sizing_params`; `aggregate`, `weights`, `alpha_deflection`, `deflection_limit` as in
    `optimize_designs`.  Every group of the data must share the geometry `x` and one support set `fix`.  GPU only."""
    weight: float
    x: torch.Tensor        # [N] node coordinates
    E: float
    fix: torch.Tensor      # [N] uint8
    wy: float
    hp: object
    aggregate: str = "sum"
    weights: Optional[Sequence[float]] = None
    alpha_deflection: float = 0.0
    deflection_limit: Optional[float] = None
    normalise: bool = True


def r2_score(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:
    """sklearn.metrics.r2_score on the raveled arrays (PINN:851)."""
    yt, yp = y_true.double().reshape(-1), y_pred.double().reshape(-1)
    ss_res = ((yt - yp) ** 2).sum()
    ss_tot = ((yt - yt.mean()) ** 2).sum()
    return float(1.0 - ss_res / ss_tot)


def _allreduce_mean(t: torch.Tensor, world: int, dp: Optional[bool] = None) -> torch.Tensor:
    if (world > 1) if dp is None else dp:
        dist.all_reduce(t)
        t /= world
    return t


def train_surrogate(kind: str, data: SurrogateData, cfg=None, device="cuda", *, autocast_dtype=torch.bfloat16, **kw) -> Dict[str, object]:
    """`_train_surrogate` (below: every argument is documented there).  With `autocast_dtype=torch.float16` -- the reference's own AMP mode,
    fp16 autocast + GradScaler (PINN:706, :759-768; TFD:690, :744-753) -- the run takes the framework's modules throughout (the hand-written
    launches are bf16): the module-level switches of the fused pieces are off for its duration."""
    if autocast_dtype != torch.float16:
        return _train_surrogate(kind, data, cfg, device, autocast_dtype=autocast_dtype, **kw)
    from . import surrogates as _s
    g = globals()
    saved = (_s._FUSED_TAILS, _s._FUSED_STENCIL, g["_FUSED_LOSS"], switches.get("fused_prep"), switches.get("fused_physics"))
    try:
        _s._FUSED_TAILS = _s._FUSED_STENCIL = False
        g["_FUSED_LOSS"] = False
        switches.set("fused_prep", 0); switches.set("fused_physics", 0)
        return _train_surrogate(kind, data, cfg, device, autocast_dtype=autocast_dtype, **kw)
    finally:
        _s._FUSED_TAILS, _s._FUSED_STENCIL, g["_FUSED_LOSS"] = saved[:3]
        switches.set("fused_prep", saved[3]); switches.set("fused_physics", saved[4])


class _PhysicsInputs:
    """The FE-residual term's device-side inputs -- loads, scalers, for the I-only models the recorded displacement fields -- and its two
    evaluations.  `g_idx`: the fused batch assembly's row output (None where the step gathers its batch some other way)."""

    def __init__(self, term: PhysicsTerm, kind: str, cfg, data: SurrogateData, device, fused: bool, g_idx, loss_acc):
        if cfg.n_cases != 1 or data.Fy_train is None:
            raise ValueError("the FE-residual term needs n_cases == 1 and data.Fy_train (per-case loads)")
        if kind != "pinn" and data.v_train is None:
            raise ValueError("the FE-residual term of an I-only model needs the recorded displacements (data.v_train)")
        self.term, self.pinn, self.nel, self.fused, self.g_idx, self.loss_acc = term, kind == "pinn", cfg.nelem, fused, g_idx, loss_acc
        self.Fy = data.Fy_train.to(device)
        self.sI = data.scalers_Y["I"]
        if self.pinn:                    # the model's own (v, theta) outputs: their scalers
            self.disp = (data.scalers_Y["deflections"], data.scalers_Y["rotations"])
        else:                            # (the fused term reads raw float64 rows)
            self.disp = (data.v_train.to(device=device, dtype=torch.float64).contiguous(),
                         data.theta_train.to(device=device, dtype=torch.float64).contiguous())
        self.x, self.fix = term.x.to(device=device, dtype=torch.float64), term.fix.to(device=device, dtype=torch.uint8)
        self.E = torch.tensor(float(term.E), dtype=torch.float64, device=device)      # device scalars: nothing crosses PCIe
        self.wy = torch.tensor(float(term.wy), dtype=torch.float64, device=device)    # inside a captured step

    def inputs(self, rows, out=None):
        """Per-batch loads (and, for the I-only models, recorded displacement fields); `out`: the graph's static buffers.
        Fused term (csrc/beam_residual.hip ops_physics_loss_*): only the ROW INDICES travel -- the launches gather by them."""
        if self.fused:
            if self.g_idx is not None:   # the front-end launch leaves the step's rows in g_idx
                return (self.g_idx[:rows.numel()],)
            if out is None:
                return (rows,)
            out[0].copy_(rows)
            return out
        srcs = (self.Fy,) if self.pinn else (self.Fy,) + self.disp
        if out is None:
            return tuple(t[rows] for t in srcs)
        for t, o in zip(srcs, out):
            torch.index_select(t, 0, rows, out=o)
        return out

    def loss(self, preds, pin):
        nel, term = self.nel, self.term
        if self.fused:           # three launches; the value is already weighted and enters the total with weight one
            from .physics import fused_residual_term
            return fused_residual_term(preds, nel, self.sI, self.disp, pin[0], self.Fy, self.x, float(term.E), self.fix, float(term.wy),
                                       term.weight, self.loss_acc)
        from .physics import fe_residual_loss
        preds = preds.float()
        I_p = self.sI.inverse_transform(preds[:, :nel]).clamp_min(1e-8)
        if self.pinn:
            v_p = self.disp[0].inverse_transform(preds[:, nel:2 * nel + 1])
            t_p = self.disp[1].inverse_transform(preds[:, 2 * nel + 1:])
        else:
            v_p, t_p = pin[1], pin[2]
        return term.weight * fe_residual_loss(I_p, v_p, t_p, self.x, self.E, self.fix, pin[0], self.wy).float()


class _DesignInputs:
    """The design-objective term's device-side inputs -- the groups' load cases, the labels' own objective, the checked argument tuple
    -- behind the interface of `_PhysicsInputs`.  Always the fused form: only the ROW INDICES travel, the launches gather by them."""

    fused = True

    def __init__(self, term: DesignTerm, kind: str, cfg, data: SurrogateData, device, g_idx, loss_acc):
        from . import design_loss
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the design-objective term needs a GPU: openpystruct_amd has no CPU fallback")
        if data.Fy_cases_train is None:
            raise ValueError("the design-objective term needs data.Fy_cases_train (records with force_nodes and force_values)")
        self.term, self.nel, self.g_idx, self.loss_acc = term, cfg.nelem, g_idx, loss_acc
        Fy = data.Fy_cases_train.to(device=device, dtype=torch.float64).contiguous()
        if Fy.dim() != 3 or Fy.shape[1] != cfg.n_cases or Fy.shape[2] != cfg.nelem + 1:
            raise ValueError(f"data.Fy_cases_train must be [G, {cfg.n_cases}, {cfg.nelem + 1}], got {tuple(Fy.shape)}")
        for split, X in (("training", data.X_train), ("validation", data.X_val)):
            _check_shared_bridge(term, data, X, cfg.n_cases, split)
        sI = data.scalers_Y["I"]
        # (the scaler's two rows on the device, in the launches' dtype: nothing is copied or cast inside a captured step)
        sI = types.SimpleNamespace(scale_=sI.scale_.to(device=device, dtype=torch.float32).contiguous(),
                                   mean_=sI.mean_.to(device=device, dtype=torch.float32).contiguous(),
                                   inverse_transform=lambda t, s=sI: s.inverse_transform(t))
        kw = dict(aggregate=term.aggregate, weights=term.weights, alpha_deflection=term.alpha_deflection,
                  deflection_limit=term.deflection_limit)
        ref = None
        if term.normalise:       # the optimiser's own objective of every training label, un-standardised
            I_lab = sI.inverse_transform(data.Y_train[:, :cfg.nelem].to(device).float()).clamp_min(design_loss.I_MIN).double()
            ref = design_loss.design_objective(I_lab, term.x, term.E, term.fix, Fy, term.wy, term.hp, n_load_cases=cfg.n_cases, **kw).value
            if not bool((torch.isfinite(ref) & (ref > 0)).all()):
                raise ValueError("the objective of a training label is not finite and positive: the term cannot be normalised by it")
            ref = ref.contiguous()
        self.ref = ref
        self.spec = design_loss._term_spec(device, cfg.nelem, sI, None, Fy, term.x, term.E, term.fix, term.wy, term.hp, term.weight,
                                           ref=ref, acc=loss_acc, **kw)
        self.term_sum = torch.zeros((), dtype=torch.float32, device=device)      # the run's total of the term's step values

    def inputs(self, rows, out=None):
        if self.g_idx is not None:       # the front-end launch leaves the step's rows in g_idx
            return (self.g_idx[:rows.numel()],)
        if out is None:
            return (rows,)
        out[0].copy_(rows)
        return out

    def loss(self, preds, pin):
        from . import design_loss
        spec = self.spec[:2] + (pin[0],) + self.spec[3:]
        value = design_loss._DesignObjectiveTerm.apply(preds, spec)
        self.term_sum.add_(value.detach())
        return value


def _check_shared_bridge(term: "DesignTerm", data: SurrogateData, X: torch.Tensor, n_cases: int, split: str) -> None:
    """ValueError unless every case of every group of X has the geometry `term.x` and ONE set of roller positions: the term's
    launches read one shared x [N] and fix [N]."""
    ml = data.max_lengths
    X3 = X.reshape(X.shape[0], n_cases, -1)
    if X3.shape[0] == 0:
        return
    o = ml["roller_x"] + ml["force_x"] + ml["force_values"]
    rollers, nodes = X3[..., :ml["roller_x"]], X3[..., o:o + ml["node_positions"]]
    if bool((rollers != rollers[:1, :1]).any()):
        raise ValueError(f"the design-objective term needs ONE support set: the roller positions differ between the {split} groups")
    if bool((nodes != nodes[:1, :1]).any()):
        raise ValueError(f"the design-objective term needs ONE geometry: the node positions differ between the {split} groups")
    x = torch.as_tensor(term.x, dtype=torch.float64).reshape(-1).cpu()
    got = data.scalers_inputs["node_positions"].inverse_transform(nodes[0, 0].float().cpu()).double()
    if got.numel() != x.numel() or not torch.allclose(got, x, rtol=1e-5, atol=1e-5 * float(x.abs().max())):
        raise ValueError(f"the design-objective term's x is not the geometry of the {split} records")


class _Step:
    """One training step's state and its pieces: [fwd_bwd] (segment A), the gradient all-reduce, [apply_update] (segment B).
    `_setup_step` sets every attribute; one that belongs to a path the run does not take is None (or False)."""

    def kl_term(self):
        from . import bayes as _bayes
        kl = _bayes.bayesian_kl(self.model)
        return self.cfg.bnn_kl_scale * (kl.detach() if self.bayes_hip is not None else kl)

    def fwd_bwd(self, Xb, Yb, noise_t, pin=None, prenoised=False):
        """Segment A: local gradients of the mean batch loss into `flat`.  `prenoised`: Xb already is the gathered, noisy
        (and, under autocast, bfloat16) batch written by the batch-assembly launch -- one launch outside the graph instead of six nodes."""
        cfg, crit, loss_acc, flat = self.cfg, self.crit, self.loss_acc, self.flat
        if self.engine is not None:      # batch and targets sit in the engine's buffers (engine.gather); every gradient is assigned
            return self.engine.fwd_bwd(int(Yb.shape[0]))
        Xn = Xb if prenoised else Xb + torch.randn_like(Xb) * noise_t   # PINN:756
        if not (self.on_gpu and self.opt.zero_grads):
            flat.zero_()                                                 # optimizer.zero_grad() (GPU: the update launch zeroes `flat` behind itself)
        alpha0 = cfg.initial_alpha if self.alpha_term else None
        with torch.autocast(device_type=self.device.type, dtype=self.autocast_dtype, enabled=self.use_ac):
            head_loss = None
            if self.head_loss_ok:
                # Transformer-Diffusion fast path: the loss on the head's output tile, finished by the head's backward launch
                self.tfd.arm_head_loss(self.model, Yb, crit, alpha0, loss_acc)
                preds = self.model(Xn)
                head_loss = self.tfd.take_head_loss(self.model)
                if head_loss is None and self.fuse_gather:
                    # (with the batch assembled by the front-end launch the static target buffer `Yb` is never filled: the framework-side
                    #  loss below would be evaluated against stale targets -- fail loudly instead)
                    raise RuntimeError("the head's loss launch did not run although the front-end launch assembles the batch itself "
                                       "(criterion / shape mismatch in tfd_fused.arm_head_loss)")
            else:
                preds = self.model(Xn)
            if head_loss is not None:
                loss = head_loss
            elif self.on_gpu and _FUSED_LOSS:       # value + d/d preds in one HIP pass instead of ~80 framework kernel nodes
                loss = fused_loss(crit, preds, Yb, alpha0=alpha0, unit_grad=True, acc=loss_acc)
            else:
                loss = crit(preds.float(), Yb)
                if self.alpha_term:
                    loss = loss + (cfg.initial_alpha - crit.alpha) ** 2   # TFD:743 / FNN (constant 0: alpha never trains)
            if self.bayes_kl:
                kl = self.kl_term()
                loss = loss + kl
                if loss_acc is not None:
                    loss_acc.add_(kl.detach())
        if self.physics is not None:
            term = self.physics.loss(preds, pin)
            # (with the running sum both launches have already added their values up: the step's scalar only roots the backward pass,
            #  so the two terms are tied without an addition node -- its value is then the data loss alone)
            loss = _TieTerms.apply(loss, term) if (loss_acc is not None and self.physics.fused) else loss + term
        # split-row weight gradients: one grouped launch after backward; the shadow-linear weight / bias gradients: one multi-tensor
        # cast-and-copy into `flat`
        with grouped_wgrads(self.device, self.g_stash, self.g_dst, enabled=bool(self.g_stash and _GROUP_WGRAD)):
            # the root gradient is a persistent ones tensor: no ones_like() fill node per step.  (r03 kept the implicit form because the
            # explicit one "produced" NaNs in bias gradients of framework-path runs; the NaNs were the HIP runtime's captured-memset
            # defect under the framework's own bias-gradient reductions -- runtime.py item 2 -- and the root gradient only moved the
            # memory layout that decided which garbage their semaphores saw)
            if self.fp16_scaler is not None:     # scaler.scale(loss).backward() (PINN:761): the root gradient IS the scale
                loss.backward(gradient=torch.full((), self.fp16_scaler["scale"], dtype=loss.dtype, device=self.device))
            elif _EXPLICIT_ROOT:
                loss.backward(gradient=_root_ones(self.device))
            else:
                loss.backward()
        return loss.detach()

    def apply_update(self):
        """Segment B: average over ranks, clip, Adam."""
        opt, flat, world = self.opt, self.flat, self.world
        if self.fp16_scaler is not None:
            # scaler.unscale_ + clip + scaler.step + scaler.update (PINN:763-768): a non-finite gradient skips the step and halves the scale,
            # 2 000 clean steps in a row double it; the unscaling rides in the update launch's gradient scale
            sc = self.fp16_scaler
            sc["steps"] += 1
            if bool(torch.isfinite(flat).all()):
                opt.step(grad_scale=1.0 / (world * sc["scale"]))
                sc["good"] += 1
                if sc["good"] >= 2000:
                    sc["scale"] *= 2.0; sc["good"] = 0
            else:
                flat.zero_()
                sc["scale"] *= 0.5; sc["good"] = 0; sc["skipped"] += 1
            return
        if self.on_gpu:
            opt.step(grad_scale=1.0 / world)                             # average, clip (PINN:766), Adam
            return
        if self.dp:
            flat.div_(world)
        torch.nn.utils.clip_grad_norm_(self.params, 1.0)                 # PINN:766
        opt.step()

    def allreduce_grads(self):
        """ONE flat all-reduce of every parameter gradient (2.38 MB PINN / 1.44 MB TFD)."""
        if _DP_ASYNC:
            dist.all_reduce(self.flat, async_op=True).wait()             # GPU: stream ordering only, the host does not block
        else:
            dist.all_reduce(self.flat)

    def train_step(self, Xb, Yb, noise_t, rows=None):
        """The eager step (no graph, or a batch size no graph was captured for)."""
        if self.engine is not None:
            self.engine.gather(self.Xtr, self.Ytr, rows, noise_t, self.engine_seed)
        loss = self.fwd_bwd(Xb, Yb, noise_t, self.physics.inputs(rows) if self.physics is not None else None)
        if self.dp:
            self.allreduce_grads()                                       # the step's only collective (RCCL over xGMI)
        self.apply_update()
        return loss


def _setup_step(kind, data, cfg, device, autocast_dtype, sync_bn, log, seed, use_graph, physics, init_fn) -> _Step:
    """Model, criterion, flat gradient buffer, optimiser and whichever hand-written pieces the run is eligible for; the data set on the device."""
    st = _Step()
    st.kind, st.seed = kind, seed
    st.cfg = cfg = cfg or {"pinn": PinnConfig, "tfd": TfdConfig, "fnn": FnnConfig, "gnn": GnnConfig, "fno": FnoConfig, "btfd": BtfdConfig,
                           "btfdm": BtfdmConfig}[kind]()
    st.alpha_term = kind in ("tfd", "fnn", "fno", "btfd", "btfdm")    # (initial_alpha - alpha)^2 in the training loss (TFD:743, FNO:615, BTFD:730)
    st.bayes_kl = bayes_kl = kind in ("btfd", "btfdm") and cfg.kl == "gaussian"
    if kind in ("btfd", "btfdm") and cfg.kl not in ("none", "gaussian"):
        raise ValueError(f"kl must be 'none' or 'gaussian', not {cfg.kl!r}")
    if kind == "fno":
        autocast_dtype = None                           # FNO:613 runs with autocast disabled
    st.autocast_dtype = autocast_dtype
    st.device = device = torch.device(device)
    st.world = world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    st.rank = rank = dist.get_rank() if world > 1 else 0
    # the data-parallel branch: more than one rank -- or, with OPS_AMD_FORCE_DP=1, a process group of ONE rank (r05: the RCCL path -- flat
    # all-reduce between graph A and graph B, its async form, the one-graph capture of the collective, dp_segments -- executed on the
    # single GPU a test box has; a one-rank all-reduce is the identity and 1 / world = 1, so losses equal the plain run bit for bit)
    st.dp = dp = world > 1 or (_FORCE_DP and dist.is_available() and dist.is_initialized())
    st.engine_seed = (seed * 7919 + 13 + rank) & 0x7FFFFFFFFFFFFFFF       # the batch-assembly launches' noise stream, whichever launch it is
    torch.manual_seed(seed)            # identical initial weights on every rank
    model, crit = build_model_and_loss(kind, cfg, data, device)
    st.tfd = tfd_fused = None
    if kind == "tfd" and device.type == "cuda":
        from . import tfd_fused          # (here and not at the top: a CPU-only process never needs it)
        st.tfd = tfd_fused
    if init_fn is not None:
        init_fn(model)
    st.bayes_hip = None
    if kind in ("btfd", "btfdm") and device.type == "cuda":
        # the four Bayesian layers: one sampling launch per forward, one fold launch per backward (bayes.py, csrc/bayes_mlp.hip); with
        # the KL term on, the fold adds its gradient and the loss its (detached) value
        from . import bayes as _bayes
        st.bayes_hip = _bayes.BayesSampler(model, seed=seed * 7919 + 307 + rank, kl_scale=cfg.bnn_kl_scale if bayes_kl else 0.0)
        model.bayes_sampler = st.bayes_hip
    if sync_bn and dp:
        model = nn.SyncBatchNorm.convert_sync_batchnorm(model)
    st.model, st.crit = model, crit
    # one flat gradient buffer; every .grad is a view into it (autograd accumulates in place)
    st.params = params = [q for q in model.parameters()]
    st.flat = flat = flat_grads(params, device)
    st.g_stash, st.g_dst, st.patched = [], [], []
    st.fast_encoder = None
    st.shared_counter = False
    if hasattr(model, "direct_param_grads"):   # fused tails (csrc/fused_bn.hip) write BatchNorm parameter gradients into `flat` themselves
        model.direct_param_grads = device.type == "cuda"
    torch.manual_seed(seed + 1 + rank)  # different noise / shuffles per rank
    st.on_gpu = on_gpu = device.type == "cuda"
    # the reference's AMP mode: GradScaler(init_scale 65536, growth 2, backoff 0.5, growth interval 2000) -- torch.cuda.amp.GradScaler's defaults
    st.fp16_scaler = {"scale": 65536.0, "good": 0, "skipped": 0, "steps": 0} if (on_gpu and autocast_dtype == torch.float16) else None
    if st.fp16_scaler is not None:
        use_graph = False                # the scale and the skip decision are per-step host state, like `scaler.step` / `scaler.update`
    if use_graph is None:
        use_graph = on_gpu and os.environ.get("OPS_AMD_GRAPH", "1") == "1"    # the step is launch-bound (~150 tiny kernels): replay it as HIP graphs
    # under graph replay the learning rate must live in a device tensor, or the scheduler's updates would
    # never reach the captured optimiser step
    st.prep_counter = torch.zeros(2, dtype=torch.int64, device=device) if on_gpu else None     # batch assembly: [calls, workgroups done]
    if on_gpu:      # clip + Adam over the flat buffers in two HIP launches; loss.alpha NOT included (PINN:696)
        st.opt = opt = FlatClipAdam(params, flat, cfg.learning_rate, weight_decay=cfg.weight_decay, max_norm=1.0, decoupled=kind == "gnn")
        st.sched = None
        if _SHADOW_LINEAR and autocast_dtype == torch.bfloat16:
            st.g_stash, st.g_dst, st.patched = enable_shadow_linears(model, opt, params, flat)
            # csrc/seq_block.hip: attention, dropout + add + LayerNorm, ReLU + dropout, diffusion front end
            if kind == "tfd" and tfd_fused.patch_model(model, seed=seed * 7919 + 211 + rank, direct_param_grads=True):
                st.fast_encoder = model
                opt.repack = getattr(model.transformer_encoder, "_ops_tile_entries", None)    # the Adam launch refreshes the layer kernels' weight tiles
                if switches.get("fused_prep") == "1":
                    # the batch-assembly launch advances its call counter once per step: the dropout / noise streams read that one
                    tfd_fused.share_step_counter(model.transformer_encoder, st.prep_counter)
                    st.shared_counter = True
    else:
        st.opt = opt = (torch.optim.AdamW if kind == "gnn" else torch.optim.Adam)(model.parameters(), lr=cfg.learning_rate,   # GNN:394
                                                                                   weight_decay=cfg.weight_decay)
        st.sched = ExponentialLR(opt, gamma=cfg.gamma)
    # PINN: forward + loss + backward as 13 hand-written launches without autograd (pinn_fused.py / csrc/mlp_block.hip);
    # the module keeps owning parameters and buffers, evaluation keeps running it
    st.engine = engine = None
    if on_gpu and kind == "pinn" and autocast_dtype == torch.bfloat16 and physics is None and not (sync_bn and dp):
        from . import pinn_fused
        if pinn_fused.eligible(model, crit, cfg.batch_size):
            st.engine = engine = pinn_fused.PinnFusedStep(model, crit, seed=seed * 7919 + 101 + rank)
            opt.repack = engine._repack      # the Adam launch refreshes the engine's bf16 weight copies
            if not dp and switches.get("pinn_norm_fold") == "1":
                # one rank: the gradients are final when the weight-gradient launch ends, so that launch leaves the clip norm's partial
                # sums and the optimiser skips its norm launch (a node and ~4.5 us per step; data parallel: the norm is the all-reduced one)
                opt.norm_ready_parts = engine.enable_norm(flat, opt.ws, opt.step_count, opt.betas)
            if not dp and switches.get("pinn_repack_in_gather") == "1":
                # one rank: the weight copies of step n ride on the batch-assembly launch of step n + 1 (adjacent launches that depend on
                # nothing of each other: one node and ~5 us less per step); the optimiser call no longer rebuilds them
                opt.repack = None
                engine.repack_in_gather(opt.p)
    if use_graph and on_gpu and engine is None and st.fast_encoder is None:
        # a step the FRAMEWORK differentiates (comparator paths, the sibling surrogates): its multi-block reductions are only right under
        # graph replay when captured memset nodes are (runtime.py item 2); the hand-written paths above contain none
        from . import runtime
        if not runtime.graph_memsets_replay_correctly(device):
            use_graph = False
            if log:
                log(f"captured hipMemsetAsync nodes replay wrong values in this process ({runtime.PACKET_CAPTURE_ENV}=0 came after its "
                    "first HIP call?): the framework-differentiated step runs eagerly")
    st.use_graph = use_graph
    st.Xtr, st.Ytr, st.Xva, st.Yva = (t.to(device) for t in (data.X_train, data.Y_train, data.X_val, data.Y_val))
    Xtr, Ytr = st.Xtr, st.Ytr
    nb_tr = max(1, (Xtr.shape[0] + cfg.batch_size - 1) // cfg.batch_size)
    if dp:   # every rank must run the same number of steps (collectives inside backward)
        # a one-row tail batch makes train-mode BatchNorm raise (as in the reference's single process); on one rank of a
        # data-parallel job that exception would leave the other ranks waiting in the step's all-reduce: drop such a tail
        if Xtr.shape[0] % cfg.batch_size == 1 and nb_tr > 1 and any(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in model.modules()):
            nb_tr -= 1
        t = torch.tensor([nb_tr], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        nb_tr = int(t.item())
    st.nb_tr = nb_tr
    st.use_ac = device.type == "cuda" and autocast_dtype is not None
    # Transformer-Diffusion fast path, r04: the front-end launch assembles its own batch (rows order[cursor ..] of the training set + the
    # input noise) and the head's loss reads its targets through those rows: no batch-assembly launch per step.  The epoch's permutation
    # lives in `g_order`, `g_cursor` is advanced by the launch itself (reset per epoch).
    st.fuse_gather = False
    st.g_order = st.g_cursor = st.g_noise = st.g_idx = None
    design = isinstance(physics, DesignTerm)
    if design and not on_gpu:
        raise RuntimeError("the design-objective term needs a GPU: openpystruct_amd has no CPU fallback")
    # A/B switch: 0 = physics.fe_residual_loss from framework ops (the design-objective term has the fused form only)
    fused_phys = on_gpu and (design or switches.get("fused_physics") == "1")
    # the loss launch adds every step's value to the epoch's running sum itself (zeroed per epoch): no add node per step
    # (with the fused physics term both launches add into the same running sum: the epoch's total of data loss + term)
    st.loss_acc = loss_acc = torch.zeros((), dtype=torch.float32, device=device) if (
        on_gpu and _FUSED_LOSS and engine is None and (physics is None or fused_phys) and switches.get("loss_acc") == "1") else None
    # the loss on the head's tile: its value exists once the head's backward launch has run, so a second term can only be tied to it
    # (not added) -- which needs the running sum to carry the step values
    st.head_loss_ok = st.fast_encoder is not None and _FUSED_LOSS and (physics is None or (fused_phys and loss_acc is not None))
    if (st.head_loss_ok and st.shared_counter and Xtr.dtype == torch.float32 and Xtr.dim() == 3
            and Xtr.is_contiguous() and Ytr.dtype == torch.float32 and Ytr.is_contiguous() and Ytr.dim() == 2
            and tfd_fused.gather_fusable(model, device, int(Xtr.shape[2]))):
        st.fuse_gather = True
        st.g_order = torch.arange(max(int(Xtr.shape[0]), cfg.batch_size), device=device) % int(Xtr.shape[0])
        st.g_cursor = torch.zeros((), dtype=torch.int64, device=device)
        st.g_noise = torch.zeros((), device=device)
        st.g_idx = torch.zeros(max(cfg.batch_size, 1), dtype=torch.int64, device=device)
        tfd_fused.arm_gather(model, Xtr, Ytr, st.g_order, st.g_cursor, st.g_idx, st.g_noise, st.engine_seed)
    st.physics = None
    if physics is not None:
        st.physics = (_DesignInputs(physics, kind, cfg, data, device, st.g_idx, loss_acc) if design else
                      _PhysicsInputs(physics, kind, cfg, data, device, fused_phys, st.g_idx, loss_acc))
    if on_gpu and engine is None and switches.get("adam_zero") == "1":
        opt.zero_grads = True            # `flat` starts zeroed (allocation) and every update leaves it zeroed
    # batch assembly in one launch (csrc/input_prep.hip): gather + noise + cast straight into the graph's input buffer
    st.fused_prep = on_gpu and switches.get("fused_prep") == "1"
    # bf16 batches only where the first module is a (shadow) Linear, which casts its operand to bf16 anyway
    st.prep_bf16 = bool(on_gpu and st.use_ac and autocast_dtype == torch.bfloat16 and st.patched and kind in ("pinn", "fnn", "gnn"))
    st.y_in_prep = bool(on_gpu and Ytr.dtype == torch.float32 and Ytr.is_contiguous() and switches.get("prep_targets") == "1")      # the targets travel in the same launch
    return st


class _CapturedStep:
    """The training step as HIP graphs over static buffers, and what feeds them: `graph` (the whole step; with `graph_b`: segment A, the
    eager all-reduce, segment B), `graph_t` (the epoch's last, partial batch).  All None where the step runs eagerly."""

    def __init__(self, st: _Step, log):
        self.st = st
        self.side = self.graph = self.graph_b = self.graph_t = None
        self.one_graph = False           # the data-parallel step with its collective inside `graph`
        self.sX = self.sY = self.sP = self.s_noise = self.s_loss = self.sXt = self.sYt = self.s_loss_t = None
        device, engine, Xtr, Ytr, bs = st.device, st.engine, st.Xtr, st.Ytr, st.cfg.batch_size
        if not (st.use_graph and Xtr.shape[0] >= bs):
            return
        # static buffers + a few eager warm-up steps on a side stream, then capture one full-batch step:
        # not dp -> one graph; dp -> one graph with the collective in it, or [fwd_bwd] graph, eager all-reduce, [apply_update] graph
        from .runtime import capture_graph, try_capture
        rewind = st.g_cursor.zero_ if st.fuse_gather else None
        self.sX, self.sY = torch.zeros_like(Xtr[:bs], dtype=torch.bfloat16 if (st.fused_prep and st.prep_bf16) else Xtr.dtype), torch.zeros_like(Ytr[:bs])
        self.s_noise = torch.zeros((), device=device)
        if st.physics is not None:               # static per-batch physics inputs, gathered before every replay
            self.sP = st.physics.inputs(torch.arange(bs, device=device))
            if not st.fuse_gather:       # (fused batch assembly: the rows are the front-end launch's own index output)
                self.sP = tuple(torch.zeros_like(t[:bs]) for t in self.sP)
        snap = (copy.deepcopy(st.model.state_dict()), copy.deepcopy(st.opt.state_dict()))
        self.side = side = torch.cuda.Stream(device=device)

        def fwd(tail=False):
            X, Y, P = (self.sXt, self.sYt, None) if tail else (self.sX, self.sY, self.sP)
            return st.fwd_bwd(X, Y, self.s_noise, P, prenoised=st.fused_prep)

        def step(tail=False, collective=False):
            loss = fwd(tail)
            if collective:
                dist.all_reduce(st.flat)
            st.apply_update()
            return loss

        def graphs():                    # the whole step; data parallel: segment A, and segment B behind the eager collective
            ga, loss = capture_graph(side, device, fwd if st.dp else step)
            return ga, loss, (capture_graph(side, device, st.apply_update)[0] if st.dp else None)

        def tail_graph(nt):
            self.sXt, self.sYt = (None if engine is not None else torch.zeros_like(self.sX[:nt])), torch.zeros_like(self.sY[:nt])
            if engine is not None:       # the engine's own buffers are the graph's inputs: Yb only carries the row count
                engine.gather(Xtr, Ytr, torch.arange(nt, device=device), self.s_noise, st.engine_seed)
            else:
                self.sXt.copy_(self.sX[:nt]); self.sYt.copy_(self.sY[:nt])
            return capture_graph(side, device, lambda: step(tail=True), 2, rewind)

        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):    # (capture_graph, called on the side stream, adds no waits of its own)
            self.sX.copy_(Xtr[:bs]); self.sY.copy_(Ytr[:bs])
            if self.sP is not None:
                st.physics.inputs(torch.arange(bs, device=device), out=self.sP)
            if engine is not None:
                engine.gather(Xtr, Ytr, torch.arange(bs, device=device), self.s_noise, st.engine_seed)
            # (fused batch assembly: every launch advances g_cursor by its batch; warm-up and capture passes each start at row 0 so that no
            #  pass reads g_order past its end -- the kernel wraps as well, ops_tfd_front_args.n_order; the epoch loop zeroes it again)
            for _ in range(3):
                if rewind:
                    rewind()
                step()                           # warm-up only: no collective needed for capture-readiness
            if rewind:
                rewind()
            side.synchronize()
            got = None
            if st.dp and _DP_ONE_GRAPH and dist.get_backend() == "nccl":
                # the collective inside the capture: one replay per step, no host work between the segments
                got = try_capture("the step with its gradient all-reduce", "two graphs around an eager collective", log, device,
                                  lambda: capture_graph(side, device, lambda: step(collective=True)) + (None,))
                self.one_graph = got is not None
            if got is None:                  # on failure: the same arithmetic eagerly; the step is then launch-bound
                got = try_capture("the training step", "training eagerly", log, device, graphs)
            if got is not None:
                self.graph, self.s_loss, self.graph_b = got
            # the epoch's LAST (partial) batch as a graph of its own: an eager step is ~25 launches' worth of host time (0.3-0.4 ms of a
            # 5 ms TFD epoch), and eager model passes between replays are what the flaky-NaN hunt of r03 kept running into
            nt = int(Xtr.shape[0]) % bs
            if (self.graph is not None and not st.dp and self.sP is None and nt >= 2 and st.nb_tr == Xtr.shape[0] // bs + 1
                    and switches.get("tail_graph") == "1"):
                got = try_capture("the tail batch", "that step runs eagerly", log, device, lambda: tail_graph(nt))
                if got is not None:
                    self.graph_t, self.s_loss_t = got
        torch.cuda.current_stream(device).wait_stream(side)
        st.model.load_state_dict(snap[0]); st.opt.load_state_dict(snap[1])     # the warm-up steps never happened
        if isinstance(st.physics, _DesignInputs):
            st.physics.term_sum.zero_()
        st.opt.refresh_shadow()
        if engine is not None:
            engine.repack_now()
        if st.fast_encoder is not None:
            st.tfd.refresh_layer_tiles(st.fast_encoder.transformer_encoder)

    def feed(self, idx, sX, sY):
        """Rows `idx` of the training set into the static buffers of the full-batch graph (sX, sY) or of the tail graph (sXt, sYt)."""
        st, Xtr, Ytr = self.st, self.st.Xtr, self.st.Ytr
        if st.fuse_gather:               # the captured step's first launch assembles the batch itself
            return
        if st.engine is not None:        # batch AND targets straight into the engine's layouts (no physics term with the engine)
            st.engine.gather(Xtr, Ytr, idx, self.s_noise, st.engine_seed)
            return
        with_y = False
        if st.fused_prep:                # gather + noise (+ bf16 cast) and, where they are float32, the targets in one launch
            with_y = st.y_in_prep and sY.dtype == torch.float32 and sY.is_contiguous()
            with torch.cuda.device(st.device):
                rc = _cabi.load().ops_gather_rows_noise_targets_f32(
                    int(idx.numel()), int(Xtr[0].numel()), Xtr.data_ptr(), idx.data_ptr(), self.s_noise.data_ptr(), st.engine_seed,
                    st.prep_counter.data_ptr(), sX.data_ptr(), int(sX.dtype == torch.bfloat16), Ytr.data_ptr() if with_y else None,
                    int(Ytr[0].numel()) if with_y else 0, sY.data_ptr() if with_y else None, torch.cuda.current_stream(st.device).cuda_stream)
            _cabi.check(rc, "ops_gather_rows_noise_targets_f32")
        else:
            torch.index_select(Xtr, 0, idx, out=sX)                      # gather straight into the graph's input buffers
        if not with_y:
            torch.index_select(Ytr, 0, idx, out=sY)
        if self.sP is not None:          # (full batches only: no tail graph is captured with a physics term)
            st.physics.inputs(idx, out=self.sP)


class _Validation:
    """The epoch's validation pass, `run()`, in the one of four modes the run is eligible for: the engine's evaluation slots in one graph;
    the engine's pass per batch (graphs keyed by row count, eager otherwise); one forward over the whole set (`val_whole`), captured or
    eager; the module per batch (graphs keyed by row count, eager otherwise).  The constructor captures what its mode replays."""

    def __init__(self, st: _Step, cap: _CapturedStep, log):
        self.st, cfg, engine, Xva, Yva = st, st.cfg, st.engine, st.Xva, st.Yva
        self.nb_va = max(1, (Xva.shape[0] + cfg.batch_size - 1) // cfg.batch_size)
        # Transformer-Diffusion fast path: the validation pass as ONE forward over all validation rows (chunks of <= `chunk` rows, whole
        # reference batches each) + the loss per reference batch on row slices of its output, every value added to `acc` by the loss launch
        # itself.  The reference's value -- the mean over its batches of the batch losses (TFD:760-775) -- is kept; a step-sized forward
        # fills 1/18 of the chip, so 20 of them in a row cost ~8x what one 20-fold forward does.  (Rows are independent in evaluation mode;
        # the diffusion draws of the pass come from one call of the stream instead of one per batch.)
        self.val_whole = bool(st.on_gpu and st.fast_encoder is not None and _FUSED_LOSS and switches.get("val_whole") == "1")
        self.chunk = cfg.batch_size * max(1, 4096 // max(cfg.batch_size, 1))
        # PINN: validation through the engine's evaluation pass (running statistics, no dropout) when the validation set has its layout
        self.engine_eval = bool(engine is not None and switches.get("pinn_engine_eval") == "1" and Xva.dtype == torch.float32
                                and Xva.is_contiguous() and Yva.dtype == torch.float32 and Yva.is_contiguous() and Xva.dim() == 2
                                and cfg.batch_size <= _cabi.MLP_MAX_ROWS)
        self.slot_graph = self.vgraph_all = self.val_rows = self.v_acc = None
        self.ev_graphs, self.vgraphs = {}, {}    # row count -> (graph, static row indices) of the engine / (graph, static batch, targets) of the module
        if cap.graph is None:
            return
        # the pass as graphs too (evaluation mode, loss accumulated on the device): one for the full batches, one for the last partial one
        from .runtime import capture_graph, try_capture
        side, device, bs = cap.side, st.device, cfg.batch_size
        nvt = int(Xva.shape[0]) % bs
        if self.engine_eval and switches.get("pinn_eval_slots") == "1":
            # PINN: the whole validation set per launch sequence -- every batch in an evaluation slot (pinn_fused.make_eval_slots:
            # gathered once, the rows never change), the engine's 7 evaluation launches run all slots side by side (grid.y): 7 nodes
            # per epoch instead of 14 batches x 8 launches of ~6 us
            def slots():
                engine.make_eval_slots(Xva, Yva, bs)
                return capture_graph(side, device, engine.evaluate_slots, 1)
            got = try_capture("the slotted evaluation pass", "one batch after the other", log, device, slots)
            self.slot_graph = got[0] if got is not None else None
        if self.engine_eval and self.slot_graph is None:
            # PINN: the engine's own evaluation pass (forward stages on the running statistics + loss, 8 launches per batch) instead of
            # the module's ~30-node forward; gather + evaluate captured per batch size, the row indices in a static buffer
            self.val_rows = torch.arange(Xva.shape[0], device=device)
            for n in sorted({bs if Xva.shape[0] >= bs else 0, nvt} - {0}):
                vi = self.val_rows[:n].clone()
                got = try_capture("the engine's evaluation pass", "those batches run eagerly", log, device,
                                  lambda: capture_graph(side, device, lambda: (engine.gather(Xva, Yva, vi, None, 0), engine.evaluate(n)), 1))
                if got is not None:
                    self.ev_graphs[n] = (got[0], vi)
        elif Xva.shape[0] >= bs or nvt >= 1:
            # the module's pass.  (Also captured next to a slot graph, where run() never replays it: inherited, and dropping those set-up
            # launches is a change of its own.)
            self.v_acc = v_acc = torch.zeros((), device=device)
            st.model.eval()

            def per_batch(rows):
                bx, by = torch.zeros_like(Xva[:rows]), torch.zeros_like(Yva[:rows])
                bx.copy_(Xva[:rows]); by.copy_(Yva[:rows])
                graph, _ = capture_graph(side, device, lambda: v_acc.add_(self._batch(bx, by)), 2, warm=lambda: self._batch(bx, by))
                return graph, bx, by

            def graphs():
                if self.val_whole:
                    self.vgraph_all = capture_graph(side, device, lambda: self._whole(v_acc), 2)[0]
                elif Xva.shape[0] >= bs:
                    self.vgraphs[bs] = per_batch(bs)
                if not self.val_whole and nvt >= 1 and not st.dp and switches.get("tail_graph") == "1":
                    self.vgraphs[nvt] = per_batch(nvt)
                return True
            if try_capture("the validation pass", "evaluating eagerly", log, device, graphs) is None:
                self.vgraph_all = None
                self.vgraphs.clear()
            v_acc.zero_()
            st.model.train()

    def _batch(self, Xb, Yb):
        st = self.st
        with torch.no_grad(), torch.autocast(device_type=st.device.type, dtype=st.autocast_dtype, enabled=st.use_ac):
            preds = st.model(Xb)
            if st.on_gpu and _FUSED_LOSS:
                v = fused_loss(st.crit, preds, Yb)
            else:
                v = st.crit(preds.float(), Yb)
            return v + st.kl_term() if st.bayes_kl else v                 # BTFD:772

    def _whole(self, acc):
        st, Xva, Yva, bs = self.st, self.st.Xva, self.st.Yva, self.st.cfg.batch_size
        nva = int(Xva.shape[0])
        with torch.no_grad(), torch.autocast(device_type=st.device.type, dtype=st.autocast_dtype, enabled=st.use_ac):
            for c0 in range(0, nva, self.chunk):
                preds = st.model(Xva[c0:c0 + self.chunk])
                for b0 in range(c0, min(c0 + self.chunk, nva), bs):
                    b1 = min(b0 + bs, nva)
                    fused_loss(st.crit, preds[b0 - c0:b1 - c0], Yva[b0:b1], acc=acc)

    def run(self):
        """The summed validation loss of the epoch (a device scalar; the caller divides by `nb_va`)."""
        st, engine, Xva, Yva, bs = self.st, self.st.engine, self.st.Xva, self.st.Yva, self.st.cfg.batch_size
        if engine is not None and engine.repack_params is not None and self.engine_eval:
            engine.repack_now()          # (the engine's evaluation launches read the weight copies: the last update's are not built yet)
        vt = torch.zeros((), device=st.device)
        if self.engine_eval and self.slot_graph is not None:
            self.slot_graph.replay()
            return engine.eval_slot_losses().sum()
        if self.engine_eval:
            engine.eval_loss_sum.zero_()
            if self.val_rows is None:
                self.val_rows = torch.arange(Xva.shape[0], device=st.device)
            for b in range(self.nb_va):
                rows = self.val_rows[b * bs:(b + 1) * bs]
                gk = self.ev_graphs.get(int(rows.numel()))
                if gk is not None:
                    gk[1].copy_(rows)
                    gk[0].replay()
                else:
                    engine.gather(Xva, Yva, rows, None, 0)
                    engine.evaluate(int(rows.numel()))
            return engine.eval_loss_sum.clone()
        if self.val_whole:
            if self.vgraph_all is None:
                self._whole(vt)
                return vt
            self.vgraph_all.replay()
        else:
            for b in range(self.nb_va):
                xb, yb = Xva[b * bs:(b + 1) * bs], Yva[b * bs:(b + 1) * bs]
                gk = self.vgraphs.get(int(xb.shape[0]))
                if gk is not None:
                    gk[1].copy_(xb); gk[2].copy_(yb)
                    gk[0].replay()
                else:
                    vt += self._batch(xb, yb)
            if not self.vgraphs:
                return vt
        vt += self.v_acc                 # what the replays added up
        self.v_acc.zero_()
        return vt


def _run_epochs(st: _Step, n_epochs: int, batch_order, log):
    """The captures, then the epochs; returns (history, best validation loss, its state dict, the data-parallel profile's event quadruples
    or None, the step's mode).  The graphs (and their private memory pools) belong to two objects that are locals of THIS frame and in no
    reference cycle: they are gone when it returns, before anything else runs on the device."""
    cap = _CapturedStep(st, log)
    val = _Validation(st, cap, log)
    # "the warm-up steps never happened" for the dropout / noise streams too: their call counters go back to zero, so that a seeded run
    # draws the same masks however many warm-up and capture passes its launch mode needed (one graph, two graphs around the collective,
    # with or without a tail graph, eager) -- r05: the one-rank data-parallel run reproduces the plain run
    if st.on_gpu:
        st.prep_counter.zero_()
        if st.engine is not None:
            st.engine.drop_counter.zero_(); st.engine.prep_counter.zero_()
        if st.fuse_gather:
            st.g_cursor.zero_()
    cfg, device, model, opt, engine, loss_acc = st.cfg, st.device, st.model, st.opt, st.engine, st.loss_acc
    Xtr, Ytr, bs, nb_tr, graph = st.Xtr, st.Ytr, st.cfg.batch_size, st.nb_tr, cap.graph
    hist = {"train": [], "val": [], "epoch_s": []}
    best_val, best_state, no_improve = float("inf"), None, 0
    # the epochs' shuffles come from a generator of their own: the framework's global one is consumed by eager steps (input noise,
    # framework dropout) but not by graph replays, so the batch order of epoch 2 would depend on which steps happened to run eagerly
    perm_gen = torch.Generator(device=device)
    perm_gen.manual_seed(st.seed * 1000003 + 17 + st.rank)
    seg_ev = [] if (_DP_PROFILE and st.on_gpu and graph is not None) else None      # per-step event quadruples (first epoch excluded by the caller)
    first_one_graph_replay = cap.one_graph               # the captured collective's first replay runs under the stall timer
    own_sum = engine is not None or loss_acc is not None # a launch of the step adds its loss to the epoch's running sum itself
    for epoch in range(1, n_epochs + 1):
        if st.on_gpu:
            torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        model.train()
        noise = cfg.sigma_0 * (cfg.gamma_noise ** epoch)                     # PINN:743
        if batch_order is not None:
            order = torch.as_tensor(batch_order(epoch), dtype=torch.long).reshape(-1).to(device)
        else:
            order = torch.randperm(Xtr.shape[0], device=device, generator=perm_gen)      # DataLoader(shuffle=True), PINN:701
        tot = torch.zeros((), device=device)
        if engine is not None:
            engine.loss_sum.zero_()                                          # the output launch adds every step's loss to it
        if loss_acc is not None:
            loss_acc.zero_()                                                 # ... and so does the fused loss launch of the other loops
        noise_t = torch.tensor(noise, device=device)
        if graph is not None:
            cap.s_noise.copy_(noise_t)                                       # constant within the epoch
        if st.fuse_gather:                                                   # the front-end launch walks this permutation with its own cursor
            st.g_order[:order.numel()].copy_(order)
            st.g_cursor.zero_()
            st.g_noise.copy_(noise_t)
        for b in range(nb_tr):
            # `order` is the DataLoader shuffle; permute_data (PINN:753) re-permutes inside the batch, which
            # changes neither the batch statistics nor the mean loss, so it is folded into `order`
            idx = order[b * bs:(b + 1) * bs]
            if graph is not None and idx.numel() == bs:
                cap.feed(idx, cap.sX, cap.sY)
                if first_one_graph_replay:
                    first_one_graph_replay = False
                    with _StallGuard(_DP_STALL_S, "the first replay of the data-parallel step graph (gradient all-reduce captured)"):
                        graph.replay()
                        torch.cuda.synchronize(device)
                    if not own_sum:
                        tot += cap.s_loss
                    continue
                if seg_ev is not None and len(seg_ev) < 4096:
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                    ev[0].record()
                    graph.replay()
                    ev[1].record()
                    if cap.graph_b is not None:
                        st.allreduce_grads()
                        ev[2].record()
                        cap.graph_b.replay()
                    else:
                        ev[2].record()
                    ev[3].record()
                    seg_ev.append(ev)
                else:
                    graph.replay()
                    if cap.graph_b is not None:
                        st.allreduce_grads()
                        cap.graph_b.replay()
                step_loss, where = cap.s_loss, (b, cap.sX, cap.sY)
            elif cap.graph_t is not None and idx.numel() == cap.sYt.shape[0]:
                cap.feed(idx, cap.sXt, cap.sYt)
                cap.graph_t.replay()
                step_loss, where = cap.s_loss_t, (-b, cap.sXt, cap.sYt)
            elif engine is not None:
                st.train_step(None, Ytr[:idx.numel()], noise_t, idx)         # Yb only carries the row count here
            else:
                if st.shared_counter and not st.fuse_gather:
                    st.prep_counter[0:1].add_(1)                             # (no batch-assembly launch on this path: advance the streams here)
                step_loss = st.train_step(Xtr[idx], Ytr[idx], noise_t, idx)
                where = (-b, Xtr[idx], Ytr[idx]) if _DEBUG_NAN else None
            if not own_sum:
                tot += step_loss
            if _DEBUG_NAN and engine is None:
                _debug_nan(model, opt, st.flat, step_loss, epoch, *where)
        if engine is not None:
            tot = engine.loss_sum.clone()
        elif loss_acc is not None:
            tot = loss_acc.clone()
        train_loss = _allreduce_mean(tot / nb_tr, st.world, st.dp)
        if st.dp:   # BatchNorm running statistics are per rank during the epoch: average them before evaluating
            for buf in model.buffers():
                if buf.is_floating_point():
                    dist.all_reduce(buf)
                    buf.div_(st.world)
        model.eval()
        val_loss = _allreduce_mean(val.run() / val.nb_va, st.world, st.dp)
        if st.sched is not None:
            st.sched.step()                                                  # PINN:788
        else:
            opt.lr.mul_(cfg.gamma)                                           # ExponentialLR on the device scalar
        tl, vl = float(train_loss), float(val_loss)                          # the epoch's only host syncs
        if st.on_gpu:
            torch.cuda.synchronize(device)
        hist["train"].append(tl); hist["val"].append(vl); hist["epoch_s"].append(time.perf_counter() - t0)
        if vl < best_val:                                                    # PINN:791-799
            best_val, no_improve = vl, 0
            best_state = copy.deepcopy(model.state_dict())
        else:
            no_improve += 1
        if log and st.rank == 0:
            log(f"Epoch {epoch}/{n_epochs} | Train Loss={tl:.6f}, Val Loss={vl:.6f}, Time={hist['epoch_s'][-1]:.2f}s")
        if no_improve >= cfg.patience:
            break
    step_mode = "one graph incl. the all-reduce" if cap.one_graph else "graph A | all-reduce | graph B" if graph is not None else "eager"
    return hist, best_val, best_state, seg_ev, step_mode


def _train_surrogate(kind: str, data: SurrogateData, cfg=None, device="cuda", *, autocast_dtype=torch.bfloat16,
                     sync_bn: bool = False, max_epochs: Optional[int] = None, log=None, seed: int = 0,
                     use_graph: Optional[bool] = None, physics: Union[PhysicsTerm, DesignTerm, None] = None,
                     init_fn=None, batch_order=None) -> Dict[str, object]:
    """Trains on THIS rank's `data` shard; uses DDP when torch.distributed is initialised with world_size > 1.
    Returns history, best state dict, validation R^2 (I only) and per-epoch times.
    `init_fn(model)`: called once on the freshly built model (load a checkpoint, deterministic test weights).
    `batch_order(epoch) -> LongTensor[n_train]`: the epoch's sample order instead of a random permutation (the
    reference's DataLoader shuffle, PINN:701, is unseeded; the golden-fixture tests replay the order it drew).
    `autocast_dtype=torch.float16`: the reference's AMP mode (fp16 autocast + GradScaler, PINN:706, :759-768) on the framework modules; the
    returned dict then carries `grad_scaler` = {"scale", "skipped_steps", "steps"}.
    (An exception in `_run_epochs` skips the teardown below, as it always has: what the run armed lives on its own model's state.)"""
    st = _setup_step(kind, data, cfg, device, autocast_dtype, sync_bn, log, seed, use_graph, physics, init_fn)
    cfg, model, device = st.cfg, st.model, st.device
    hist, best_val, best_state, seg_ev, step_mode = _run_epochs(st, max_epochs if max_epochs is not None else cfg.num_epochs, batch_order, log)
    if st.on_gpu:
        import gc
        gc.collect()                     # (no cycle of this module's making is left to collect; kept for whatever a model's own pieces form)
        torch.cuda.synchronize(device)
        # BLAS workspaces that were allocated while capturing live in the graphs' private pools but stay cached per (handle, stream):
        # a later run whose side stream gets the same id would hand that freed memory to its GEMMs as scratch space (seen as NaNs /
        # drifting losses in a framework-path TFD run after a fast-path one in the same process)
        clear_blas_workspaces()
    disable_shadow_linears(st.patched)   # the returned model is a plain module again
    if st.fast_encoder is not None:
        st.tfd.unpatch_model(st.fast_encoder)      # (its states go, and the armed batch assembly with them)
    if hasattr(model, "direct_param_grads"):
        model.direct_param_grads = False
    if best_state is not None:
        model.load_state_dict(best_state)
    model.eval()
    Xva, Yva, nel, sI = st.Xva, st.Yva, cfg.nelem, data.scalers_Y["I"]
    with torch.no_grad():
        preds = torch.cat([model(Xva[i:i + cfg.batch_size]).float() for i in range(0, Xva.shape[0], cfg.batch_size)])
    p = sI.inverse_transform(preds[:, :nel]).clamp(0.0, 1e10)                # PINN:843-848
    t = sI.inverse_transform(Yva[:, :nel]).clamp(0.0, 1e10)
    # (the reference's evaluation block, PINN:815-852 / TFD:800-829: best checkpoint reloaded, evaluation-mode pass over the validation
    #  set in loader order, inertias un-standardised and clipped to [0, 1e10], r2_score on the raveled arrays)
    out = {"model": model, "history": hist, "best_val": best_val, "best_state": best_state, "r2_val_I": r2_score(t, p),
           "val_pred_I": p, "val_true_I": t, "epochs": len(hist["train"]), "steps_per_epoch": st.nb_tr}
    if isinstance(physics, DesignTerm):
        # the metric a user of the surrogate cares about: how far the predicted designs are from the labels in objective
        from .design_loss import design_gap
        out["design_gap_val"] = design_gap(model, data, physics, "val")
        out["design_term_sum"] = float(st.physics.term_sum)
    if st.fp16_scaler is not None:
        out["grad_scaler"] = {"scale": st.fp16_scaler["scale"], "skipped_steps": st.fp16_scaler["skipped"], "steps": st.fp16_scaler["steps"]}
    if st.dp:
        out["dp_mode"] = {"world": st.world, "forced_one_rank": bool(st.world == 1), "backend": dist.get_backend(), "async": bool(_DP_ASYNC),
                          "step": step_mode}
    if seg_ev:                           # mean device time of the step's segments over the profiled steps (first epoch's excluded)
        use = seg_ev[st.nb_tr:] or seg_ev
        mean = lambda i, j: 1e3 * sum(e[i].elapsed_time(e[j]) for e in use) / len(use)      # noqa: E731
        out["dp_segments"] = {"steps": len(use), "step_us": mean(0, 3), "graph_a_us": mean(0, 1), "allreduce_us": mean(1, 2),
                              "graph_b_us": mean(2, 3), "one_graph": step_mode.startswith("one graph"), "world": st.world}
    return out


def save_best(state: Dict[str, torch.Tensor], path: str) -> None:
    """`torch.save(model.state_dict(), "best_model_*.pth")` (PINN:794, TFD:777)."""
    torch.save(state, path)
