"""The flat float32 gradient buffer of a training step and the optimiser over it: host side of csrc/flat_adam.hip."""
import torch

from . import _cabi


def flat_grads(params, device) -> torch.Tensor:
    """One zeroed float32 buffer with every `q.grad` of `params` a view of it, in parameter order (autograd accumulates in place): what
    FlatClipAdam, shadow.enable_shadow_linears and pinn_fused.PinnFusedStep expect, and what the data-parallel step all-reduces."""
    params = list(params)                # (walked twice: a generator such as model.parameters() must not run dry before the views are attached)
    flat = torch.zeros(sum(q.numel() for q in params), device=device, dtype=torch.float32)
    off = 0
    for q in params:
        q.grad = flat[off:off + q.numel()].view_as(q)
        off += q.numel()
    return flat


class FlatClipAdam:
    """`clip_grad_norm_(params, max_norm)` + `torch.optim.Adam(lr, weight_decay)` as two HIP launches over flat buffers
    (csrc/flat_adam.hip).  The parameters are re-homed into one flat float32 buffer (each `p.data` becomes a view of it),
    next to the flat gradient buffer the training loop already all-reduces; `lr` and the step count are device scalars,
    so a captured HIP graph follows the scheduler."""

    def __init__(self, params, flat_grad: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_norm: float = 1.0, decoupled: bool = False):
        self._lib = _cabi.load()
        dev = flat_grad.device
        self.p = torch.empty_like(flat_grad)
        off = 0
        with torch.no_grad():
            for q in params:
                n = q.numel()
                self.p[off:off + n].copy_(q.reshape(-1))
                q.data = self.p[off:off + n].view_as(q)
                off += n
        assert off == flat_grad.numel()
        self.g = flat_grad
        self.m, self.v = torch.zeros_like(flat_grad), torch.zeros_like(flat_grad)
        self.lr = torch.tensor(float(lr), dtype=torch.float32, device=dev)
        self.step_count = torch.zeros((), dtype=torch.int32, device=dev)
        self.ws = torch.empty(int(self._lib.ops_flat_adam_workspace_bytes()), dtype=torch.uint8, device=dev)
        self.betas, self.eps, self.weight_decay, self.max_norm, self.decoupled = betas, eps, weight_decay, max_norm, decoupled
        self.p_bf16 = None          # bfloat16 shadow of the parameters (enable_shadow)
        self.zero_grads = False     # zero the gradient buffer inside the update launch (the next step's zero_grad(): one fill node less)
        self.repack = None          # ctypes array of MlpRepackEntry: padded bf16 weight copies the update refreshes too (pinn_fused.py)
        self.norm_ready_parts = 0   # > 0: the gradient producers leave that many norm partial sums + the advanced step in `ws` (pinn_fused.enable_norm)

    def enable_shadow(self) -> torch.Tensor:
        """A bfloat16 copy of the flat parameter buffer that every step refreshes in the Adam kernel itself: layers that
        run their GEMMs in bfloat16 read it instead of casting their float32 weights in every forward pass."""
        if self.p_bf16 is None:
            self.p_bf16 = self.p.to(torch.bfloat16)
        return self.p_bf16

    def refresh_shadow(self) -> None:
        if self.p_bf16 is not None:
            self.p_bf16.copy_(self.p)

    def step(self, grad_scale: float = 1.0) -> None:
        dev = self.g.device
        args = (self.g.numel(), self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.lr.data_ptr(),
                self.step_count.data_ptr(), self.max_norm, grad_scale, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                int(self.decoupled) | (2 if self.zero_grads else 0) | ((_cabi.ADAM_NORM_READY | (self.norm_ready_parts << 16)) if self.norm_ready_parts else 0),
                self.p_bf16.data_ptr() if self.p_bf16 is not None else None, self.ws.data_ptr())
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            if self.repack is not None:
                _cabi.check(self._lib.ops_flat_clip_adam_step_repack_f32(*args, len(self.repack), self.repack, s), "ops_flat_clip_adam_step_repack_f32")
            else:
                _cabi.check(self._lib.ops_flat_clip_adam_step_f32(*args, s), "ops_flat_clip_adam_step_f32")

    def state_dict(self):
        return {"m": self.m.clone(), "v": self.v.clone(), "step": self.step_count.clone(), "lr": self.lr.clone()}

    def load_state_dict(self, sd) -> None:
        self.m.copy_(sd["m"]); self.v.copy_(sd["v"]); self.step_count.copy_(sd["step"]); self.lr.copy_(sd["lr"])
