"""The bf16 shadow-product protocol: y = x W^T + b on the optimiser's bfloat16 copy of the parameters, and how a product's weight / bias
gradients leave a backward pass (shadow_param_grads) -- for the autograd path (_ShadowLinearFn) and the fused blocks of tfd_fused.py."""
import contextlib

import torch

from . import _cabi, switches

F_linear = torch.nn.functional.linear

# products over at least this many rows take the split-row kernel (0: never).  r04: 16 (was 512) -- the kernel now keeps a whole tile per wave and
# reduces inside the workgroup, so a 10-sample tail batch (70 / 10 rows: twelve library GEMMs of ~16 us + twelve column sums per epoch)
# is one grouped launch too; only products over fewer rows than one MFMA tile stay with the library
_SPLIT_WGRAD_ROWS = int(switches.get("split_wgrad_rows"))

# The step that is collecting right now (grouped_wgrads; autograd nodes reach it here): the list of what its backward pass has queued for
# the grouped weight-gradient launches -- job tuples (dY, X, dW, dbias), whose operands stay alive in here, and at most one callable, a
# launch that must run in front of them (run_before_wgrad_flush).  None: no step is collecting
_WGRAD_QUEUE = None


class ShadowRec:
    """One shadow product's operands and gradient destinations (enable_shadow_linears): the weight / bias gradients leave (in bfloat16)
    through `stash`, from where ONE multi-tensor copy moves all of them into the flat float32 gradient buffer -- or, for products over
    many rows, are added straight into `w_grad` / `b_grad`, the parameters' slices of the zeroed flat gradient buffer."""
    __slots__ = ("w_sh", "b_sh", "w_grad", "b_grad", "stash", "iw", "ib")

    def __init__(self, w_sh, b_sh, w_grad, b_grad, stash, iw, ib):
        self.w_sh, self.b_sh, self.w_grad, self.b_grad, self.stash, self.iw, self.ib = w_sh, b_sh, w_grad, b_grad, stash, iw, ib


class _ShadowLinearFn(torch.autograd.Function):
    """y = x W^T + b with W, b taken from the optimiser's bfloat16 shadow (`rec`: ShadowRec); the weight / bias gradients are not
    returned to autograd but go where `shadow_param_grads` sends them.  Same arithmetic as nn.Linear under bf16 autocast (bf16 operands,
    fp32 accumulation, bf16 results), without its per-step kernels: weight cast, bias cast, gradient cast back and accumulate -- four
    per parameter."""

    @staticmethod
    def forward(ctx, x, rec, anchor, gx_dest=None):
        # `anchor` (the layer's float32 weight Parameter) is not read: it makes autograd record the node even when x
        # needs no gradient (first layer); its own gradient slot stays None
        # `gx_dest`: the backward pass writes the input gradient straight into it (a [rows, K] bfloat16 tensor, rows may be strided) instead of
        # a fresh tensor: the Transformer-Diffusion head hands the [CLS] rows of a persistent zero tensor, and the row scatter that followed
        # the product disappears from the step
        w_sh, b_sh = rec.w_sh, rec.b_sh
        xb = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        x2 = xb.reshape(-1, xb.shape[-1])
        y = torch.addmm(b_sh, x2, w_sh.t()) if b_sh is not None else x2 @ w_sh.t()
        ctx.save_for_backward(x2, w_sh)
        ctx.rec, ctx.xshape, ctx.xdtype = rec, x.shape, x.dtype
        ctx.gx_dest = gx_dest if (gx_dest is not None and switches.get("gx_dest") == "1") else None
        return y.reshape(*x.shape[:-1], w_sh.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, w_sh = ctx.saved_tensors
        g2 = gy.reshape(-1, gy.shape[-1])
        if g2.dtype != torch.bfloat16:
            g2 = g2.to(torch.bfloat16)
        g2 = shadow_param_grads(ctx.rec, g2, x2, row_stride_switch=True)
        gx = None
        if ctx.needs_input_grad[0]:
            dest = ctx.gx_dest
            if dest is not None and dest.dtype == torch.bfloat16 and tuple(dest.shape) == (g2.shape[0], w_sh.shape[1]) and ctx.xdtype == torch.bfloat16:
                gx = torch.mm(g2, w_sh, out=dest)
            else:
                gx = (g2 @ w_sh).reshape(ctx.xshape)
                if gx.dtype != ctx.xdtype:
                    gx = gx.to(ctx.xdtype)
        return gx, None, None, None


def collecting() -> bool:
    """True inside a `grouped_wgrads` block that collects: what the backward pass queues is launched at the block's exit."""
    return _WGRAD_QUEUE is not None


def queue_column_sums(rows: torch.Tensor, dest: torch.Tensor) -> bool:
    """dest [N] (float32, a slice of the zeroed flat gradient buffer) += column sums of rows [T, N] (float32, unit column stride) as a job
    of the step's grouped weight-gradient launch.  False when no grouped launch is being collected (the caller adds them itself)."""
    if _WGRAD_QUEUE is None or rows.dtype != torch.float32 or rows.stride(1) != 1 or dest.dtype != torch.float32 or not dest.is_contiguous():
        return False
    _WGRAD_QUEUE.append((rows, None, dest, None))
    return True


def shadow_param_grads(rec: ShadowRec, g2: torch.Tensor, x2: torch.Tensor, row_stride_switch: bool = False) -> torch.Tensor:
    """Weight / bias gradients of y = x W^T + b given dY = g2 [T, N] and X = x2 [T, K] (bfloat16) -- the one statement of the protocol,
    for _ShadowLinearFn.backward and for the fused blocks that run the product themselves: queued for the step's grouped split-row launch
    (launched at once where no step collects) when the product has many rows, the library's product into the stash otherwise.
    `row_stride_switch`: a row-strided x2 travels without a copy only with the switch wgrad_rows on (the autograd path; the fused blocks
    always hand theirs over as it is).  Returns dY as it was used (made contiguous on the split-row path)."""
    if rec.w_grad is not None and x2.shape[0] >= _SPLIT_WGRAD_ROWS and _SPLIT_WGRAD_ROWS > 0:
        # many rows, small output: the library walks all rows inside a handful of tiles (25 us for 3584 x 360 x 120) and the bias
        # gradient is another reduction pass (11 us); the split-row kernel of csrc/seq_block.hip adds partial tiles -- and the
        # column sums of the slabs it reads anyway -- into the float32 gradients itself
        g2 = g2.contiguous()
        rows_ok = ((not row_stride_switch or switches.get("wgrad_rows") == "1") and _WGRAD_QUEUE is not None and x2.dim() == 2
                   and x2.stride(1) == 1 and x2.stride(0) >= x2.shape[1])
        x2c = x2 if rows_ok else x2.contiguous()          # the grouped launch takes row strides (the head reads the [CLS] rows in place)
        fused_bias = rec.ib is not None and rec.b_grad is not None
        if _WGRAD_QUEUE is not None:
            # deferred: the training step launches every queued product at once after backward (flush_wgrad_queue)
            _WGRAD_QUEUE.append((g2, x2c, rec.w_grad, rec.b_grad if fused_bias else None))
        else:
            with torch.cuda.device(g2.device):
                rc = _cabi.load().ops_linear_wgrad_accumulate(x2c.shape[0], g2.shape[1], x2c.shape[1], g2.data_ptr(), x2c.data_ptr(),
                                                              rec.w_grad.data_ptr(), rec.b_grad.data_ptr() if fused_bias else None,
                                                              torch.cuda.current_stream(g2.device).cuda_stream)
            _cabi.check(rc, "ops_linear_wgrad_accumulate")
        if rec.ib is not None and not fused_bias:
            rec.stash[rec.ib] = g2.sum(0)
    else:
        rec.stash[rec.iw] = g2.t() @ x2
        if rec.ib is not None:
            rec.stash[rec.ib] = g2.sum(0)
    return g2


def shadow_grads_are_deferred(rec: ShadowRec, rows: int) -> bool:
    """True when `shadow_param_grads(rec, g2, x2)` over `rows` rows only QUEUES its work for the step's grouped launch -- it then reads
    neither operand before `flush_wgrad_queue`.  A caller whose kernel has not yet written g2 (tfd_fused: the later layer of a
    pair launch) may only wait in that case: the library products and column sums of the other branches run at once."""
    return (_WGRAD_QUEUE is not None and rec.w_grad is not None and _SPLIT_WGRAD_ROWS > 0 and rows >= _SPLIT_WGRAD_ROWS
            and (rec.ib is None or rec.b_grad is not None))


@contextlib.contextmanager
def grouped_wgrads(device, stash, dst, enabled: bool = True):
    """`with grouped_wgrads(device, stash, dst): loss.backward()` -- the backward protocol of a step on shadow products: while the body runs
    the split-row weight gradients are collected (`enabled` False: every product launches inside backward); a clean exit launches them
    grouped, moves the live `stash` entries (bfloat16) into their float32 destinations `dst` with one multi-tensor copy and clears the
    stash.  An exception skips all that; either way nothing is left collecting."""
    global _WGRAD_QUEUE
    _WGRAD_QUEUE = [] if enabled else None
    try:
        yield _WGRAD_QUEUE
        flush_wgrad_queue(device)
    finally:
        _WGRAD_QUEUE = None
    live = [(dd, ss) for dd, ss in zip(dst, stash) if ss is not None]      # (a product nobody called this step leaves None)
    if live:
        torch._foreach_copy_([dd for dd, _ in live], [ss for _, ss in live])
    for k in range(len(stash)):
        stash[k] = None


def run_before_wgrad_flush(launch) -> None:
    """`launch()` runs at the collecting step's flush, in front of its grouped launches (tfd_fused: a layer's backward launch that waits
    for a predecessor which may never run); None: the one that waited has been taken care of.  At most one waits at a time."""
    if _WGRAD_QUEUE is not None:
        waiting = [e for e in _WGRAD_QUEUE if callable(e)]
        assert launch is None or not waiting
        for e in waiting:
            _WGRAD_QUEUE.remove(e)
        if launch is not None:
            _WGRAD_QUEUE.append(launch)


def flush_wgrad_queue(device) -> None:
    """Launch what the collecting step holds: the waiting launch, then everything queued, 16 products per launch."""
    if not _WGRAD_QUEUE:
        return
    for launch in [e for e in _WGRAD_QUEUE if callable(e)]:
        launch()
    q = [e for e in _WGRAD_QUEUE if not callable(e)]
    _WGRAD_QUEUE.clear()
    if not q:
        return
    lib = _cabi.load()
    with torch.cuda.device(device):
        s = torch.cuda.current_stream(device).cuda_stream
        for i0 in range(0, len(q), _cabi.WGRAD_MAX_GROUP):
            part = q[i0:i0 + _cabi.WGRAD_MAX_GROUP]
            arr = (_cabi.WgradProblem * len(part))()
            for e, (g2, x2, wg, bg) in zip(arr, part):
                if x2 is None:                                           # column-sum job: wg [N] += column sums of the float32 rows g2 [T, N]
                    e.T, e.N, e.K = g2.shape[0], g2.shape[1], 0
                    e.dY, e.X, e.dW, e.dbias, e.ldy, e.ldx = g2.data_ptr(), None, wg.data_ptr(), None, g2.stride(0), 0
                    continue
                e.T, e.N, e.K = x2.shape[0], g2.shape[1], x2.shape[1]
                e.dY, e.X, e.dW, e.dbias = g2.data_ptr(), x2.data_ptr(), wg.data_ptr(), (bg.data_ptr() if bg is not None else None)
                e.ldy, e.ldx = g2.stride(0), x2.stride(0)                # (row views with unit column stride travel without a copy)
            _cabi.check(lib.ops_linear_wgrad_accumulate_group(len(part), arr, s), "ops_linear_wgrad_accumulate_group")


def enable_shadow_linears(model: torch.nn.Module, opt, params, flat: torch.Tensor):
    """Routes every plain nn.Linear of `model` through _ShadowLinearFn (`opt`: a flat_adam.FlatClipAdam).  Returns (stash, grad_views, patched modules)."""
    import types
    sh = opt.enable_shadow()
    offs, off = {}, 0
    for q in params:
        offs[id(q)] = off
        off += q.numel()
    stash, dst, patched = [], [], []

    def register(weight, bias):
        """y = x W^T + b through the shadow of (weight, bias); their gradients travel through `stash` (or, for products over
        thousands of rows, are added straight into their slices of the zeroed flat gradient buffer)."""
        ow = offs[id(weight)]
        w_sh = sh[ow:ow + weight.numel()].view_as(weight)
        w_grad = flat[ow:ow + weight.numel()].view_as(weight)
        iw = len(stash); stash.append(None); dst.append(w_grad)
        b_sh, ib, b_grad = None, None, None
        if bias is not None:
            ob = offs[id(bias)]
            b_sh = sh[ob:ob + bias.numel()]
            b_grad = flat[ob:ob + bias.numel()]
            ib = len(stash); stash.append(None); dst.append(b_grad)
        # (also what a fused block that runs this product itself needs: the shadow operands, and where its gradients go -- shadow_param_grads)
        rec = ShadowRec(w_sh, b_sh, w_grad, b_grad, stash, iw, ib)

        def prod(x, gx_dest=None):
            return _ShadowLinearFn.apply(x, rec, weight, gx_dest)

        prod.rec = rec
        return prod

    for mod in model.modules():
        if isinstance(mod, torch.nn.MultiheadAttention):
            # the attention's projections are bare Parameters / a Linear subclass that its functional forward never calls: hand the
            # shadow products to the encoder fast path (tfd_fused.py), which is their only user
            if mod._qkv_same_embed_dim and mod.in_proj_bias is not None and id(mod.in_proj_weight) in offs and id(mod.out_proj.weight) in offs:
                mod._ops_in_proj = register(mod.in_proj_weight, mod.in_proj_bias)
                mod._ops_out_proj = register(mod.out_proj.weight, mod.out_proj.bias)
                patched.append(mod)
            continue
        if type(mod) is not torch.nn.Linear or id(mod.weight) not in offs:
            continue
        prod = register(mod.weight, mod.bias)

        def fwd(self, x, prod=prod):
            if not x.is_cuda:
                return F_linear(x, self.weight, self.bias)
            return prod(x)

        mod.forward = types.MethodType(fwd, mod)
        mod._ops_prod = prod
        patched.append(mod)
    return stash, dst, patched


def disable_shadow_linears(patched) -> None:
    for mod in patched:
        if "forward" in mod.__dict__:
            del mod.__dict__["forward"]
        for name in ("_ops_in_proj", "_ops_out_proj", "_ops_prod"):
            if name in mod.__dict__:
                del mod.__dict__[name]
