"""Bayesian Transformer-Diffusion surrogates (BTFD / BTFDM): weight sampling for the training step and Monte-Carlo uncertainty.

    mean, std = predict_with_uncertainty(model, X, n_samples=50, scaler=scaler_Y)

is the GPU replacement of the _Meta_ script's `get_bnn_output_stats` (50 sequential eager forwards, a `.cpu()` each) followed by its
un-standardisation: every sample's diffusion draws and Bayesian weights come from counter-based streams inside two MC calls of
csrc/bayes_mlp.hip (the diffusion MLP and the output head, fp32), the encoder runs ONCE over the S * B sequences, a third launch
reduces the samples to mean and std (ddof = 0).  There is no CPU path: without the HIP library this raises.

Training: `BayesSampler` draws the four Bayesian layers' weights of a step in ONE launch (ops_bayes_sample_f32) behind an autograd
Function whose backward folds dW into (dmu, dls) in ONE launch (ops_bayes_grad_fold_f32), recomputing the draws from the step counter.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _cabi
from .surrogates import BayesLinear

_MASK64 = (1 << 64) - 1


def _mix(z: int) -> int:
    """splitmix64 finaliser (seeds of the sub-streams)."""
    z = (z + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _check_gpu(*ts):
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("the Bayesian launches take contiguous float32 GPU tensors")


def bayes_layers(model) -> list:
    return model.bayes_layers() if hasattr(model, "bayes_layers") else [m for m in model.modules() if isinstance(m, BayesLinear)]


def bayesian_kl(model, prior_mu: Optional[float] = None, prior_sigma: Optional[float] = None) -> torch.Tensor:
    """sum over every BayesLinear parameter of KL(N(mu, exp(ls)^2) || N(prior_mu, prior_sigma^2)) (closed form; the layers' own prior
    unless given).  The opt-in KL term of `train_surrogate` is `bnn_kl_scale` times this."""
    total = None
    for m in bayes_layers(model):
        m0 = m.prior_mu if prior_mu is None else prior_mu
        s0 = m.prior_sigma if prior_sigma is None else prior_sigma
        pairs = [(m.weight_mu, m.weight_log_sigma)] + ([(m.bias_mu, m.bias_log_sigma)] if m.bias else [])
        for mu, ls in pairs:
            kl = (torch.log(torch.tensor(s0, dtype=mu.dtype, device=mu.device)) - ls
                  + (torch.exp(2 * ls) + (mu - m0) ** 2) / (2 * s0 * s0) - 0.5).sum()
            total = kl if total is None else total + kl
    if total is None:
        raise ValueError("the model has no BayesLinear layer")
    return total


# ------------------------------------------------------------------------------------------------------------------------------------
# training: one sampling launch per step, one fold launch in backward
# ------------------------------------------------------------------------------------------------------------------------------------
def _layer_structs(layers, outs=None, eps=None, grads=None, dparams=None):
    arr = (_cabi.BayesLayer * len(layers))()
    for i, m in enumerate(layers):
        e = arr[i]
        e.out_f, e.in_f = m.out_features, m.in_features
        e.w_mu, e.w_ls, e.b_mu, e.b_ls = (_ptr(m.weight_mu), _ptr(m.weight_log_sigma), _ptr(m.bias_mu), _ptr(m.bias_log_sigma))
        if outs is not None:
            e.w, e.b = _ptr(outs[2 * i]), _ptr(outs[2 * i + 1])
        if eps is not None:
            e.w_eps, e.b_eps = _ptr(eps[2 * i]), _ptr(eps[2 * i + 1])
        if grads is not None:
            e.dw, e.db = _ptr(grads[2 * i]), _ptr(grads[2 * i + 1])
            e.d_wmu, e.d_wls, e.d_bmu, e.d_bls = (_ptr(t) for t in dparams[4 * i:4 * i + 4])
    return arr


class _BayesSampleFn(torch.autograd.Function):
    """(mu, ls) of every layer -> (W, b) of every layer; backward: the fold launch."""

    @staticmethod
    def forward(ctx, sampler, *params):
        layers = sampler.layers
        outs = []
        for m in layers:
            outs += [torch.empty_like(m.weight_mu), torch.empty_like(m.bias_mu)]
        eps, mode = sampler.eps_buffers()
        lib = _cabi.load()
        dev = params[0].device
        # this call's counter value, kept for ITS backward (another forward before it may advance the sampler's counter)
        ctr = sampler.counter.clone()
        with torch.cuda.device(dev):
            rc = lib.ops_bayes_sample_f32(len(layers), _layer_structs(layers, outs=outs, eps=eps), sampler.seed, ctr.data_ptr(),
                                          mode, torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(rc, "ops_bayes_sample_f32")
        ctx.sampler = sampler
        ctx.eps = eps
        ctx.ctr = ctr
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        sampler = ctx.sampler
        layers = sampler.layers
        g = []
        for i, m in enumerate(layers):
            for k, ref in ((2 * i, m.weight_mu), (2 * i + 1, m.bias_mu)):
                gi = grads[k]
                g.append(torch.zeros_like(ref) if gi is None else gi.float().contiguous())
        dparams = []
        for m in layers:
            dparams += [torch.empty_like(m.weight_mu), torch.empty_like(m.weight_log_sigma), torch.empty_like(m.bias_mu),
                        torch.empty_like(m.bias_log_sigma)]
        mode = _cabi.BAYES_EPS_READ if ctx.eps is not None else _cabi.BAYES_EPS_DRAW
        lib = _cabi.load()
        dev = g[0].device
        with torch.cuda.device(dev):
            rc = lib.ops_bayes_grad_fold_f32(len(layers), _layer_structs(layers, eps=ctx.eps, grads=g, dparams=dparams), sampler.seed,
                                             ctx.ctr.data_ptr(), mode, float(sampler.kl_scale), float(sampler.prior_mu),
                                             float(sampler.prior_sigma), torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(rc, "ops_bayes_grad_fold_f32")
        return (None, *dparams)


class BayesSampler:
    """Set as `model.bayes_sampler`: every forward call advances the device-resident step counter (a captured node under graph replay)
    and draws all Bayesian layers' (W, b) in one launch.  `kl_scale` > 0: the fold adds kl_scale * the KL gradient (the loss then adds
    the KL VALUE without a graph: `bayesian_kl(model).detach()`).  `replay` = list of [w_eps, b_eps] per layer and `mode` "write" (the
    launch writes its draws there) or "read" (it uses them): tests only."""

    def __init__(self, model, seed: int = 0, kl_scale: float = 0.0, device=None):
        self.layers = bayes_layers(model)
        if not self.layers or len(self.layers) > _cabi.BAYES_MAX_LAYERS or not all(m.bias for m in self.layers):
            raise ValueError("BayesSampler needs 1 .. 8 BayesLinear layers with biases")
        dev = device or self.layers[0].weight_mu.device
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.seed = _mix(int(seed) ^ 0xB7E151628AED2A6B)
        self.kl_scale = float(kl_scale)
        self.prior_mu, self.prior_sigma = self.layers[0].prior_mu, self.layers[0].prior_sigma
        self.replay, self.mode = None, None

    def eps_buffers(self):
        if self.replay is None:
            return None, _cabi.BAYES_EPS_DRAW
        flat = [t for pair in self.replay for t in pair]
        return flat, (_cabi.BAYES_EPS_WRITE if self.mode == "write" else _cabi.BAYES_EPS_READ)

    def __call__(self, model=None):
        for m in self.layers:
            _check_gpu(m.weight_mu, m.weight_log_sigma, m.bias_mu, m.bias_log_sigma)
        self.counter.add_(1)
        params = [p for m in self.layers for p in (m.weight_mu, m.weight_log_sigma, m.bias_mu, m.bias_log_sigma)]
        return _BayesSampleFn.apply(self, *params)


# ------------------------------------------------------------------------------------------------------------------------------------
# inference: Monte-Carlo mean and std
# ------------------------------------------------------------------------------------------------------------------------------------
def _mc_args(mlp, x, S, P, ldx, seed, epilogue, y, eps_out=None):
    l1, l2 = mlp.lin1, mlp.lin2
    a = _cabi.BayesMcArgs()
    a.S, a.rows_per_sample, a.K, a.H, a.N, a.x, a.ldx = S, P, l1.in_features, l1.out_features, l2.out_features, x.data_ptr(), ldx
    a.w1_mu, a.w1_ls, a.b1_mu, a.b1_ls = (_ptr(t) for t in (l1.weight_mu, l1.weight_log_sigma, l1.bias_mu, l1.bias_log_sigma))
    a.ln_g, a.ln_b, a.ln_eps, a.slope = mlp.norm.weight.data_ptr(), mlp.norm.bias.data_ptr(), float(mlp.norm.eps), float(mlp.relu.negative_slope)
    a.w2_mu, a.w2_ls, a.b2_mu, a.b2_ls = (_ptr(t) for t in (l2.weight_mu, l2.weight_log_sigma, l2.bias_mu, l2.bias_log_sigma))
    a.seed, a.epilogue, a.y, a.eps_out = seed, epilogue, y.data_ptr(), _ptr(eps_out)
    return a


def _launch_mc(lib, a, dev):
    with torch.cuda.device(dev):
        rc = lib.ops_bayes_mlp_mc_f32(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_bayes_mlp_mc_f32")


def _check_mc_shapes(S: int, blocks) -> None:
    """The limits of ops_bayes_mlp_mc_f32 (one lin1 tile and 32 input rows, or one lin2 tile and 32 hidden rows, in LDS; S on grid.y),
    checked before anything is allocated or launched: the C call would only return OPS_AMD_ERR_UNSUPPORTED."""
    if S > 65535:
        raise NotImplementedError(f"n_samples {S} exceeds the Monte-Carlo kernels' limit of 65535 samples per call")
    for name, mlp in blocks:
        K, H = mlp.lin1.in_features, mlp.lin1.out_features
        for what, v, lim in (("input width K", K, _cabi.BAYES_MC_MAX_K), ("hidden width H", H, _cabi.BAYES_MC_MAX_H),
                             ("K + H", K + H, _cabi.BAYES_MC_MAX_KH)):
            if v > lim:
                raise NotImplementedError(f"{name}: {what} = {v} exceeds the Monte-Carlo kernels' limit of {lim} "
                                          f"(K = feat_dim = {K}, H = {H}; K <= {_cabi.BAYES_MC_MAX_K}, H <= {_cabi.BAYES_MC_MAX_H}, "
                                          f"K + H <= {_cabi.BAYES_MC_MAX_KH})")


def mc_seeds(seed: int):
    """(diffusion block, head block) stream seeds of `predict_with_uncertainty(seed=seed)`."""
    return _mix(int(seed) * 2 + 1), _mix(int(seed) * 2 + 2)


@torch.no_grad()
def predict_with_uncertainty(model, X: torch.Tensor, n_samples: int = 50, seed: int = 0, scaler=None, max_rows: Optional[int] = None,
                             return_draws: bool = False):
    """Mean and std (ddof = 0) over `n_samples` stochastic forwards of a BTFD / BTFDM `model` (eval mode: dropout off; the diffusion draws
    and the Bayesian weights stay random) for X [B, n_cases, feat_dim] -> (mean, std), each [B, n_elem] float32 on X's device.
    scaler: sklearn StandardScaler-like (`scale_`, `mean_`) or a pair (scale, center): mean * scale + center, std * scale.
    max_rows: bound on the encoder's rows per call, S * chunk * (n_cases + 1); the batch is processed in chunks (same draws, same result).
    return_draws: also return {"t", "xeps", "w_diff", "w_head"} -- every sample's diffusion and weight draws (tests replay them)."""
    lib = _cabi.load()           # raises without the HIP library: there is no CPU path
    if not X.is_cuda:
        raise RuntimeError("predict_with_uncertainty runs on the GPU only (csrc/bayes_mlp.hip); move the model and X to a HIP device")
    if model.training:
        raise RuntimeError("predict_with_uncertainty expects model.eval() (the reference's get_bnn_output_stats switches dropout off)")
    S = int(n_samples)
    B, Nc, d = X.shape
    if S < 1 or Nc != model.n_cases or d != model.feat_dim:
        raise ValueError(f"X {tuple(X.shape)} / n_samples {S} do not fit the model (n_cases {model.n_cases}, feat_dim {model.feat_dim})")
    dm, head = model.diffusion.mlp, model.bnn_output
    _check_mc_shapes(S, (("diffusion block", dm), ("output head", head)))
    dev = X.device
    X = X.float().contiguous()
    for p in model.parameters():
        _check_gpu(p.data)
    n_elem = head.lin2.out_features
    sd, sh = mc_seeds(seed)
    seqs = S * (Nc + 1)
    chunk = B if max_rows is None else max(1, min(B, int(max_rows) // seqs))
    pe = model.pos_encoder.pe[0].float().contiguous()
    cls = model.cls_token.reshape(-1).contiguous()
    acp = model.diffusion._acp.float().contiguous()
    scale = center = None
    if scaler is not None:
        sc, ce = (scaler.scale_, scaler.mean_) if hasattr(scaler, "scale_") else scaler
        scale = torch.as_tensor(sc, dtype=torch.float32, device=dev).contiguous()
        center = None if ce is None else torch.as_tensor(ce, dtype=torch.float32, device=dev).contiguous()
    out_scale = None if model.output_scales is None else model.output_scales.detach().contiguous()
    mean = torch.empty(B, n_elem, dtype=torch.float32, device=dev)
    std = torch.empty_like(mean)
    draws = None
    if return_draws:
        nw = lambda m: m.lin1.out_features * m.lin1.in_features + m.lin1.out_features + m.lin2.out_features * m.lin2.in_features + m.lin2.out_features
        draws = {"t": torch.empty(S, B, Nc, dtype=torch.int64, device=dev), "xeps": torch.empty(S, B, Nc, d, device=dev),
                 "w_diff": torch.empty(S, nw(dm), device=dev), "w_head": torch.empty(S, nw(head), device=dev)}
    stream = torch.cuda.current_stream(dev).cuda_stream
    for b0 in range(0, B, chunk):
        bc = min(chunk, B - b0)
        # 1. diffusion block: draws, MLP, denoise, [CLS], positional encoding -> z [S * bc, Nc + 1, d]
        z = torch.empty(S * bc, Nc + 1, d, dtype=torch.float32, device=dev)
        t_out = torch.empty(S, bc, Nc, dtype=torch.int64, device=dev) if return_draws else None
        x_out = torch.empty(S, bc, Nc, d, device=dev) if return_draws else None
        h_ws = torch.empty(S * bc * Nc, dm.lin1.out_features, dtype=torch.float32, device=dev)
        xn_ws = torch.empty(S * bc * Nc, d + 2, dtype=torch.float32, device=dev)
        a = _mc_args(dm, X[b0:b0 + bc], S, bc * Nc, d, sd, _cabi.BAYES_MC_DIFFUSION, z, draws["w_diff"] if (return_draws and b0 == 0) else None)
        a.Nc, a.T, a.acp, a.row_base, a.cls, a.pe = Nc, int(model.diffusion.T), acp.data_ptr(), b0 * Nc, cls.data_ptr(), pe.data_ptr()
        a.t_out, a.xeps_out, a.h_ws, a.xn_ws = _ptr(t_out), _ptr(x_out), h_ws.data_ptr(), xn_ws.data_ptr()
        _launch_mc(lib, a, dev)
        # 2. ONE encoder pass over all S * bc sequences
        enc = model.transformer_encoder(z).float().contiguous()
        # 3. head block on the [CLS] rows -> preds [S, bc, n_elem]
        preds = torch.empty(S, bc, n_elem, dtype=torch.float32, device=dev)
        a = _mc_args(head, enc, S, bc, (Nc + 1) * d, sh, _cabi.BAYES_MC_HEAD, preds, draws["w_head"] if (return_draws and b0 == 0) else None)
        del h_ws, xn_ws
        h_ws = torch.empty(S * bc, head.lin1.out_features, dtype=torch.float32, device=dev)
        a.out_scale, a.h_ws = _ptr(out_scale), h_ws.data_ptr()
        _launch_mc(lib, a, dev)
        # 4. moments (+ un-standardisation)
        mc, sc_ = mean[b0:b0 + bc], std[b0:b0 + bc]
        with torch.cuda.device(dev):
            rc = lib.ops_mc_moments_f32(S, bc * n_elem, n_elem, preds.data_ptr(), _ptr(scale), _ptr(center), mc.data_ptr(), sc_.data_ptr(), stream)
        _cabi.check(rc, "ops_mc_moments_f32")
        if return_draws:
            draws["t"][:, b0:b0 + bc] = t_out
            draws["xeps"][:, b0:b0 + bc] = x_out
    return (mean, std, draws) if return_draws else (mean, std)


def split_draws(model, w: torch.Tensor, block: str) -> list:
    """One sample's exported weight draws of `block` ("diffusion" | "head") -> [w1_eps, b1_eps, w2_eps, b2_eps] in the layers' shapes."""
    mlp = model.diffusion.mlp if block == "diffusion" else model.bnn_output
    out, o = [], 0
    for m in (mlp.lin1, mlp.lin2):
        for shape in ((m.out_features, m.in_features), (m.out_features,)):
            n = 1
            for s_ in shape:
                n *= s_
            out.append(w[o:o + n].reshape(shape))
            o += n
    return out


def set_frozen_draws(layers: Sequence[BayesLinear], eps: Optional[Sequence[torch.Tensor]]) -> None:
    """Pin the layers' draws (torchbnn's frozen state): eps = [w_eps, b_eps] per layer, flattened; None: fresh draws again."""
    for i, m in enumerate(layers):
        m.weight_eps = None if eps is None else eps[2 * i]
        m.bias_eps = None if eps is None else eps[2 * i + 1]
