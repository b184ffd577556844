"""BTFD / BTFDM (Bayesian Transformer-Diffusion surrogates) without a GPU: the torchbnn-style layer, the models' state dicts, the KL
closed form, the CPU training loop, and the argument checks of the four HIP entry points (refused before any HIP call)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from openpystruct_amd import _cabi, bayes, build, dataprep, train
from openpystruct_amd.surrogates import BayesianTransformerWithDiffusion, BayesLinear


def test_bayes_linear_parameters_and_initialisation():
    torch.manual_seed(0)
    m = BayesLinear(0.0, 0.01, 400, 300)
    assert [n for n, _ in m.named_parameters()] == ["weight_mu", "weight_log_sigma", "bias_mu", "bias_log_sigma"]
    assert set(m.state_dict()) == {"weight_mu", "weight_log_sigma", "bias_mu", "bias_log_sigma"}    # the eps buffers never are
    assert not hasattr(m, "kl_loss")            # the reference's KL sum (BTFD:730) must find nothing, as with torchbnn
    b = 1 / math.sqrt(400)
    w = m.weight_mu.detach()
    assert float(w.abs().max()) <= b and abs(float(w.mean())) < 0.02 * b
    assert abs(float(w.var()) - b * b / 3) < 0.02 * b * b / 3          # U(-b, b): variance b^2 / 3
    assert torch.all(m.weight_log_sigma == math.log(0.01)) and torch.all(m.bias_log_sigma == math.log(0.01))
    assert float(m.bias_mu.abs().max()) <= b


def test_bayes_linear_draws_every_call_and_frozen_draws_replay():
    torch.manual_seed(1)
    m = BayesLinear(0.0, 0.1, 8, 5).eval()
    x = torch.randn(3, 8)
    assert not torch.equal(m(x), m(x))          # eval mode draws too
    we, be = torch.randn(5, 8), torch.randn(5)
    bayes.set_frozen_draws([m], [we, be])
    y = m(x)
    ref = x @ (m.weight_mu + torch.exp(m.weight_log_sigma) * we).T + (m.bias_mu + torch.exp(m.bias_log_sigma) * be)
    torch.testing.assert_close(y, ref)
    assert torch.equal(y, m(x))
    assert set(m.state_dict()) == {"weight_mu", "weight_log_sigma", "bias_mu", "bias_log_sigma"}    # frozen: still loads strictly
    bayes.set_frozen_draws([m], None)


def _ref_keys(n_layers, output_scales):
    """The reference model's state-dict keys and shapes (BTFD:503-584, d = 120, hidden 512, ff 512, n_elem 100, 24 heads)."""
    d, h, ff, ne = 120, 512, 512, 100
    k = {"cls_token": (1, 1, d), "pos_encoder.pe": (1, 512, d)}
    for blk, (i, o) in (("diffusion.mlp", (d, d)), ("bnn_output", (d, ne))):
        k.update({f"{blk}.lin1.weight_mu": (h, i), f"{blk}.lin1.weight_log_sigma": (h, i), f"{blk}.lin1.bias_mu": (h,),
                  f"{blk}.lin1.bias_log_sigma": (h,), f"{blk}.lin2.weight_mu": (o, h), f"{blk}.lin2.weight_log_sigma": (o, h),
                  f"{blk}.lin2.bias_mu": (o,), f"{blk}.lin2.bias_log_sigma": (o,), f"{blk}.norm.weight": (h,), f"{blk}.norm.bias": (h,)})
    for L in range(n_layers):
        p = f"transformer_encoder.layers.{L}."
        k.update({p + "self_attn.in_proj_weight": (3 * d, d), p + "self_attn.in_proj_bias": (3 * d,), p + "self_attn.out_proj.weight": (d, d),
                  p + "self_attn.out_proj.bias": (d,), p + "linear1.weight": (ff, d), p + "linear1.bias": (ff,), p + "linear2.weight": (d, ff),
                  p + "linear2.bias": (d,), p + "norm1.weight": (d,), p + "norm1.bias": (d,), p + "norm2.weight": (d,), p + "norm2.bias": (d,)})
    if output_scales:
        k["output_scales"] = (ne,)
    return k


@pytest.mark.parametrize("kind", ["btfd", "btfdm"])
def test_state_dict_keys_and_shapes_equal_the_reference(kind):
    cfg = train.BtfdConfig() if kind == "btfd" else train.BtfdmConfig()
    m = BayesianTransformerWithDiffusion(cfg.n_cases, 120, cfg.nelem, cfg.hidden_units, cfg.num_transformer_layers, cfg.num_heads,
                                         cfg.dim_feedforward, cfg.dropout_rate, cfg.max_len, cfg.diffusion_hidden_dim, cfg.diffusion_T,
                                         output_scales=kind == "btfdm")
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == _ref_keys(4, kind == "btfdm")
    assert torch.all(m.cls_token == 0)          # BTFD:537: zeros (the TFD restatement draws N(0, 0.02))
    m.load_state_dict(m.state_dict(), strict=True)


def test_configs_are_the_scripts_values():
    a, b = train.BtfdConfig(), train.BtfdmConfig()
    assert (a.n_cases, a.dropout_rate, a.c, a.hidden_units, a.num_heads, a.dim_feedforward, a.num_transformer_layers) == (6, 0.1, 0.5, 512, 24, 512, 4)
    assert (a.learning_rate, a.weight_decay, a.gamma, a.gamma_noise, a.bnn_kl_scale, a.kl) == (3e-4, 1e-6, 0.99, 0.95, 1e-6, "none")
    assert (b.n_cases, b.dropout_rate, b.c) == (8, 0.01, 1.0)


def test_model_eval_mode_is_stochastic_and_replayable():
    torch.manual_seed(2)
    m = BayesianTransformerWithDiffusion(6, 24, 10, 32, 1, 4, 32, 0.1, 16, 32, 512, output_scales=True).eval()
    x = torch.randn(3, 6, 24)
    with torch.no_grad():
        assert not torch.equal(m(x), m(x))
        draws = (torch.randint(0, 512, (3, 6)), torch.randn(3, 6, 24))
        eps = [torch.randn_like(p) for l in m.bayes_layers() for p in (l.weight_mu, l.bias_mu)]
        bayes.set_frozen_draws(m.bayes_layers(), eps)
        assert torch.equal(m(x, draws), m(x, draws))
        bayes.set_frozen_draws(m.bayes_layers(), None)


def test_bayesian_kl_matches_the_closed_form():
    torch.manual_seed(3)
    m = BayesianTransformerWithDiffusion(6, 24, 10, 32, 1, 4, 32, 0.1, 16, 32, 512)
    with torch.no_grad():
        for l in m.bayes_layers():
            l.weight_log_sigma.add_(torch.randn_like(l.weight_log_sigma) * 0.3)
    want = 0.0
    for l in m.bayes_layers():
        for mu, ls in ((l.weight_mu, l.weight_log_sigma), (l.bias_mu, l.bias_log_sigma)):
            q = torch.distributions.Normal(mu.double(), torch.exp(ls.double()))
            p = torch.distributions.Normal(torch.zeros_like(mu.double()), torch.full_like(mu.double(), 0.01))
            want += float(torch.distributions.kl_divergence(q, p).sum())
    got = float(bayes.bayesian_kl(m))
    assert abs(got - want) <= 1e-5 * abs(want)
    kl = bayes.bayesian_kl(m)
    kl.backward()
    l = m.bayes_layers()[0]
    torch.testing.assert_close(l.weight_mu.grad, l.weight_mu.detach() / 1e-4, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(l.weight_log_sigma.grad, torch.exp(2 * l.weight_log_sigma.detach()) / 1e-4 - 1, rtol=1e-4, atol=1e-4)


def _small_cfg(kind, **kw):
    c = (train.BtfdConfig if kind == "btfd" else train.BtfdmConfig)(batch_size=8, patience=3, hidden_units=32, diffusion_hidden_dim=32,
                                                                      dim_feedforward=32, num_transformer_layers=1, **kw)
    return c


@pytest.mark.parametrize("kind,kl", [("btfd", "none"), ("btfdm", "none"), ("btfd", "gaussian")])
def test_cpu_training_loop_runs(kind, kl):
    from tests.test_surrogates import _fake_records
    cfg = _small_cfg(kind, kl=kl)
    d = dataprep.prepare(_fake_records(160, seed=4), kind="tfd", n_cases=cfg.n_cases, c=cfg.c, nheads=cfg.num_heads, seed=1,
                         refit_val_scalers=False)
    assert d.feat_dim % 24 == 0 and d.X_train.shape[1] == cfg.n_cases
    out = train.train_surrogate(kind, d, cfg, device="cpu", autocast_dtype=None, max_epochs=3)
    h = out["history"]
    assert np.isfinite(h["train"]).all() and np.isfinite(h["val"]).all()
    assert isinstance(out["model"], BayesianTransformerWithDiffusion) and (out["model"].output_scales is not None) == (kind == "btfdm")
    if kl == "gaussian":
        assert h["val"][0] > 1e-6 * 0.5 * float(bayes.bayesian_kl(out["model"]))    # the KL term is in the validation loss


def test_unknown_kl_mode_is_refused():
    from tests.test_surrogates import _fake_records
    d = dataprep.prepare(_fake_records(60, seed=5), kind="tfd", nheads=24, seed=1, refit_val_scalers=False)
    with pytest.raises(ValueError):
        train.train_surrogate("btfd", d, _small_cfg("btfd", kl="l2"), device="cpu", autocast_dtype=None, max_epochs=1)


def test_predict_with_uncertainty_has_no_cpu_path():
    m = BayesianTransformerWithDiffusion(6, 24, 10, 32, 1, 4, 32, 0.1, 16, 32, 512).eval()
    with pytest.raises(RuntimeError):
        bayes.predict_with_uncertainty(m, torch.randn(2, 6, 24), n_samples=4)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _cabi.load()


def test_argument_validation_without_gpu(lib):
    z = ctypes.c_void_p(0)
    L = (_cabi.BayesLayer * 2)()
    ok_ptr = ctypes.c_void_p(16)        # never dereferenced: every call below is refused before a launch
    for e in L:
        e.out_f, e.in_f = 4, 3
        e.w_mu = e.w_ls = e.b_mu = e.b_ls = e.w = e.b = ok_ptr
        e.dw = e.db = e.d_wmu = e.d_wls = e.d_bmu = e.d_bls = ok_ptr
    EINVAL = _cabi.ERR_INVALID_ARG
    assert lib.ops_bayes_sample_f32(0, L, 1, ok_ptr, 0, z) == EINVAL                       # no layer
    assert lib.ops_bayes_sample_f32(9, L, 1, ok_ptr, 0, z) == EINVAL                       # more than OPS_BAYES_MAX_LAYERS
    assert lib.ops_bayes_sample_f32(2, L, 1, z, 0, z) == EINVAL                            # no counter
    assert lib.ops_bayes_sample_f32(2, L, 1, ok_ptr, 1, z) == EINVAL                       # write mode without eps buffers
    assert lib.ops_bayes_sample_f32(2, L, 1, ok_ptr, 3, z) == EINVAL                       # unknown mode
    assert lib.ops_bayes_sample_f32(2, None, 1, ok_ptr, 0, z) == EINVAL
    L[1].in_f = 0
    assert lib.ops_bayes_sample_f32(2, L, 1, ok_ptr, 0, z) == EINVAL
    L[1].in_f = 3
    assert lib.ops_bayes_grad_fold_f32(2, L, 1, ok_ptr, 1, 0.0, 0.0, 0.01, z) == EINVAL     # the fold only draws or reads
    assert lib.ops_bayes_grad_fold_f32(2, L, 1, ok_ptr, 0, 1e-6, 0.0, 0.0, z) == EINVAL     # KL with prior sigma 0
    assert lib.ops_bayes_grad_fold_f32(2, L, 1, ok_ptr, 0, -1.0, 0.0, 0.01, z) == EINVAL
    L[0].dw = None
    assert lib.ops_bayes_grad_fold_f32(2, L, 1, ok_ptr, 0, 0.0, 0.0, 0.01, z) == EINVAL
    a = _cabi.BayesMcArgs()
    assert lib.ops_bayes_mlp_mc_f32(None, z) == EINVAL
    assert lib.ops_bayes_mlp_mc_f32(ctypes.byref(a), z) == EINVAL                           # all zero
    a.S, a.rows_per_sample, a.K, a.H, a.N, a.ldx, a.ln_eps = 2, 6, 120, 512, 120, 120, 1e-5
    for f in ("x", "w1_mu", "w1_ls", "b1_mu", "b1_ls", "ln_g", "ln_b", "w2_mu", "w2_ls", "b2_mu", "b2_ls", "y", "h_ws"):
        setattr(a, f, 16)
    a.epilogue = _cabi.BAYES_MC_DIFFUSION
    a.Nc, a.T = 6, 512
    assert lib.ops_bayes_mlp_mc_f32(ctypes.byref(a), z) == EINVAL                           # diffusion epilogue without acp / cls / pe
    a.epilogue = 7
    assert lib.ops_bayes_mlp_mc_f32(ctypes.byref(a), z) == EINVAL
    a.epilogue, a.h_ws = _cabi.BAYES_MC_HEAD, None
    assert lib.ops_bayes_mlp_mc_f32(ctypes.byref(a), z) == EINVAL                           # no workspace
    a.h_ws = 16
    a.K, a.ldx = 300, 300
    assert lib.ops_bayes_mlp_mc_f32(ctypes.byref(a), z) == _cabi.ERR_UNSUPPORTED             # K beyond OPS_BAYES_MC_MAX_K
    a.K, a.ldx = 900, 900
    assert lib.ops_bayes_mlp_mc_f32(ctypes.byref(a), z) == _cabi.ERR_UNSUPPORTED             # K + H beyond OPS_BAYES_MC_MAX_KH
    a.ldx = 100
    assert lib.ops_bayes_mlp_mc_f32(ctypes.byref(a), z) == EINVAL                           # row stride below K
    assert lib.ops_mc_moments_f32(0, 100, 100, ok_ptr, None, None, ok_ptr, ok_ptr, z) == EINVAL
    assert lib.ops_mc_moments_f32(4, 150, 100, ok_ptr, None, None, ok_ptr, ok_ptr, z) == EINVAL   # M not a multiple of N
    assert lib.ops_mc_moments_f32(4, 100, 100, ok_ptr, None, ok_ptr, ok_ptr, ok_ptr, z) == EINVAL # center without scale
    assert lib.ops_mc_moments_f32(4, 100, 100, None, None, None, ok_ptr, ok_ptr, z) == EINVAL
