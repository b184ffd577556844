"""BTFD / BTFDM on the MI355X: the sampling and fold launches against the framework's BayesLinear, the training loop on the HIP path,
and `predict_with_uncertainty` against the reference's loop of stochastic forwards replayed with the kernels' own draws."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from openpystruct_amd import bayes, dataprep, train  # noqa: E402
from openpystruct_amd.surrogates import BayesianTransformerWithDiffusion, BayesLinear  # noqa: E402
from tests.helpers import framework_loop  # noqa: E402


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")


def _layers(seed=0, shapes=((512, 120), (120, 512), (100, 512))):
    torch.manual_seed(seed)
    ls = [BayesLinear(0.0, 0.01, i, o).cuda() for o, i in shapes]
    with torch.no_grad():
        for m in ls:        # varied sigmas: exp(ls) is not one constant
            m.weight_log_sigma.add_(torch.randn_like(m.weight_log_sigma) * 0.5)
            m.bias_log_sigma.add_(torch.randn_like(m.bias_log_sigma) * 0.5)
    return ls


class _Holder(torch.nn.Module):
    def __init__(self, ls):
        super().__init__()
        self.ls = torch.nn.ModuleList(ls)

    def bayes_layers(self):
        return list(self.ls)


def _sampler(ls, seed=5, kl_scale=0.0, replay=None, mode=None):
    s = bayes.BayesSampler(_Holder(ls), seed=seed, kl_scale=kl_scale)
    if replay is not None:
        s.replay, s.mode = replay, mode
    return s


def _eps_like(ls):
    return [[torch.empty_like(m.weight_mu), torch.empty_like(m.bias_mu)] for m in ls]


def test_sampling_exports_its_draws_and_reproduces_them():
    ls = _layers()
    eps = _eps_like(ls)
    s = _sampler(ls, replay=eps, mode="write")
    with torch.no_grad():
        wb = s()
    torch.cuda.synchronize()
    for i, m in enumerate(ls):
        w, b = wb[2 * i], wb[2 * i + 1]
        want_w = m.weight_mu + torch.exp(m.weight_log_sigma) * eps[i][0]
        want_b = m.bias_mu + torch.exp(m.bias_log_sigma) * eps[i][1]
        # the same float32 operations; the device expf and the framework's exp may round one ulp apart
        assert torch.equal(w, want_w) or float(((w - want_w).abs() / want_w.abs().clamp_min(1e-30)).max()) <= 2.4e-7
        assert torch.equal(b, want_b) or float(((b - want_b).abs() / want_b.abs().clamp_min(1e-30)).max()) <= 2.4e-7
    # same seed + counter: the same draws; the next counter: new draws
    s2 = _sampler(ls, replay=_eps_like(ls), mode="write")
    with torch.no_grad():
        s2()
        assert all(torch.equal(a, c) for pa, pc in zip(eps, s2.replay) for a, c in zip(pa, pc))
        s2()
    assert not torch.equal(s2.replay[0][0], eps[0][0])
    # replay: read mode gives back the same weights
    s3 = _sampler(ls, seed=99, replay=eps, mode="read")
    with torch.no_grad():
        wb3 = s3()
    assert all(torch.equal(a, c) for a, c in zip(wb, wb3))


@pytest.mark.stochastic
def test_sampling_draws_are_standard_normal():
    ls = _layers(1, shapes=((1024, 512), (512, 1024), (256, 256)))
    s = _sampler(ls, seed=3, replay=_eps_like(ls), mode="write")
    with torch.no_grad():
        s()
    e = torch.cat([t.reshape(-1) for pair in s.replay for t in pair]).double()
    n = e.numel()
    assert n > 1_000_000
    # mean: sd 1 / sqrt(n); variance: sd sqrt(2 / n); bounds at 6 sd
    assert abs(float(e.mean())) < 6 / math.sqrt(n)
    assert abs(float(e.var()) - 1.0) < 6 * math.sqrt(2 / n)
    assert abs(float((e ** 4).mean()) - 3.0) < 6 * math.sqrt(96 / n)        # kurtosis of a normal: 3 (Var of x^4 = 96)


def test_fold_uses_the_draws_of_its_own_forward():
    """Two forwards before one backward: each backward folds with the eps of ITS forward (the counter is kept per call)."""
    ls = _layers(4, shapes=((64, 32), (16, 64)))
    s = _sampler(ls, seed=8)
    x = torch.randn(8, 32, device="cuda")
    wb1 = s()
    wb2 = s()                                   # advances the counter before the first backward
    y1 = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, wb1[0], wb1[1])), wb1[2], wb1[3])
    (y1 ** 2).sum().backward()
    hip = [p.grad.clone() for m in ls for p in (m.weight_mu, m.weight_log_sigma, m.bias_mu, m.bias_log_sigma)]
    for m in ls:
        for p in m.parameters():
            p.grad = None
    # the first call's eps, recovered from its weights: eps = (W - mu) / exp(ls)
    eps = []
    for i, m in enumerate(ls):
        eps += [((wb1[2 * i] - m.weight_mu) / torch.exp(m.weight_log_sigma)).detach(),
                ((wb1[2 * i + 1] - m.bias_mu) / torch.exp(m.bias_log_sigma)).detach()]
    bayes.set_frozen_draws(ls, eps)
    (ls[1](torch.relu(ls[0](x))) ** 2).sum().backward()
    bayes.set_frozen_draws(ls, None)
    ref = [p.grad for m in ls for p in (m.weight_mu, m.weight_log_sigma, m.bias_mu, m.bias_log_sigma)]
    for a, b in zip(hip, ref):
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-5 * float(b.abs().max()) + 1e-12)
    del wb2


@pytest.mark.parametrize("kl_scale", [0.0, 1e-3])
def test_fold_equals_autograd_through_the_framework_layer(kl_scale):
    ls = _layers(2, shapes=((512, 120), (120, 512), (100, 120)))
    eps = _eps_like(ls)
    s = _sampler(ls, kl_scale=kl_scale, replay=eps, mode="write")
    x = torch.randn(64, 120, device="cuda")
    # HIP: sampled weights, the same products, fold
    wb = s()
    y = torch.nn.functional.linear(x, wb[0], wb[1])
    y = torch.nn.functional.linear(torch.relu(y), wb[2], wb[3])
    loss = (y ** 2).mean() + torch.nn.functional.linear(torch.relu(y), wb[4], wb[5]).sum() * 1e-3
    loss.backward()
    hip = [p.grad.clone() for m in ls for p in (m.weight_mu, m.weight_log_sigma, m.bias_mu, m.bias_log_sigma)]
    for m in ls:
        for p in m.parameters():
            p.grad = None
    # framework: frozen draws, autograd (+ the KL term through autograd)
    bayes.set_frozen_draws(ls, [t for pair in eps for t in pair])
    y = ls[1](torch.relu(ls[0](x)))
    loss = (y ** 2).mean() + ls[2](torch.relu(y)).sum() * 1e-3
    if kl_scale:
        loss = loss + kl_scale * bayes.bayesian_kl(_Holder(ls))
    loss.backward()
    bayes.set_frozen_draws(ls, None)
    ref = [p.grad for m in ls for p in (m.weight_mu, m.weight_log_sigma, m.bias_mu, m.bias_log_sigma)]
    for a, b in zip(hip, ref):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6 * float(b.abs().max()) + 1e-12)


def _model(n_cases, output_scales, seed=0, layers=4):
    torch.manual_seed(seed)
    m = BayesianTransformerWithDiffusion(n_cases, 120, 100, 512, layers, 24, 512, 0.1, 512, 512, 512, output_scales=output_scales).cuda()
    with torch.no_grad():
        m.cls_token.normal_(std=0.1)
        if output_scales:
            m.output_scales.uniform_(0.5, 1.5)
        for l in m.bayes_layers():        # wider posteriors than the prior's 0.01: the samples must differ visibly
            l.weight_log_sigma.fill_(math.log(0.05))
            l.bias_log_sigma.fill_(math.log(0.05))
    return m


def test_one_training_step_on_the_hip_path_matches_the_framework_modules():
    """One BTFD step: forward + backward with the sampling / fold launches (replayed draws) == the framework modules with the same
    weight and diffusion draws, under the loop's bf16 autocast (the TFD tests' bf16 tolerances)."""
    m = _model(6, False, seed=3, layers=2).train()
    for mod in m.modules():      # dropout masks are not replayable between the two runs
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    x = torch.randn(32, 6, 120, device="cuda")
    draws = (torch.randint(0, 512, (32, 6), device="cuda"), torch.randn(32, 6, 120, device="cuda"))
    eps = _eps_like(m.bayes_layers())
    s = bayes.BayesSampler(m, seed=1)
    s.replay, s.mode = eps, "write"
    m.bayes_sampler = s
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x, draws)
    (y.float() ** 2).mean().backward()
    hip_y = y.float().detach()
    hip_g = [p.grad.clone() for p in m.parameters()]
    m.zero_grad(set_to_none=True)
    m.bayes_sampler = None
    bayes.set_frozen_draws(m.bayes_layers(), [t for pair in eps for t in pair])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x, draws)
    (y.float() ** 2).mean().backward()
    bayes.set_frozen_draws(m.bayes_layers(), None)
    y = y.float().detach()
    assert torch.allclose(hip_y, y, rtol=2e-2, atol=2e-2 * float(y.abs().max()))
    for a, p in zip(hip_g, m.parameters()):
        b = p.grad
        assert torch.allclose(a, b, rtol=5e-2, atol=5e-2 * float(b.abs().max()) + 1e-12)


@pytest.mark.parametrize("kind", ["btfd", "btfdm"])
def test_train_surrogate_end_to_end(kind):
    from openpystruct_amd import sizing
    cfg = (train.BtfdConfig if kind == "btfd" else train.BtfdmConfig)(batch_size=32, patience=20)
    rec = sizing.generate_dataset(960, sizing.SizingConfig(max_e=30), "cuda", seed=11)
    d = dataprep.prepare(rec, kind="tfd", n_cases=cfg.n_cases, c=cfg.c, nheads=cfg.num_heads, seed=0, device="cuda", refit_val_scalers=False)
    assert d.feat_dim % 24 == 0
    out = train.train_surrogate(kind, d, cfg, device="cuda", max_epochs=4)
    h = out["history"]
    assert np.isfinite(h["train"]).all() and np.isfinite(h["val"]).all()
    assert h["train"][-1] < h["train"][0], h["train"]
    assert out["model"].bayes_sampler is not None and int(out["model"].bayes_sampler.counter) > 0


@pytest.mark.parametrize("B,n_cases", [(1, 6), (7, 8), (512, 6), (1, 8), (512, 8)])
def test_predict_with_uncertainty_equals_the_replayed_loop(B, n_cases):
    S = 50
    m = _model(n_cases, output_scales=n_cases == 8, seed=B).eval()
    X = torch.randn(B, n_cases, 120, device="cuda")
    mean, std, draws = bayes.predict_with_uncertainty(m, X, n_samples=S, seed=4, return_draws=True)
    P = framework_loop(m, X, draws)
    rm, rs = P.mean(0), P.std(0, unbiased=False)
    scale_m, scale_s = float(rm.abs().max()), float(rs.max())
    em = float((mean.double() - rm).abs().max()) / scale_m
    es = float((std.double() - rs).abs().max()) / scale_s
    print(f"B={B} n_cases={n_cases}: max |mean - loop| / max|mean| = {em:.2e}, max |std - loop| / max std = {es:.2e}")
    assert em < 2e-5 and es < 1e-4
    assert float(rs.min()) > 0
    # un-standardisation: mean * scale + center, std * scale
    sc = torch.rand(100, device="cuda") + 0.5
    ce = torch.randn(100, device="cuda")
    m2, s2 = bayes.predict_with_uncertainty(m, X, n_samples=S, seed=4, scaler=(sc, ce))
    torch.testing.assert_close(m2, mean * sc + ce, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(s2, std * sc, rtol=1e-6, atol=1e-7)


def test_encoder_runs_once_per_chunk_and_chunking_changes_nothing():
    m = _model(6, False, seed=9).eval()
    X = torch.randn(37, 6, 120, device="cuda")
    calls = []
    inner = m.transformer_encoder.forward

    def counting(*a, **k):
        calls.append(a[0].shape[0])
        return inner(*a, **k)

    m.transformer_encoder.forward = counting
    mean, std = bayes.predict_with_uncertainty(m, X, n_samples=50, seed=2)
    assert calls == [50 * 37]                       # ONE encoder pass over S * B sequences, not S passes
    calls.clear()
    mc, sc = bayes.predict_with_uncertainty(m, X, n_samples=50, seed=2, max_rows=50 * 7 * 10)   # chunks of 10 samples
    assert calls == [500, 500, 500, 350]
    torch.testing.assert_close(mc, mean, rtol=1e-5, atol=1e-5 * float(mean.abs().max()))
    torch.testing.assert_close(sc, std, rtol=1e-4, atol=1e-5 * float(std.max()))


@pytest.mark.stochastic
def test_statistics_agree_with_independent_framework_draws():
    """S = 4000: the kernels' mean and std against S framework forwards with torch's own draws (independent streams)."""
    S = 4000
    m = _model(6, False, seed=5).eval()
    X = torch.randn(1, 6, 120, device="cuda")
    mean, std = bayes.predict_with_uncertainty(m, X, n_samples=S, seed=11)
    with torch.no_grad():
        P = torch.stack([m(X).double() for _ in range(S)])
    rm, rs = P.mean(0), P.std(0, unbiased=False)
    # two independent estimates: their mean difference has sd sigma * sqrt(2 / S); the std's relative sd is ~ sqrt(1 / (2S)) per
    # estimate (normal-ish outputs), sqrt(1 / S) for the difference; 6 sd bounds per element (200 elements)
    dm = ((mean.double() - rm).abs() / (rs * math.sqrt(2 / S))).max()
    ds = ((std.double() - rs).abs() / (rs * math.sqrt(1 / S))).max()
    print(f"S={S}: max standardised mean difference {float(dm):.2f}, std difference {float(ds):.2f}")
    assert float(dm) < 6 and float(ds) < 8
