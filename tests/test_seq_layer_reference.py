"""tests/seq_layer_ref.py on the CPU: (1) the host tiling against pinn_fused.to_tiled; (2) the float32 evaluation of every launch
through the very protocols tests/test_gpu_seq_layer.py runs, whose largest constants are seq_layer_ref.CPU_CONST (the GPU bounds are
four times these), the no-rounding twin held to the reference with no slack, and the products' ceiling; (3) teeth: every wrong variant
in seq_layer_ref.BUGS violates the GPU bound or an exact condition on a case of the tables; (4) every stage reference of the
layer against float64 torch and its autograd on the stage's given inputs, so no hand-written derivative stands unchecked.
"""
import functools

import numpy as np
import pytest

from tests import seq_layer_ref as R

f32, f64 = np.float32, np.float64
_ids = lambda v: "-".join(map(str, v)).replace(" ", "").replace("(", "").replace(")", "")[:60] if isinstance(v, tuple) else str(v)      # noqa: E731


@functools.lru_cache(maxsize=None)
def _measured(kind, case, bug=()):
    proto, _ = R.PROTOCOLS[kind]
    return R.measure(proto(*case, R.CpuImpl(bug)))


def test_tiling_is_pinn_fused():
    torch = pytest.importorskip("torch")
    from openpystruct_amd import pinn_fused
    rng = np.random.default_rng(1)
    for N, K in ((24, 8), (17, 33), (136, 120), (384, 128)):
        w = rng.integers(1, 2 ** 15, (N, K)).astype(np.uint16)
        pad = np.zeros((R.ru(N, 16), R.ru(K, 32)), dtype=np.int64)
        pad[:N, :K] = w
        assert np.array_equal(R.tiled_weight(w), pinn_fused.to_tiled(torch.from_numpy(pad)).numpy().astype(np.uint16))
        assert np.array_equal(R.tiled_weight_t(w), R.tiled_weight(np.ascontiguousarray(w.T)))


@pytest.mark.parametrize("kind", list(R.PROTOCOLS))
def test_float32_evaluation_within_the_constants(kind):
    """No output of the float32 evaluation (nor of its twin without bf16 roundings, which is given no slack) exceeds CPU_CONST, and
    every exact condition holds."""
    worst = {}
    for case in R.PROTOCOLS[kind][1]:
        ratios, failed = _measured(kind, case)
        assert not failed, (case, failed)
        for n, e in ratios.items():
            worst[n] = max(worst.get(n, 0.0), e)
    for n in sorted(worst):
        print(f"{n:12s} measured {worst[n]:6.2f}   CPU_CONST {R.CPU_CONST[n]:5.2f}   GPU bound {R.bound_constant(n):6.2f}")
    over = {n: (e, R.CPU_CONST[n]) for n, e in worst.items() if e > R.CPU_CONST[n]}
    assert not over, over


def test_every_output_has_a_constant_and_products_stay_below_their_ceiling():
    seen = set()
    for kind, (_, cases) in R.PROTOCOLS.items():
        for case in cases:
            seen |= set(_measured(kind, case)[0])
    assert seen == set(R.CPU_CONST), seen ^ set(R.CPU_CONST)
    ks = {"d": [c[2] * c[3] for c in R.LAYER_CASES] + [c[2] for c in R.HEAD_CASES + R.FRONT_CASES],
          "hid": [c[4] for c in R.LAYER_CASES] + [c[3] for c in R.HEAD_CASES + R.FRONT_CASES]}
    for name, which in R.PRODUCTS.items():
        for K in ks[which]:
            assert R.bound_constant(name) < R.product_ceiling(K), (name, K)


@pytest.mark.parametrize("kind,bug", [(k, b) for k, bugs in R.BUGS.items() for b in bugs], ids=_ids)
def test_teeth(kind, bug):
    """The wrong variant of the float32 evaluation exceeds the GPU bound (4 x CPU_CONST) or breaks an exact condition on some case."""
    for case in R.PROTOCOLS[kind][1]:
        ratios, failed = _measured(kind, case, bug)
        if failed or any(e > R.bound_constant(n) for n, e in ratios.items()):
            return
    pytest.fail(f"{bug}: no case of the {kind} table notices")


def test_relu_gate_taken_from_h_is_no_different_launch():
    """"ReLU' taken from h instead of u" cannot have teeth in this launch: h > 0 exactly where the element was kept AND u > 0, and the
    dropout factor zeroes the gradient of every dropped element anyway -- the variant stores the same d_u, bit for bit, at every case."""
    for case, drop in R.PROTOCOLS["layer"][1]:
        a = R.layer_inputs(case, drop)
        sv = R.CpuImpl().layer_fwd(a)
        want, got = (R.store("lb.d_u", R.layer_bwd(a, sv, "both", False, f32, bug)["lb.d_u"][0]) for bug in ((), ("relu_from_h",)))
        assert np.array_equal(want, got)


@pytest.mark.parametrize("case,drop", [((7, 3, 2, 12, 40), "mixed"), ((3, 2, 4, 10, 16), "p01"), ((17, 1, 8, 1, 24), "off")], ids=_ids)
def test_layer_stage_references_against_autograd(case, drop):
    """Every stage of the float64 reference against float64 torch (softmax, F.layer_norm, relu, the same masks as multipliers) fed the
    stage's GIVEN inputs, forward and -- through autograd, so that no hand-written derivative stands unchecked -- backward."""
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    Bn, S, H, dh, ff = case
    d, T = H * dh, Bn * S
    a = R.layer_inputs(case, drop)
    p, seeds, call, eps = a["p"], a["seeds"], a["call"], float(f32(a["eps"]))
    t = lambda x, g=False: torch.tensor(np.asarray(x, dtype=f64), dtype=torch.float64, requires_grad=g)      # noqa: E731
    wide = lambda n: t(R.widen(n, sv[n]))      # noqa: E731
    W = {n: t(R.bf16_f64(a[n])) for n in ("W_in", "W_out", "W_1", "W_2", "b_in", "b_out", "b_1", "b_2")}
    rows = np.arange(T, dtype=np.uint64)
    mult = lambda j, N: t(R._keep(seeds[j], call, rows, N, p[j]) / (1.0 - p[j]))      # noqa: E731
    keep = R.sb._att_keep(Bn, S, H, p[0], seeds[0], call, None, 16 // S)

    def agree(name, ref, want, tol=1e-11):
        v, u = np.asarray(ref[0], dtype=f64), np.asarray(ref[1], dtype=f64)
        want = want.detach().numpy().reshape(v.shape)
        assert (np.abs(v - want) <= tol * np.maximum(u, np.abs(v).max())).all(), (name, float(np.abs(v - want).max()))

    def attention(qkv):
        q, k, v = (qkv.reshape(Bn, S, 3, H, dh)[:, :, n].permute(0, 2, 1, 3) for n in range(3))
        P = torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(dh), dim=-1) * t(keep / (1.0 - p[0]))
        return (P @ v).permute(0, 2, 1, 3).reshape(T, d)

    sv = {k: v for k, v in R.CpuImpl().layer_fwd(a).items() if k.startswith("lf.")}      # a representable state of the launch
    ref = R.layer_fwd(a, f64, (), sv)
    g1, be1, g2, be2 = (t(a[n], True) for n in ("gamma1", "beta1", "gamma2", "beta2"))
    z1s, z2s = t(sv["lf.z1"], True), t(sv["lf.z2"], True)
    y1, y2 = F.layer_norm(z1s, (d,), g1, be1, eps), F.layer_norm(z2s, (d,), g2, be2, eps)
    y1_given = (z1s - wide("lf.mean1")[:, None]) * wide("lf.rstd1")[:, None] * g1 + be1
    agree("qkv", ref["lf.qkv"], t(R.bf16_f64(R.bf16_bits(a["x32"]))) @ W["W_in"].T + W["b_in"])
    agree("ctx", ref["lf.ctx"], attention(wide("lf.qkv")))
    agree("z1", ref["lf.z1"], t(a["x32"]) + (wide("lf.ctx") @ W["W_out"].T + W["b_out"]) * mult(1, d))
    agree("y1", ref["lf.y1_16"], y1)
    agree("mean1", ref["lf.mean1"], z1s.mean(-1))
    agree("rstd1", ref["lf.rstd1"], 1 / torch.sqrt(z1s.var(-1, unbiased=False) + eps))
    agree("u", ref["lf.u"], wide("lf.y1_16") @ W["W_1"].T + W["b_1"])
    agree("h", ref["lf.h"], torch.relu(wide("lf.u")) * mult(2, ff))
    agree("z2", ref["lf.z2"], y1_given + (wide("lf.h") @ W["W_2"].T + W["b_2"]) * mult(3, d))
    agree("y2", ref["lf.y32"], y2)
    # backward, stage by stage: the reference takes the STORED float32 mean / rstd as given where autograd recomputes them exactly, hence
    # 1e-5 on the stages behind a LayerNorm; the given d_f, d_u, d_a, dqkv are the reference's own values as they would be stored
    bw = R.layer_bwd(a, sv, "both", False)
    given = {k: R.store(k, bw[k][0]) for k in ("lb.d_f", "lb.d_u", "lb.d_a", "lb.dqkv")}
    bw = R.layer_bwd(a, sv, "both", False, f64, (), given)
    gw = lambda n: t(R.bf16_f64(given[n]))      # noqa: E731
    y2.backward(t(a["g32"].astype(f64) + R.bf16_f64(a["g16"])))
    agree("d_f", bw["lb.d_f"], z2s.grad * mult(3, d), 1e-5)
    agree("dgamma2", bw["lb.dgamma2"], g2.grad + t(a["dg0"][0]), 1e-5)
    agree("dbeta2", bw["lb.dbeta2"], be2.grad + t(a["dg0"][1]), 1e-5)
    agree("d_u", bw["lb.d_u"], (gw("lb.d_f") @ W["W_2"]) * mult(2, ff) * t(R.bf16_f64(sv["lf.u"]) > 0))
    y1.backward(z2s.grad + gw("lb.d_u") @ W["W_1"])
    agree("d_a", bw["lb.d_a"], z1s.grad * mult(1, d), 1e-5)
    agree("dgamma1", bw["lb.dgamma1"], g1.grad + t(a["dg0"][2]), 1e-5)
    agree("dbeta1", bw["lb.dbeta1"], be1.grad + t(a["dg0"][3]), 1e-5)
    qs = t(R.bf16_f64(sv["lf.qkv"]), True)
    attention(qs).backward(gw("lb.d_a") @ W["W_out"])
    agree("dqkv", bw["lb.dqkv"], qs.grad, 1e-9)
    agree("dx32", bw["lb.dx32"], z1s.grad + gw("lb.dqkv") @ W["W_in"], 1e-5)
