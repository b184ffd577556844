"""tests/seq_block_ref.py on the CPU: (1) the float64 references against torch float64 autograd -- torch.softmax, F.layer_norm and
F.leaky_relu fed the same masks as multipliers, so no hand-written derivative stands unchecked; (2) the float32 evaluation of every
formula on the inputs tests/test_gpu_seq_block.py runs, whose largest constants are seq_block_ref.CPU_CONST (the GPU bounds are four
times these); (3) teeth: every wrong variant of the float32 evaluation listed in BUGS violates the GPU bound on a shape of the table.
"""
import functools

import numpy as np
import pytest

from tests import seq_block_ref as R

torch = pytest.importorskip("torch")
F = torch.nn.functional


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


def _agree(name, ref_unit, want):
    ref, unit = ref_unit
    want = want.detach().numpy().reshape(np.shape(ref))
    assert (np.abs(ref - want) <= 1e-12 * unit).all(), (name, float(np.abs(ref - want).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# (1) the references against autograd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ATT_CASES)
def test_attention_reference_against_autograd(case):
    Bn, S, H, dh, p = case
    call = R.case_counter("att", case)
    i = R.att_inputs(case)
    ref = R.evaluate("att", case)
    a = _t(R.bf16_f64(i["qkv"]).reshape(Bn, S, 3, H, dh), grad=True)
    q, k, v = (a[:, :, n].permute(0, 2, 1, 3) for n in range(3))
    keep = R._att_keep(Bn, S, H, p, R.SEED, call, None, 8)
    assert p == 0.0 or 0 < (~keep).sum() < keep.size
    mult = _t(keep / (1.0 - float(np.float32(p))))
    ctx = (torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(dh), dim=-1) * mult) @ v
    ctx = ctx.permute(0, 2, 1, 3).reshape(Bn * S, H * dh)
    ctx.backward(_t(R.bf16_f64(i["dctx"])))
    _agree("ctx", ref["att.ctx"], ctx)
    for n, name in enumerate(("dq", "dk", "dv")):
        _agree(name, ref["att." + name], a.grad[:, :, n].reshape(Bn * S, H * dh))


@pytest.mark.parametrize("case", R.LN_CASES)
def test_layernorm_reference_against_autograd(case):
    T, d, res16, p, _ = case
    call = R.case_counter("ln", case)
    i = R.ln_inputs(case)
    fwd = R.layernorm_fwd(i["x"], i["res"], res16, i["gamma"], i["beta"], R.LN_EPS, p, R.SEED, call)
    z, mean, rstd = (fwd[k][0] for k in ("z", "mean", "rstd"))            # the backward on the exact float64 forward
    bwd = R.layernorm_bwd(i["dy32"], i["dy16"], z, mean, rstd, i["gamma"], p, R.SEED, call, i["dgamma0"], i["dbeta0"])
    x, res = _t(R.bf16_f64(i["x"]), True), _t(R.bf16_f64(i["res"]) if res16 else i["res"], True)
    gamma, beta = _t(i["gamma"], True), _t(i["beta"], True)
    mult = _t(R._ln_keep(T, d, p, R.SEED, call) / (1.0 - float(np.float32(p))))
    zt = res + x * mult
    y = F.layer_norm(zt, (d,), gamma, beta, float(np.float32(R.LN_EPS)))
    g = np.zeros((T, d))
    g = g + (0 if i["dy32"] is None else i["dy32"].astype(np.float64)) + (0 if i["dy16"] is None else R.bf16_f64(i["dy16"]))
    y.backward(_t(g))
    _agree("y", fwd["y32"], y)
    _agree("z", fwd["z"], zt)
    _agree("mean", fwd["mean"], zt.mean(-1))
    _agree("rstd", fwd["rstd"], 1.0 / torch.sqrt(zt.var(-1, unbiased=False) + float(np.float32(R.LN_EPS))))
    _agree("dres", bwd["dres"], res.grad)
    _agree("dx", bwd["dx"], x.grad)
    _agree("dgamma", bwd["dgamma"], gamma.grad + _t(i["dgamma0"]))
    _agree("dbeta", bwd["dbeta"], beta.grad + _t(i["dbeta0"]))
    if d == 1:                       # variance zero: y = beta, nothing flows back
        assert (fwd["y32"][0] == i["beta"].astype(np.float64)).all() and (bwd["dres"][0] == 0).all()


@pytest.mark.parametrize("case", [c for c in R.ACT_CASES if c[0] in (257, 2048 * 256 + 3)])
def test_act_dropout_reference_against_autograd(case):
    n, slope, p = case
    call = R.case_counter("act", case)
    i = R.act_inputs(case)
    ref = R.evaluate("act", case)
    x = _t(R.bf16_f64(i["x"]), True)
    mult = _t(R.keep_mask(R.SEED, call, np.arange(n), p) / (1.0 - float(np.float32(p))))
    y = F.leaky_relu(x, float(np.float32(slope))) * mult
    y.backward(_t(R.bf16_f64(i["dy"])))
    _agree("y", ref["act.y"], y)
    _agree("dx", ref["act.dx"], x.grad)


@pytest.mark.parametrize("case", R.COMBINE_CASES)
def test_diffusion_references_against_autograd(case):
    B, Nc, d, _ = case
    i = R.combine_inputs(case)
    ref = R.evaluate("comb", case)
    m, cls = _t(R.bf16_f64(i["m"]), True), _t(i["cls"], True)
    sa, sb = _t(i["sa"]).reshape(B, Nc, 1), _t(i["sb"]).reshape(B, Nc, 1)
    rows = (_t(i["xn32"]).reshape(B, Nc, d) - sb * m.reshape(B, Nc, d)) / sa
    z = torch.cat([cls.expand(B, 1, d), rows], dim=1) + _t(i["pe"])
    g = np.zeros((B, Nc + 1, d)) + (0 if i["g"] is None else i["g"].astype(np.float64)) + (0 if i["g16"] is None else R.bf16_f64(i["g16"]))
    z.backward(_t(g))
    _agree("z", ref["comb.z"], z)
    _agree("dm", ref["comb.dm"], m.grad)
    _agree("dcls", ref["comb.dcls"], cls.grad + _t(i["dcls0"]))


def test_noise_reference_is_the_formula():
    for case in R.NOISE_CASES:
        i = R.noise_inputs(case)
        ref = R.evaluate("noise", case)
        a = _t(i["acp"])[torch.as_tensor(i["t"])][:, None]
        _agree("xn", ref["noise.xn32"], torch.sqrt(a) * _t(i["x"]) + torch.sqrt(1 - a) * _t(i["eps"]))


@pytest.mark.parametrize("case", R.WGRAD_CASES)
def test_weight_gradient_reference_against_autograd(case):
    T, N, K = case
    i = R.wgrad_inputs(case)
    ref = R.evaluate("wgrad", case)
    W, b = torch.zeros(N, K, dtype=torch.float64, requires_grad=True), torch.zeros(N, dtype=torch.float64, requires_grad=True)
    F.linear(_t(R.bf16_f64(i["X"])), W, b).backward(_t(R.bf16_f64(i["dY"])))
    _agree("dW", ref["wgrad.dW"], W.grad + _t(i["dW0"]))
    _agree("dbias", ref["wgrad.dbias"], b.grad + _t(i["dbias0"]))
    c = R.colsum_inputs()
    _agree("colsum", R.evaluate("colsum", R.COLSUM_CASE)["colsum.out"], _t(c["M"]).sum(0) + _t(c["out0"]))


def test_mask_is_the_device_stream_and_has_no_ties():
    """Uniforms on the 2^-24 grid against a float32 p: u >= p is decided exactly; the three counters give three different masks."""
    idx = np.arange(4096, dtype=np.uint64)
    masks = [R.keep_mask(R.SEED, c, idx, 0.1) for c in R.COUNTERS]
    u = R.bs.drop_uniform(R.bs.drop_key(R.SEED, R.COUNTERS[2]), idx)
    assert (u * 2.0 ** 24 == np.round(u * 2.0 ** 24)).all()
    assert all(0.85 < m.mean() < 0.95 for m in masks)
    assert not any(np.array_equal(masks[a], masks[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    assert R.bs.drop_key(R.SEED, 5) != R.bs.drop_key(R.SEED & ~(1 << 62), 5)


# ---------------------------------------------------------------------------------------------------------------------------------
# (2) the float32 evaluation: the constants behind the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def f32_constants(kind, case, bug=None, det=False, as_stored=True):
    """{output: largest error of the float32 evaluation in units of unit x EPS32}; sums over rows: the worse of the two orders.
    as_stored: bf16 outputs rounded to bf16 and held against 1/2 ulp_bf16 + the unit, as the GPU test holds the kernels' (the teeth
    check); False: the float32 value before that rounding against the unit alone -- the constant proper: after the rounding only the
    few elements next to a rounding tie would still show the float32 error at all."""
    ref = R.evaluate(kind, case, det=det)
    got = R.evaluate(kind, case, np.float32, bug, det)
    out = {}
    for name, (want, unit) in ref.items():
        vals = got[name][0]
        worst = 0.0
        for val in (vals if isinstance(vals, list) else [vals]):
            val = R.stored(name, val, truncate=bug == "trunc") if as_stored else np.asarray(val, dtype=np.float64)
            if bug == "tail_row" and val.ndim == 2:
                val = val.copy()
                val[-1] = R.SENT_BF16_VALUE if name in R.BF16_OUTPUTS else float(R.SENT_F32)
            worst = max(worst, R.error_ratio(val, want, unit, as_stored and name in R.BF16_OUTPUTS))
            if not R.exact_zeros(val, want):
                worst = np.inf
        out[name] = worst
    return out


ALL_CASES = [(kind, case) for kind, cases in R.CASES.items() for case in cases]


@functools.lru_cache(maxsize=None)
def case_constants(kind, case):
    """The constants of one case: the float32 values before and after they are stored (the weight gradient's largest shape in
    deterministic mode as well), the larger per output."""
    runs = [f32_constants(kind, case, as_stored=False), f32_constants(kind, case)]
    if case == (1025, 70, 65):
        runs.append(f32_constants(kind, case, det=True))
    return {name: max(r[name] for r in runs) for name in runs[0]}


@pytest.mark.parametrize("kind,case", ALL_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_float32_evaluation_stays_inside_the_table(kind, case):
    c = case_constants(kind, case)
    print(kind, case, "  ".join(f"{k} {v:.2f}" for k, v in c.items()))
    for name, v in c.items():
        assert v <= R.CPU_CONST[name], (name, v)


def test_table_of_constants_is_what_was_measured():
    """One line per output (pytest -s): the largest measured constant, the table's entry and the GPU bound.  An entry of the table is
    the measurement plus a tenth, rounded up: a slack entry would be a slack bound, so none may exceed 1.5 x measured + 0.1."""
    measured = {}
    for kind, case in ALL_CASES:
        for name, v in case_constants(kind, case).items():
            measured[name] = max(measured.get(name, 0.0), v)
    assert set(measured) == set(R.CPU_CONST)
    for name in R.CPU_CONST:
        print(f"{name:12s} measured {measured[name]:6.2f}   table {R.CPU_CONST[name]:5.2f}   GPU bound {R.bound_constant(name):6.2f}")
    for name in R.CPU_CONST:
        assert measured[name] <= R.CPU_CONST[name] <= 1.5 * measured[name] + 0.1, name


# ---------------------------------------------------------------------------------------------------------------------------------
# (3) teeth
# ---------------------------------------------------------------------------------------------------------------------------------
BUGS = [("mask_ji", "att", ("att.ctx", "att.dq", "att.dk", "att.dv")),          # the mask indexed (.. S + j) S + i
        ("local_b", "att", ("att.ctx", "att.dq")),                               # the sample index within the workgroup
        ("no_ks", "att", ("att.dq", "att.dk")),                                  # 1 / (1 - p) left out of one backward
        ("no_ks", "ln", ("ln.dx",)),
        ("no_ks", "act", ("act.dx",)),
        ("dv_P", "att", ("att.dv",)),                                            # P instead of P~
        ("drop_after_add", "ln", ("ln.z", "ln.y32")),                            # dropout(res + x)
        ("trunc", "act", ("act.y", "act.dx")),                                   # bf16 by truncation
        ("trunc", "att", ("att.ctx", "att.dv")),
        ("trunc", "ln", ("ln.y16", "ln.dx")),
        ("tail_row", "att", ("att.ctx", "att.dq", "att.dk", "att.dv")),          # one row of the tail workgroup keeps the sentinel
        ("tail_row", "ln", ("ln.y32", "ln.dres", "ln.dx")),
        ("dw_overwrite", "wgrad", ("wgrad.dW",))]


@pytest.mark.parametrize("bug,kind,outputs", BUGS, ids=[f"{b}-{k}" for b, k, _ in BUGS])
def test_wrong_variants_violate_the_gpu_bound(bug, kind, outputs):
    broken = set()
    for case in R.CASES[kind]:
        if kind == "act" and case[0] > 257:
            continue
        for name, v in f32_constants(kind, case, bug).items():
            if v > R.bound_constant(name):
                broken.add(name)
    assert broken >= set(outputs), (bug, kind, sorted(broken))


def test_attention_support_states_both_entry_points_host_checks():
    """tfd_fused.attention_support against the samples-per-workgroup rule of seq_block.hip (mirrored in seq_block_ref): d = 256, H = 64
    fits the forward's LDS for every S <= 8 and the backward's only up to S = 5; the training path needs both."""
    from openpystruct_amd import tfd_fused as TF
    assert float(R.bf16_f64(R.SENT_BF16).reshape(-1)[0]) == R.SENT_BF16_VALUE
    for S in range(1, 9):
        for H in (1, 2, 4, 8, 16, 32, 48, 64, 128):
            for dh in (1, 2, 4, 8, 15, 16, 20, 32):
                if H * dh <= 256 and (H * dh) % 8 == 0:
                    want = tuple(S * H <= 512 and R.att_samples_per_wg(S, H, dh, bwd) >= 1 for bwd in (False, True))
                    assert TF.attention_support(S, H, dh) == want, (S, H, dh)
    assert [TF.attention_support(S, 64, 4) for S in (5, 6, 8)] == [(True, True), (True, False), (True, False)]
    assert TF.attention_support(8, 48, 4) == (True, False) and TF.attention_support(8, 128, 2) == (False, False)
    assert TF.attention_support(7, 8, 15) == (True, True) and TF.attention_support(9, 8, 15) == (False, False)
