"""tests/mlp_block_ref.py on the CPU: (1) the layout helpers against pinn_fused.to_tiled / from_tiled and the kernel's offset formula;
(2) the float64 reference against float64 torch autograd of the plain composition -- nn.Linear, Conv1d(1, 1, 3, padding=1),
BatchNorm1d(1), BatchNorm1d, LeakyReLU, the mirrored masks, CompositeLoss -- forward and backward, so no hand-written derivative stands
unchecked (module path for B >= 2; the B = 1 guard is asserted directly); (3) the float32 evaluation through the very protocols
tests/test_gpu_mlp_block.py runs, whose largest constants are mlp_block_ref.CPU_CONST (the GPU bounds are four times these), and the
product's ceiling; (4) teeth: every wrong variant in BUGS violates the GPU bound or an exact condition.
"""
import functools

import numpy as np
import pytest

from tests import mlp_block_ref as R

torch = pytest.importorskip("torch")
nn = torch.nn
f32, f64 = np.float32, np.float64
_ids = lambda v: v if isinstance(v, str) else "-".join(map(str, v)).replace(" ", "")[:60]      # noqa: E731


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=f64), dtype=torch.float64, requires_grad=grad)


def _agree(name, ref, want):
    ref, unit = np.asarray(ref[0], dtype=f64), np.asarray(ref[1], dtype=f64)
    want = want.detach().numpy().reshape(ref.shape)
    assert (np.abs(ref - want) <= 1e-11 * np.maximum(unit, np.abs(ref))).all(), (name, float(np.abs(ref - want).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# (1) layout
# ---------------------------------------------------------------------------------------------------------------------------------
def test_layout_helpers_are_pinn_fused_and_the_kernels_offsets():
    from openpystruct_amd import pinn_fused
    for rows, K in ((16, 32), (48, 96), (128, 1056)):
        x = np.arange(rows * K, dtype=np.int64).reshape(rows, K)
        t = R.to_tiled(x)
        assert np.array_equal(t, pinn_fused.to_tiled(torch.from_numpy(x)).numpy())
        assert np.array_equal(R.from_tiled(t), x) and np.array_equal(pinn_fused.from_tiled(torch.from_numpy(t)).numpy(), x)
        r, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
        assert np.array_equal(t.ravel()[R.tiled_offset(r, k, K // 32)], x)
    bits = np.arange(1, 3 * 5 + 1, dtype=np.uint16).reshape(3, 5)
    p = R.from_tiled(R.pack(bits, 16, 64))
    assert np.array_equal(p[:3, :5], bits) and not p[:, :32][3:].any() and not p[:3, 5:32].any() and (p[:, 32:] == R.SENT_BF16).all()
    assert np.array_equal(R.from_tiled(R.pack_t(bits))[:5, :3], bits.T)


# ---------------------------------------------------------------------------------------------------------------------------------
# (2) the reference against autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def _bn(n, gamma, beta, rmean, rvar, eps, mom):
    bn = nn.BatchNorm1d(n, eps=float(f32(eps)), momentum=float(f32(mom))).double()
    with torch.no_grad():
        bn.weight.copy_(_t(gamma)); bn.bias.copy_(_t(beta)); bn.running_mean.copy_(_t(rmean)); bn.running_var.copy_(_t(rvar))
    return bn


def _linear(a):
    N, K = a["W"].shape
    lin = nn.Linear(K, N).double()
    with torch.no_grad():
        lin.weight.copy_(_t(R.bf16_f64(a["W"])))
        lin.bias.copy_(_t(R.bf16_f64(R.bf16_bits(a["bias"]))))
    return lin


def _mask(a):
    B, N = a["B"], a["N"]
    r, c = np.arange(B, dtype=np.uint64)[:, None], np.arange(N, dtype=np.uint64)[None, :]
    return R.keep_mask(a["seed"], a["call"], r * np.uint64(N) + c, a["p"]) / (1.0 - float(f32(a["p"])))


@pytest.mark.parametrize("B,N,K,ev", [(33, 17, 33, 0), (2, 40, 70, 0), (33, 17, 33, 1)])
def test_forward_tail_reference_against_the_modules(B, N, K, ev):
    """dropout(LeakyReLU(BatchNorm1d(Linear(x)))) with the mirrored mask."""
    a = R.launch(B, N, K, R.BN_ACT_DROP, ev=ev, p=0.0 if ev else 0.1, slope=0.01, call=5)
    ref = R.strip(a)
    lin, bn = _linear(a), _bn(N, a["gamma"], a["beta"], a["rmean"], a["rvar"], a["eps"], a["momentum"])
    bn.train(not ev)
    z = lin(_t(R.bf16_f64(a["A"])))
    y = nn.LeakyReLU(float(f32(a["slope"])))(bn(z)) * _t(_mask(a))
    _agree("z", ref["z"], z)
    _agree("y", ref["y"], y)
    if not ev:
        _agree("mean", ref["mean"], z.mean(0))
        _agree("rstd", ref["rstd"], 1 / torch.sqrt(z.var(0, unbiased=False) + float(f32(a["eps"]))))
        _agree("rmean", ref["rmean"], bn.running_mean)
        _agree("rvar", ref["rvar"], bn.running_var)
    else:
        assert "mean" not in ref and "rmean" not in ref


def _stencil_modules(a):
    conv = nn.Conv1d(1, 1, 3, padding=1).double()
    with torch.no_grad():
        conv.weight.copy_(_t(a["cw"]).view(1, 1, 3)); conv.bias.copy_(_t(a["cb"]))
    return conv, _bn(1, a["sgamma"], a["sbeta"], a["srm"], a["srv"], a["seps"], a["smom"])


@pytest.mark.parametrize("B,N,K,ev", [(33, 17, 33, 0), (2, 9, 70, 0), (5, 1, 32, 0), (33, 17, 33, 1)])
def test_block_sum_reference_against_the_modules(B, N, K, ev):
    """norm(fc2(h) + bn1(conv1(o)) + o): the ResidualBlock's sum and the BatchNorm1d behind it, the side job's partial sums included."""
    a = R.launch(B, N, K, R.BN, R.ADD_FWD, ev=ev)
    part = R.side_job(dict(a, side=R.SIDE_FWD))[0]
    assert part.shape == ((N + 7) // 8, 2)
    ref = R.strip(dict(a, spart=part.ravel()))
    lin, bn = _linear(a), _bn(N, a["gamma"], a["beta"], a["rmean"], a["rvar"], a["eps"], a["momentum"])
    conv, bn1 = _stencil_modules(a)
    for m in (bn, bn1):
        m.train(not ev)
    o = _t(R.bf16_f64(a["O"]))
    y1 = conv(o.unsqueeze(1))
    z = lin(_t(R.bf16_f64(a["A"]))) + bn1(y1).squeeze(1) + o
    _agree("z", ref["z"], z)
    _agree("y", ref["y"], bn(z))
    if not ev:
        _agree("ssave", ref["ssave"], torch.stack([y1.mean(), 1 / torch.sqrt(y1.var(unbiased=False) + float(f32(a["seps"])))]))
        _agree("srm", ref["srm"], bn1.running_mean)
        _agree("srv", ref["srv"], bn1.running_var)
        _agree("rvar", ref["rvar"], bn.running_var)


@pytest.mark.parametrize("B,N,K,p,slope", [(33, 17, 33, 0.1, 0.01), (2, 9, 70, 0.5, 1.0), (7, 1, 32, 0.0, 0.0), (5, 40, 33, 0.1, 0.01)])
def test_backward_reference_against_autograd(B, N, K, p, slope):
    """u -> o = dropout(LeakyReLU(BatchNorm1d(u))) -> { bn1(conv1(o)) + o  (gradient dZ),  fc1(o)  (gradient dH) }: the launch
    TAIL_BWD_BN_ACT_DROP + ADD_BWD_BLOCK gives d/du, dgamma, dbeta and the stencil's six parameter gradients."""
    a = R.launch(B, N, K, R.BWD_BN_ACT_DROP, R.ADD_BWD, p=p, slope=slope, call=5)
    u = _t(R.bf16_f64(a["Z"]), True)
    bn = _bn(N, a["gamma"], a["beta"], a["rmean"], a["rvar"], a["eps"], a["momentum"])
    keep = R.bf16_f64(a["Yref"]) != 0
    o = nn.LeakyReLU(float(f32(slope)))(bn(u)) * _t(keep / (1.0 - float(f32(p))))
    conv, bn1 = _stencil_modules(a)
    y1 = conv(o.unsqueeze(1))
    t = bn1(y1).squeeze(1) + o
    h1 = o @ _t(R.bf16_f64(a["W"]))                       # W of the launch: the transposed weight of fc1, [N, K]
    ((t * _t(R.bf16_f64(a["dZ"]))).sum() + (h1 * _t(R.bf16_f64(a["A"]))).sum()).backward()
    # the launch's inputs as the forward left them, unrounded: block input, its sign / mask, the saved statistics
    ud = u.detach()
    a = dict(a, O=o.detach().numpy(), Yref=o.detach().numpy(), mean=ud.mean(0).numpy(),
             rstd=(1 / torch.sqrt(ud.var(0, unbiased=False) + float(f32(a["eps"])))).numpy(),
             ssave=np.array([float(y1.detach().mean()), float(1 / torch.sqrt(y1.detach().var(unbiased=False) + float(f32(a["seps"]))))]))
    if B * N == 1:
        return
    part = R.side_job(dict(a, side=R.SIDE_BWD))[0]
    assert part.shape == ((N + 7) // 8, 12)
    ref = R.strip(dict(a, spart=part.ravel()))
    _agree("dgamma", ref["dgamma"], bn.weight.grad)
    _agree("dbeta", ref["dbeta"], bn.bias.grad)
    _agree("du", ref["y"], u.grad)
    want = torch.cat([conv.weight.grad.view(3), conv.bias.grad.view(1), bn1.weight.grad.view(1), bn1.bias.grad.view(1)])
    _agree("sdparams", ref["sdparams"], want)


def test_backward_tails_without_the_block_against_autograd():
    B, N, K = 33, 17, 33
    for tail in (R.BWD_ACT_DROP, R.BWD_BN):
        a = R.launch(B, N, K, tail, p=0.1, slope=0.01, call=5)
        dH, W = _t(R.bf16_f64(a["A"])), _t(R.bf16_f64(a["W"]))
        if tail == R.BWD_ACT_DROP:
            yr = R.bf16_f64(a["Yref"])
            u = _t(np.where(yr > 0, 1.0, -1.0), True)                           # any pre-activation with the saved output's signs
            o = nn.LeakyReLU(float(f32(0.01)))(u) * _t((yr != 0) / (1.0 - float(f32(0.1))))
        else:
            u = _t(R.bf16_f64(a["Z"]), True)
            bn = _bn(N, a["gamma"], a["beta"], a["rmean"], a["rvar"], a["eps"], a["momentum"])
            o = bn(u)
            ud = u.detach()
            a = dict(a, mean=ud.mean(0).numpy(), rstd=(1 / torch.sqrt(ud.var(0, unbiased=False) + float(f32(a["eps"])))).numpy())
        ((o @ W) * dH).sum().backward()
        ref = R.strip(a)
        _agree("du", ref["y"], u.grad)
        if tail == R.BWD_BN:
            _agree("dgamma", ref["dgamma"], bn.weight.grad)
            _agree("dbeta", ref["dbeta"], bn.bias.grad)


def test_batch_of_one_takes_the_documented_guard():
    """B = 1: mean = z, variance 0, and the running variance moves by momentum x 0 x (B / max(B - 1, 1) = 1) -- BatchNorm1d refuses it."""
    a = R.launch(1, 16, 32, R.BN)
    for dt in (f64, f32):
        o = R.strip(a, dt)
        eps, mo = dt(f32(R.EPS)), dt(f32(R.MOM))
        assert np.array_equal(o["mean"][0], o["z"][0][0].astype(dt))
        assert np.allclose(o["rstd"][0], 1 / np.sqrt(eps), rtol=1e-6) and np.allclose(o["rvar"][0], (1 - mo) * a["rvar"].astype(dt), rtol=1e-6)
        assert np.allclose(o["y"][0][0], a["beta"], rtol=1e-6)
    b = R.launch(1, 9, 32, R.BN, R.ADD_FWD)
    b = dict(b, spart=R.side_job(dict(b, side=R.SIDE_FWD))[0].ravel())
    assert np.isfinite(R.strip(b)["srv"][0])
    one = R.launch(1, 1, 32, R.BN, R.ADD_FWD)                                    # n = 1: n / (n > 1 ? n - 1 : 1) = 1, variance 0
    one = dict(one, spart=R.side_job(dict(one, side=R.SIDE_FWD))[0].ravel())
    assert abs(float(R.strip(one)["srv"][0]) - (1 - float(f32(R.SMOM))) * float(one["srv"][0])) < 1e-12


def test_loss_reference_against_the_module_and_the_finishing_sum():
    from openpystruct_amd.surrogates import CompositeLoss
    for case in R.LOSS_CASES:
        a = R.loss_launches(case)[0]
        B, C, nI, nD = case[:4]
        ref = R.strip(a)
        pb = R.bf16_bits(ref["p"][0].astype(f32))
        v, uv = R.loss_finish(ref["parts"][0], a, B)
        assert abs(v - float(ref["value"][0])) <= 1e-12 * uv, case
        if nD > 0 and C - nI - nD > 0:
            a32 = float(f32(a["alpha"]))
            crit = CompositeLoss(nI, nD, C - nI - nD, a32, float(f32(a["box_w"])), penalty_pinn=float(f32(a["pen"])),
                                 min_constraint=None if a["lo"] is None else float(f32(a["lo"])),
                                 max_constraint=None if a["hi"] is None else float(f32(a["hi"]))).double()
            crit.l1l2_loss.alpha.data.fill_(a32)
            p = _t(R.bf16_f64(pb), True)
            loss = crit(p, _t(a["targets"]))
            if a["alpha0"] == a["alpha0"]:
                loss = loss + (float(f32(a["alpha0"])) - a32) ** 2
            loss.backward()
            _agree("value", ref["value"], loss)
            _agree("grad", ref["y"], p.grad)
        assert (R.bf16_f64(pb) == a["targets"]).any() or B * C < 6, "p == t is planted"


def test_weight_gradient_reference_against_autograd():
    case = R.WG_CASES[1]
    problems, _ = R.wgrad_inputs(case)
    ref = R.wgrad_group(problems)
    for (At, Bt), (v, u) in zip(problems, ref["out"]):
        lin = nn.Linear(Bt.shape[0], At.shape[0], bias=False).double()
        (lin(_t(R.bf16_f64(Bt).T)) * _t(R.bf16_f64(At).T)).sum().backward()
        _agree("dW", (v, u), lin.weight.grad)


# ---------------------------------------------------------------------------------------------------------------------------------
# (3) the float32 evaluation: the constants behind the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
ALL_CASES = [(kind, case) for kind, (_, cases) in R.PROTOCOLS.items() for case in cases]


@functools.lru_cache(maxsize=None)
def case_constants(kind, case_index, bug=()):
    return R.measure(R.PROTOCOLS[kind][0](R.PROTOCOLS[kind][1][case_index], R.CpuImpl(bug)))


def _constants(kind, case, bug=()):
    return case_constants(kind, R.PROTOCOLS[kind][1].index(case), bug)


@pytest.mark.parametrize("kind,case", ALL_CASES, ids=_ids)
def test_float32_evaluation_stays_inside_the_table(kind, case):
    ratios, failed = _constants(kind, case)
    print(kind, case, "  ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert not failed, failed
    for name, v in ratios.items():
        assert v <= R.CPU_CONST[name], (name, v)


def test_table_of_constants_is_what_was_measured():
    """One line per output (pytest -s): the largest measured constant, the table's entry and the GPU bound.  An entry is the measurement
    plus about 12 %, rounded up: a slack entry would be a slack bound, so none may exceed 1.5 x measured + 0.1."""
    measured = {name: 0.0 for name in R.CPU_CONST}
    for kind, case in ALL_CASES:
        for name, v in _constants(kind, case)[0].items():
            measured[name] = max(measured[name], v)
    for name in R.CPU_CONST:
        print(f"{name:12s} measured {measured[name]:6.2f}   table {R.CPU_CONST[name]:5.2f}   GPU bound {R.bound_constant(name):6.2f}")
    for name in R.CPU_CONST:
        assert measured[name] <= R.CPU_CONST[name] <= 1.5 * measured[name] + 0.1, name


def test_product_bound_stays_below_the_any_order_ceiling():
    """bf16 x bf16 is exact in float32, only the additions round: any order of the K r.u. 32 additions is within 2 (K r.u. 32) units.  The
    GPU bound of every output that is a product must stay below it at every K of the tables (K = 1: 64)."""
    ks = {c[2] for c in R.PRODUCT_CASES} | {s[2] for s in R.SHAPES} | {32, 33, 70, 175}
    for name in ("prod.y", "fwd.z", "loss.p", "wg.out"):
        for K in sorted(ks):
            print(f"{name}: K = {K}: bound {R.bound_constant(name):.2f} < ceiling {R.product_ceiling(K):.0f}")
            assert R.bound_constant(name) < R.product_ceiling(K)
    assert sorted({(c[2] + 31) // 32 for c in R.PRODUCT_CASES}) == [1, 2, 8, 9, 16, 17, 24, 25, 33]
    assert {c[1] for c in R.PRODUCT_CASES} == {1, 15, 16, 17, 175} and {c[0] for c in R.PRODUCT_CASES} == {1, 31, 32, 33, 127, 128}


def test_exact_twins_stay_below_two_to_the_eighth():
    for k, (B, N, K, pd) in enumerate(R.PRODUCT_CASES):
        a = R.launch(B, N, K, key=k, exact=True)
        assert R.exact_twin_ok(a), (B, N, K)
        A = R.bf16_f64(a["A"])
        assert all(A[:, 32 * s:32 * s + 32].any() for s in range((K + 31) // 32)), "a reduction step without a non-zero operand"
        y = R.strip(a)["y"][0]
        assert np.array_equal(y, np.round(y)) and np.abs(y).max() < 256 and np.array_equal(R.strip(a, f32)["y"][0], y)


# ---------------------------------------------------------------------------------------------------------------------------------
# (4) teeth
# ---------------------------------------------------------------------------------------------------------------------------------
BUGS = [("skip_last_step", "product", ("prod.y", "twin: bit for bit")),
        ("fa1_reuse", "product", ("prod.y", "twin: bit for bit")),
        ("left_tap_col0", "block", ("st.part", "fwd.z", "st.bsums", "bwd.y")),
        ("right_tap_last", "block", ("st.part", "fwd.z", "st.bsums", "bwd.y")),
        ("biased_running_var", "combo", ("fwd.rvar", "st.rvar")),
        ("count_padded", "combo", ("st.save", "fwd.z", "bwd.y")),
        ("invB_128", "combo", ("fwd.mean", "fwd.rstd", "fwd.y", "bwd.y")),
        ("keep_gt", "tie", ("fwd.y",)),
        ("dbias_unrounded", "combo", ("bwd.dbias",)),
        ("dbias_unrounded", "loss", ("loss.dbias",)),
        ("dgamma_no_mean", "combo", ("bwd.dgamma", "bwd.y")),
        ("dgamma_no_mean", "bwdx", ("bwd.dgamma", "bwd.y")),
        ("invB_128", "bwdx", ("bwd.y",)),
        ("yt_tile_transposed", "combo", ("Y and Yt hold identical bit patterns",)),
        ("loss_mean_N", "loss", ("loss.grad",)),
        ("wgrad_past_edge", "wgrad", ("columns K .. ldo - 1 untouched",)),
        ("range_half", "wgrad", ("wg.range",))]


@pytest.mark.parametrize("bug,kind,outputs", BUGS, ids=[f"{b}-{k}" for b, k, _ in BUGS])
def test_wrong_variants_violate_the_gpu_bound(bug, kind, outputs):
    broken, first = set(), {}
    for case in R.PROTOCOLS[kind][1]:
        ratios, failed = _constants(kind, case, bug)
        now = {name for name, v in ratios.items() if v > R.bound_constant(name)} | set(failed)
        for name in now - broken:
            first[name] = case
        broken |= now
    print(f"{bug}: caught on {sorted(broken)}; first at {({k: first[k] for k in outputs if k in first})}")
    assert broken >= set(outputs), (bug, kind, sorted(broken))


def test_wrong_variants_are_caught_at_the_smallest_case_that_can_show_them():
    """The K edges of the product table: a skipped last step shows at K = 33 (two steps), a reused second chunk first at 25 steps."""
    small = lambda bug, K: _constants("product", next(c for c in R.PRODUCT_CASES if c[2] == K), bug)      # noqa: E731
    assert small("skip_last_step", 33)[0]["prod.y"] > R.bound_constant("prod.y")
    assert small("fa1_reuse", 768)[0]["prod.y"] <= R.bound_constant("prod.y")        # 24 steps: the chunk is not reloaded yet
    assert small("fa1_reuse", 769)[0]["prod.y"] > R.bound_constant("prod.y")         # 25 steps
    for No in (1, 2):                                    # a single column has no neighbours: both tap variants are invisible there and show at 2
        case = next(c for c in R.BLOCK_CASES if c[2] == No and c[0] == R.BN)
        for bug in ("left_tap_col0", "right_tap_last"):
            r, _ = _constants("block", case, bug)
            caught = r["fwd.z"] > R.bound_constant("fwd.z")
            assert caught == (No > 1 or (bug == "right_tap_last" and case[3] > 1)), (bug, No, r)
