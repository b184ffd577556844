"""The row-wise encoder kernels of csrc/seq_block.hip, entry point by entry point through the C ABI, against the float64 references of
tests/seq_block_ref.py WITH dropout on: the masks are reproduced on the host (tests/bayes_stream.py), every element of every output
is compared (none excluded), every output buffer is pre-filled with a sentinel between two guard rows.

Errors are elementwise in units of unit x 2^-24 (bf16 outputs: beyond 1/2 ulp_bf16 of the reference); the unit is the output's formula
with absolute values throughout (seq_block_ref.py).  "CPU": largest constant of the float32 NumPy evaluation on these inputs
(tests/test_seq_block_reference.py); bound = 4 x CPU (device exp / rsqrt / reciprocal, butterfly and atomic orders, 1 / (1 - p) in
float32); "MI355X": largest value seen there.

  output        CPU    bound   MI355X           output        CPU    bound   MI355X
  att.ctx       5.48   24.0     0.32            act.y         1.91    8.4     0.00
  att.dq        1.43    6.4     0.28            act.dx        2.04    9.0     0.00
  att.dk        1.82    8.0     0.15            noise.xn32    2.28   10.0     2.28
  att.dv        4.53   20.0     1.71            noise.xn16    2.28   10.0     0.00
  ln.y32        3.84   16.8     3.49            noise.sa      0.88    4.0     0.88
  ln.y16        3.84   16.8     0.41            noise.sb      1.00    4.4     1.00
  ln.z          2.52   11.2     2.52            comb.z        2.65   11.6     2.65
  ln.mean       2.23   10.0     2.25            comb.z16      2.65   11.6     0.02
  ln.rstd       0.81    3.6     0.97            comb.dm       2.69   12.0     0.00
  ln.dres       1.25    5.6     1.34            comb.dcls     1.71    7.6     1.10
  ln.dx         1.60    7.2     0.07            wgrad.dW      1.70    7.6     1.37
  ln.dgamma     0.77    3.4     0.43            wgrad.dbias   0.25    1.12    0.25
  ln.dbeta      1.02    4.6     0.71            colsum.out    0.62    2.8     0.62

(A bf16 output shows its float32 error only at the few elements next to a rounding tie -- everywhere else the stored value is the
reference's own rounding and the error beyond 1/2 ulp is zero -- so the CPU column measures those on the float32 value before it is
stored, and the MI355X column of the bf16 outputs is small.  No bound was widened.)

Protocol: the call counter is 0, 5 and 2^32 + 5 in turn down each table, the seed has bit 62 set; `used_call` must come back as the
counter's value (0 where p = 0: such a launch reads no counter), and the counter is changed between the forward and the backward
call, which must reproduce the forward's mask from `used_call`.

Defects found with these tests (shape, cause):
  attention d = 256, H = 64, S in {6, 7, 8} (and d = 192, H = 48, S = 8): the backward's LDS (S 4 H DHP 2 + 2 H S^2 4 bytes per sample)
      does not fit where the forward's (S 3 H DHP 2) does, and tfd_fused._layer_ok gated on neither: the layer trained one forward, then
      its backward was refused inside autograd.  tfd_fused.attention_support states both checks; a training pass whose backward
      cannot run takes the framework's forward (test_attention_support_agreement, test_layer_whose_backward_cannot_run_...).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import seq_block_ref as R  # noqa: E402

DEV = "cuda"
WORST = {}                 # output -> largest error seen in units of unit x 2^-24, printed when the module is done
_ids = lambda c: "-".join(map(str, c))      # noqa: E731


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi
    yield _cabi.load()
    for name, e in sorted(WORST.items()):
        print(f"\nlargest error on the GPU, {name:12s} {e:7.2f} = {e / R.bound_constant(name):5.2f} of its bound {R.bound_constant(name):.2f}", end="")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    """A host array on the device, 16-byte aligned; bf16 travels as its bit patterns."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _i64(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


class Out:
    """An output of `shape` ("bf16" or "f32") between two guard rows, all pre-filled with a sentinel -- or, for an output the kernel
    adds to, holding `init` between the guards."""

    def __init__(self, shape, kind, init=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.guard = -(-max(self.n // shape[0], 1) // 8) * 8             # a row, rounded up: the output proper stays 16-byte aligned
        self.bf16 = kind == "bf16"
        self.sent = int(np.array(R.SENT_BF16).view(np.int16)) if self.bf16 else float(R.SENT_F32)
        self.buf = torch.full((self.n + 2 * self.guard,), self.sent, dtype=torch.int16 if self.bf16 else torch.float32, device=DEV)
        self.added = init is not None
        if self.added:
            self.buf[self.guard:self.guard + self.n] = _dev(np.asarray(init, dtype=np.float32).reshape(-1))
        self.ptr = self.buf.data_ptr() + self.guard * self.buf.element_size()

    def get(self, untouched=False):
        """The output widened to float64; asserts the guards are untouched and (unless the kernel adds) every element was written."""
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        g, body = self.guard, raw[self.guard:self.guard + self.n]
        assert (raw[:g] == raw.dtype.type(self.sent)).all() and (raw[g + self.n:] == raw.dtype.type(self.sent)).all(), "a guard row was written"
        if untouched:
            assert (body == raw.dtype.type(self.sent)).all(), "a refused call wrote its output"
        elif not self.added:
            assert not (body == raw.dtype.type(self.sent)).any(), "an element of the output was not written"
        self.bits = body.view(np.uint16).reshape(self.shape) if self.bf16 else None
        return (R.bf16_f64(body.view(np.uint16)) if self.bf16 else body.astype(np.float64)).reshape(self.shape)


def check(name, got, ref_unit):
    ref, unit = ref_unit
    ref, unit = np.asarray(ref).reshape(got.shape), np.asarray(unit).reshape(got.shape)
    e = R.error_ratio(got, ref, unit, name in R.BF16_OUTPUTS)
    WORST[name] = max(WORST.get(name, 0.0), e)
    print(f"{name} {got.shape}: {e:.2f} of {R.bound_constant(name):.2f}")
    assert R.exact_zeros(got, ref), (name, "non-zero where the reference is exactly zero")
    assert e <= R.bound_constant(name), (name, e, R.bound_constant(name))


def _used_ok(used, call, p):
    torch.cuda.synchronize()
    assert int(used.item()) == (call if p > 0 else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ATT_CASES, ids=_ids)
def test_attention(lib, case):
    Bn, S, H, dh, p = case
    d, call = H * dh, R.case_counter("att", case)
    i, ref = R.att_inputs(case), R.evaluate("att", case)
    qkv, dctx = _dev(i["qkv"]), _dev(i["dctx"])
    counter, used = _i64(call), _i64(-1)
    ctx, dqkv = Out((Bn * S, d), "bf16"), Out((Bn * S, 3 * d), "bf16")
    assert lib.ops_seq_attention_fwd(Bn, S, H, dh, qkv.data_ptr(), ctx.ptr, p, R.SEED, counter.data_ptr(), used.data_ptr(), _stream()) == 0
    _used_ok(used, call, p)
    check("att.ctx", ctx.get(), ref["att.ctx"])
    counter.fill_(call + 1)                                  # the backward reads used_call, not the counter
    assert lib.ops_seq_attention_bwd(Bn, S, H, dh, qkv.data_ptr(), dctx.data_ptr(), dqkv.ptr, p, R.SEED, used.data_ptr(), _stream()) == 0
    got = dqkv.get()
    for n, name in enumerate(("att.dq", "att.dk", "att.dv")):
        check(name, got[:, n * d:(n + 1) * d], ref[name])
    if S == 1 and p > 0:                                     # one key: a row is kept whole or exactly zero
        rows = ctx.get().reshape(Bn * H, dh)
        assert (rows == 0).all(-1).any() and (rows != 0).any(-1).any()


@pytest.mark.parametrize("case", R.LN_CASES, ids=_ids)
def test_dropout_add_layernorm(lib, case):
    T, d, res16, p, grads = case
    call = R.case_counter("ln", case)
    i, ref = R.ln_inputs(case), R.evaluate("ln", case)
    x, res, gamma, beta = _dev(i["x"]), _dev(i["res"]), _dev(i["gamma"]), _dev(i["beta"])
    counter, used = _i64(call), _i64(-1)
    o = {k: Out((T, d), "f32") for k in ("y32", "z", "dres")}
    o.update({k: Out((T, d), "bf16") for k in ("y16", "dx")}, mean=Out((T,), "f32"), rstd=Out((T,), "f32"),
             dgamma=Out((d,), "f32", i["dgamma0"]), dbeta=Out((d,), "f32", i["dbeta0"]))
    assert lib.ops_dropout_add_layernorm_fwd(T, d, x.data_ptr(), res.data_ptr(), int(res16), gamma.data_ptr(), beta.data_ptr(), R.LN_EPS, p, R.SEED,
                                             counter.data_ptr(), used.data_ptr(), o["y32"].ptr, o["y16"].ptr, o["z"].ptr, o["mean"].ptr,
                                             o["rstd"].ptr, _stream()) == 0
    _used_ok(used, call, p)
    for k in ("y32", "y16", "z", "mean", "rstd"):
        check("ln." + k, o[k].get(), ref["ln." + k])
    if d == 1:                                               # variance zero: y = beta exactly
        assert (o["y32"].get() == float(i["beta"][0])).all()
    # the backward on the reference's saved arrays (seq_block_ref.ln_saved), the mask from used_call under a changed counter
    z, mean, rstd = (_dev(a) for a in R.ln_saved(case))
    dy32, dy16 = (None if i[k] is None else _dev(i[k]) for k in ("dy32", "dy16"))
    counter.fill_(call + 7)
    assert lib.ops_dropout_add_layernorm_bwd(T, d, _ptr(dy32), _ptr(dy16), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), p, R.SEED,
                                             used.data_ptr(), o["dx"].ptr, o["dres"].ptr, o["dgamma"].ptr, o["dbeta"].ptr, _stream()) == 0
    for k in ("dres", "dx", "dgamma", "dbeta"):
        check("ln." + k, o[k].get(), ref["ln." + k])


@pytest.mark.parametrize("case", R.ACT_CASES, ids=_ids)
def test_act_dropout(lib, case):
    n, slope, p = case
    call = R.case_counter("act", case)
    i, ref = R.act_inputs(case), R.evaluate("act", case)
    x, dy = _dev(i["x"]), _dev(i["dy"])
    counter, used = _i64(call), _i64(-1)
    y, dx = Out((n,), "bf16"), Out((n,), "bf16")
    assert lib.ops_act_dropout_fwd(n, x.data_ptr(), y.ptr, slope, p, R.SEED, counter.data_ptr(), used.data_ptr(), _stream()) == 0
    _used_ok(used, call, p)
    counter.fill_(call + 1)
    assert lib.ops_act_dropout_bwd(n, x.data_ptr(), dy.data_ptr(), dx.ptr, slope, p, R.SEED, used.data_ptr(), _stream()) == 0
    check("act.y", y.get(), ref["act.y"])
    check("act.dx", dx.get(), ref["act.dx"])
    if p == 0:                                               # nothing but one product and one rounding: bit for bit
        assert np.array_equal(y.bits, R.act_exact_bits(i["x"], slope)) and np.array_equal(dx.bits, R.act_exact_bits(i["x"], slope, i["dy"]))


@pytest.mark.parametrize("case", R.NOISE_CASES, ids=_ids)
def test_diffusion_noise(lib, case):
    rows, d = case
    i, ref = R.noise_inputs(case), R.evaluate("noise", case)
    x, t, eps, acp = (_dev(i[k]) for k in ("x", "t", "eps", "acp"))
    o = dict(xn32=Out((rows, d), "f32"), xn16=Out((rows, d), "bf16"), sa=Out((rows,), "f32"), sb=Out((rows,), "f32"))
    assert lib.ops_diffusion_noise(rows, d, x.data_ptr(), t.data_ptr(), eps.data_ptr(), acp.data_ptr(), o["xn32"].ptr, o["xn16"].ptr, o["sa"].ptr,
                                   o["sb"].ptr, _stream()) == 0
    for k, out in o.items():
        check("noise." + k, out.get(), ref["noise." + k])


@pytest.mark.parametrize("case", R.COMBINE_CASES, ids=_ids)
def test_diffusion_combine(lib, case):
    B, Nc, d, _ = case
    i, ref = R.combine_inputs(case), R.evaluate("comb", case)
    m, xn32, sa, sb, cls, pe = (_dev(i[k]) for k in ("m", "xn32", "sa", "sb", "cls", "pe"))
    g, g16 = (None if i[k] is None else _dev(i[k]) for k in ("g", "g16"))
    z, z16 = Out((B * (Nc + 1), d), "f32"), Out((B * (Nc + 1), d), "bf16")
    dm, dcls = Out((B * Nc, d), "bf16"), Out((d,), "f32", i["dcls0"])
    assert lib.ops_diffusion_combine_fwd(B, Nc, d, m.data_ptr(), xn32.data_ptr(), sa.data_ptr(), sb.data_ptr(), cls.data_ptr(), pe.data_ptr(), z.ptr,
                                         z16.ptr, _stream()) == 0
    assert lib.ops_diffusion_combine_bwd(B, Nc, d, _ptr(g), _ptr(g16), sa.data_ptr(), sb.data_ptr(), dm.ptr, dcls.ptr, _stream()) == 0
    check("comb.z", z.get(), ref["comb.z"])
    check("comb.z16", z16.get(), ref["comb.z16"])
    check("comb.dm", dm.get(), ref["comb.dm"])
    check("comb.dcls", dcls.get(), ref["comb.dcls"])


# ---------------------------------------------------------------------------------------------------------------------------------
def _wgrad_once(lib, case, det=False):
    T, N, K = case
    i, ref = R.wgrad_inputs(case), R.evaluate("wgrad", case, det=det)
    dY, X = _dev(i["dY"]), _dev(i["X"])
    dW, db = Out((N, K), "f32", i["dW0"]), Out((N,), "f32", i["dbias0"])
    assert lib.ops_linear_wgrad_accumulate(T, N, K, dY.data_ptr(), X.data_ptr(), dW.ptr, db.ptr, _stream()) == 0
    check("wgrad.dW", dW.get(), ref["wgrad.dW"])
    check("wgrad.dbias", db.get(), ref["wgrad.dbias"])


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=_ids)
def test_weight_gradient(lib, case):
    _wgrad_once(lib, case)


def test_weight_gradient_deterministic_option(lib):
    """One row split for all 1 025 rows."""
    from openpystruct_amd import _cabi
    before = _cabi.get_option("deterministic")
    _cabi.set_option("deterministic", 1)
    try:
        _wgrad_once(lib, (1025, 70, 65), det=True)
    finally:
        _cabi.set_option("deterministic", before)
    assert _cabi.get_option("deterministic") == before


def _strided(bits, ld, off):
    """A [T, C] bf16 matrix as rows of stride ld elements starting `off` elements into a 16-byte aligned buffer: (tensor, pointer)."""
    T, C = bits.shape
    host = np.full(off + T * ld + 8, R.SENT_BF16, dtype=np.uint16)
    host[off:off + T * ld].reshape(T, ld)[:, :C] = bits
    t = _dev(host)
    return t, t.data_ptr() + 2 * off


def test_weight_gradients_grouped_strided_and_misaligned(lib):
    """The five products in ONE launch: even ones with row strides that keep 16-byte alignment (vector loads of a strided view), odd
    ones with strides N + 3 / K + 5 from a base 2 bytes past a 16-byte boundary (element loads), and the K = 0 column-sum job."""
    from openpystruct_amd import _cabi
    probs, keep, outs = (_cabi.WgradProblem * (len(R.WGRAD_CASES) + 1))(), [], []
    for n, case in enumerate(R.WGRAD_CASES):
        T, N, K = case
        i = R.wgrad_inputs(case)
        ldy, ldx, off = (N + 3, K + 5, 1) if n % 2 else (-(-N // 8) * 8 + 8, -(-K // 8) * 8 + 16, 0)
        (ty, py), (tx, px) = _strided(i["dY"], ldy, off), _strided(i["X"], ldx, off)
        assert py % 16 == 2 * off and px % 16 == 2 * off
        dW, db = Out((N, K), "f32", i["dW0"]), Out((N,), "f32", i["dbias0"])
        keep += [ty, tx]
        outs.append((case, dW, db))
        pr = probs[n]
        pr.T, pr.N, pr.K, pr.dY, pr.X, pr.dW, pr.dbias, pr.ldy, pr.ldx = T, N, K, py, px, dW.ptr, db.ptr, ldy, ldx
    T, N = R.COLSUM_CASE
    c = R.colsum_inputs()
    M, out = _dev(c["M"]), Out((N,), "f32", c["out0"])
    pr = probs[len(R.WGRAD_CASES)]
    pr.T, pr.N, pr.K, pr.dY, pr.X, pr.dW, pr.dbias, pr.ldy, pr.ldx = T, N, 0, M.data_ptr(), None, out.ptr, None, 0, 0
    assert lib.ops_linear_wgrad_accumulate_group(len(probs), probs, _stream()) == 0
    for case, dW, db in outs:
        ref = R.evaluate("wgrad", case)
        check("wgrad.dW", dW.get(), ref["wgrad.dW"])
        check("wgrad.dbias", db.get(), ref["wgrad.dbias"])
    check("colsum.out", out.get(), R.evaluate("colsum", R.COLSUM_CASE)["colsum.out"])


# ---------------------------------------------------------------------------------------------------------------------------------
SUPPORT_GRID = [(S, H, dh) for S in range(1, 9) for H in (1, 2, 4, 8, 16, 32, 48, 64) for dh in (1, 4, 8, 15, 16, 20, 32)
                if H * dh <= 256 and (H * dh) % 8 == 0]


def test_attention_support_agreement(lib):
    """Both entry points over the grid with Bn = 1: what tfd_fused lets into the training path (attention_support) is accepted by
    both, its answer per direction IS the entry point's, and a refusal comes before any launch (the outputs keep their sentinel)."""
    from openpystruct_amd import _cabi, tfd_fused as TF
    qkv = torch.zeros(8 * 768, dtype=torch.int16, device=DEV)
    dctx = torch.zeros(8 * 256, dtype=torch.int16, device=DEV)

    def both(S, H, dh, ctx, dqkv):
        return (lib.ops_seq_attention_fwd(1, S, H, dh, qkv.data_ptr(), ctx.ptr, 0.0, R.SEED, None, None, _stream()),
                lib.ops_seq_attention_bwd(1, S, H, dh, qkv.data_ptr(), dctx.data_ptr(), dqkv.ptr, 0.0, R.SEED, None, _stream()))

    ctx, dqkv = Out((8, 256), "bf16"), Out((8, 768), "bf16")
    codes = {g: both(*g, ctx, dqkv) for g in SUPPORT_GRID}
    torch.cuda.synchronize()
    assert set(c for rc in codes.values() for c in rc) <= {_cabi.OK, _cabi.ERR_UNSUPPORTED}
    for g, (rf, rb) in codes.items():
        assert TF.attention_support(*g) == (rf == _cabi.OK, rb == _cabi.OK), (g, rf, rb)
    assert codes[(8, 64, 4)] == (_cabi.OK, _cabi.ERR_UNSUPPORTED) and codes[(8, 48, 4)] == (_cabi.OK, _cabi.ERR_UNSUPPORTED)
    assert codes[(5, 64, 4)] == (_cabi.OK, _cabi.OK)
    # the refusals once more into fresh sentinels: nothing is launched
    ctx, dqkv = Out((8, 256), "bf16"), Out((8, 768), "bf16")
    for g, (rf, rb) in codes.items():
        if rf != _cabi.OK and rb != _cabi.OK:
            assert both(*g, ctx, dqkv) == (rf, rb)
        elif rb != _cabi.OK:
            assert lib.ops_seq_attention_bwd(1, *g, qkv.data_ptr(), dctx.data_ptr(), dqkv.ptr, 0.0, R.SEED, None, _stream()) == rb
    ctx.get(untouched=True)
    dqkv.get(untouched=True)


@pytest.mark.parametrize("S,fast", [(8, False), (5, True)])
def test_layer_whose_backward_cannot_run_trains_through_the_framework(monkeypatch, S, fast):
    """d = 256, H = 64: eight tokens fit the forward kernel and not the backward one, so a training pass takes the framework's forward
    (and its backward runs); five tokens fit both and stay on the fast path."""
    import torch.nn as nn
    from openpystruct_amd import flat_adam, shadow, tfd_fused as TF
    torch.manual_seed(0)
    layer = nn.TransformerEncoderLayer(d_model=256, nhead=64, dim_feedforward=64, dropout=0.1, activation="relu", batch_first=True)
    enc = nn.TransformerEncoder(layer, num_layers=1).to(DEV)
    params = list(enc.parameters())
    flat = flat_adam.flat_grads(params, DEV)
    opt = flat_adam.FlatClipAdam(params, flat, 1e-3)
    stash, dst, patched = shadow.enable_shadow_linears(enc, opt, params, flat)
    assert TF.patch_encoder(enc, seed=5, direct_param_grads=True)
    calls = []
    inner = TF.encoder_forward
    monkeypatch.setattr(TF, "encoder_forward", lambda *a: calls.append(1) or inner(*a))
    x = torch.randn(4, S, 256, device=DEV, requires_grad=True)
    enc.train()
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = enc(x)
            out.float().square().mean().backward()
        torch.cuda.synchronize()
        assert bool(calls) == fast
        assert torch.isfinite(out).all() and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    finally:
        shadow.disable_shadow_linears(patched)
        TF.unpatch_encoder(enc)
