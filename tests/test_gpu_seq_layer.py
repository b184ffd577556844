"""The one-launch kernels of csrc/seq_layer.hip -- `ops_tfd_encoder_layer_fwd / _bwd` and their pair launches, `ops_tfd_head_fwd / _bwd`,
`ops_tfd_front_fwd / _bwd` -- ONE LAUNCH per comparison through the C ABI structures of `_cabi`, stage by stage against the float64
references of tests/seq_layer_ref.py at the protocols defined there (the same ones tests/test_seq_layer_reference.py runs in float32 on
the CPU).  Every element of every output is compared (none excluded); every output sits between two guard rows, pre-filled with a
sentinel (the `Out` class of tests/test_gpu_seq_block.py); every stage's inputs are what the launch itself stored for the stage before.
The fragment-tiled weights are built ON THE HOST (seq_layer_ref.tiled_weight); test_host_tiles_are_the_repack_launch's holds them to
`ops_mlp_repack_weights` bit for bit.

Errors are elementwise in units of unit x 2^-24 beyond the output's slack (seq_layer_ref's docstring).  "CPU": largest constant of the
float32 NumPy evaluation on these inputs; bound = 4 x the table's entry; "MI355X": largest value seen there (the module fixture's
teardown report).

  output         CPU  bound  MI355X   output         CPU  bound  MI355X   output         CPU  bound  MI355X
  lf.qkv        1.05    4.8    0.06   lb.dbeta2     2.11    9.6    1.56   hb.dcls       1.15    5.2    0.14
  lf.ctx        4.73   21.2    0.54   lb.d_u        1.08    5.0    0.17   hb.dgamma     0.82    3.8    0.00
  lf.z1         1.10    5.0    0.14   lb.d_a        0.49    2.2    0.00   hb.dbeta      0.91    4.2    0.00
  lf.mean1      1.40    6.4    1.40   lb.dgamma1    0.51    2.4    0.00   hb.loss       1.01    4.6    0.74
  lf.rstd1      0.58    2.6    0.54   lb.dbeta1     0.47    2.2    0.00   hb.loss_sum   0.96    4.4    0.98
  lf.y1_16      1.60    7.2    0.00   lb.dqkv       1.57    7.2    0.00   ff.sa         0.83    3.8    0.83
  lf.u          1.00    4.6    0.19   lb.dx32       0.32    1.6    0.00   ff.sb         0.84    3.8    0.84
  lf.h          1.73    7.8    0.00   hf.a16        0.87    4.0    0.00   ff.xn16       2.11    9.6    0.40
  lf.z2         1.02    4.6    1.23   hf.mean       0.34    1.6    0.34   ff.h          0.77    3.6    0.00
  lf.mean2      0.85    4.0    0.85   hf.rstd       0.52    2.4    0.43   ff.z          1.00    4.6    1.00
  lf.rstd2      0.52    2.4    0.53   hf.h          0.99    4.6    0.00   ff.z16        1.00    4.6    0.00
  lf.y32        1.66    7.6    1.54   hf.out        1.00    4.6    0.02   fb.dm         2.36   10.6    0.80
  lf.y16        1.66    7.6    0.02   hf.grad       3.11   14.0    0.00   fb.d_h        1.00    4.6    0.03
  lb.d_f        1.75    8.0    0.00   hf.parts      1.29    5.8    0.75   fb.dcls       1.48    6.8    2.03
  lb.dgamma2    1.41    6.4    0.70   hb.d_a        0.52    2.4    0.00

(A bf16 output shows its float32 error only at the few elements next to a rounding tie, hence the small MI355X figures of the bf16
outputs.  lb.d_a, lb.dgamma1, lb.dbeta1, lb.dqkv, lb.dx32, hb.d_a, hb.dgamma, hb.dbeta stand behind a product whose bf16 rounding is not
stored: its half ulp is their slack, and the device stays inside it everywhere.  No bound was widened.)

Protocol: the call counter is 0, 5 and 2^32 + 5 in turn down each table, every seed has bit 62 set; three dropout settings per layer case
(off, all sites 0.1, four probabilities with four seeds); the counter is changed between the forward and the backward launch, which takes
its masks from `used_call`; each backward runs in the atomic form on pre-filled dgamma / dbeta and in the ln_part form (dgamma / dbeta
untouched, columns >= d exactly zero, the rows' fixed-order sums at the totals' bound); the pair launches are bit-equal to the two single
launches (the atomic sums of several workgroups, which have no fixed order, are held to their stage's reference instead); the
self-assembled batch of the front end starts with cursor + B beyond n_order.

Defects found with these tests: none in csrc/seq_layer.hip or in the gates of tfd_fused.py.  Every accepted shape of the tables -- S = 1, 2,
3, 5, 6, dh = 1 and dh not a multiple of 4, d = 8 and d not a multiple of 16, ff not a multiple of 16, odd H -- meets its bounds, no output
uses more than 0.30 of its bound (fb.dcls; lf.z2 0.27), nothing is written outside an output, every refusal returns its
documented code with the outputs untouched.  Two observations that are no defects: `ops_mlp_repack_weights` writes the live elements
of Wp / Wtp only (the padding is the zeros the caller allocated; the optimiser's repack launch writes whole tiles), and a steep noise
schedule (alpha_cumprod ~ 4e-5 at T = 1000) gives |z| ~ 150, where a stored bf16 value can equal the sentinel of `Out` (-123.5): the
front end's inputs use a schedule that ends at 0.08.
"""
import ctypes
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import seq_layer_ref as R  # noqa: E402
from tests.test_gpu_mlp_block import Buf  # noqa: E402
from tests.test_gpu_seq_block import Out, _dev, _stream  # noqa: E402

DEV = "cuda"
WORST = {}                 # output -> largest error seen in units of unit x 2^-24, printed when the module is done
f32, f64 = np.float32, np.float64
_ids = lambda v: "-".join(map(str, v)).replace(" ", "").replace("(", "").replace(")", "")[:60] if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi
    yield _cabi.load()
    for name, e in sorted(WORST.items()):
        print(f"\nlargest error on the GPU, {name:12s} {e:7.2f} = {e / R.bound_constant(name):5.2f} of its bound {R.bound_constant(name):.2f}", end="")


def check(recs, what):
    """The records of a protocol: every comparison within 4 x CPU_CONST of its unit beyond the slack, every exact condition holds; the
    worst ratio per output is kept for the module's report."""
    ratios, failed = R.measure(recs)
    for n, e in ratios.items():
        WORST[n] = max(WORST.get(n, 0.0), e)
        print(f"{what} {n}: {e:.2f} of {R.bound_constant(n):.2f}")
    assert not failed, (what, failed)
    over = {n: (e, R.bound_constant(n)) for n, e in ratios.items() if not e <= R.bound_constant(n)}
    assert not over, (what, over)


def _out(name, shape, init=None):
    return Out(shape, "bf16" if name in R.BF16_OUTPUTS else "f32", init)


def _get(o):
    """An Out's content in storage form: bf16 bit patterns or float32 (guards checked, every element written)."""
    v = o.get()
    return o.bits.copy() if o.bf16 else v.astype(f32)


class GpuImpl:
    """The launches of seq_layer_ref's protocols through the C ABI."""

    def __init__(self, lib):
        from openpystruct_amd import _cabi
        self.lib, self.cabi, self.keep = lib, _cabi, []

    def dev(self, host):
        t = _dev(host)
        self.keep.append(t)
        assert t.data_ptr() % 16 == 0
        return t.data_ptr()

    # ---- the encoder layer ----
    def layer_fwd_args(self, a, x_ptr=None):
        Bn, S, H, dh, ff = a["case"]
        d, T = H * dh, Bn * S
        s = self.cabi.TfdLayerArgs()
        s.Bn, s.S, s.H, s.dh, s.d, s.ff = Bn, S, H, dh, d, ff
        s.x32 = x_ptr if x_ptr is not None else self.dev(a["x32"])
        for n in ("W_in", "W_out", "W_1", "W_2"):
            setattr(s, n, self.dev(R.tiled_weight(a[n])))
        for n in ("b_in", "b_out", "b_1", "b_2", "gamma1", "beta1", "gamma2", "beta2"):
            setattr(s, n, self.dev(a[n]))
        s.eps1 = s.eps2 = a["eps"]
        s.p_attn, s.p_1, s.p_act, s.p_2 = a["p"]
        s.seed_attn, s.seed_1, s.seed_act, s.seed_2 = a["seeds"]
        counter, used = torch.tensor([a["call"]], dtype=torch.int64, device=DEV), torch.tensor([-1], dtype=torch.int64, device=DEV)
        s.counter, s.used_call = counter.data_ptr(), used.data_ptr()
        self.keep += [counter, used]
        shapes = {"qkv": (T, 3 * d), "ctx": (T, d), "z1": (T, d), "mean1": (T,), "rstd1": (T,), "y1_16": (T, d), "u": (T, ff), "h": (T, ff), "z2": (T, d),
                  "mean2": (T,), "rstd2": (T,), "y32": (T, d), "y16": (T, d)}
        outs = {n: _out("lf." + n, sh) for n, sh in shapes.items()}
        for n, o in outs.items():
            setattr(s, n, o.ptr)
        return s, outs, counter, used

    def layer_fwd(self, a):
        s, outs, counter, used = self.layer_fwd_args(a)
        assert self.lib.ops_tfd_encoder_layer_fwd(ctypes.byref(s), _stream()) == 0
        st = {"lf." + n: _get(o) for n, o in outs.items()}
        st["used_call"] = int(used.item())
        assert int(counter.item()) == a["call"], "the counter is only read"
        counter.fill_(a["call"] + 1)                          # the backward must take its masks from used_call, not from the counter
        st["_used"] = used
        return st

    def layer_bwd_args(self, a, sv, grads, ln_part, g32_ptr=None):
        Bn, S, H, dh, ff = a["case"]
        d, T = H * dh, Bn * S
        s = self.cabi.TfdLayerBwdArgs()
        s.Bn, s.S, s.H, s.dh, s.d, s.ff = Bn, S, H, dh, d, ff
        if grads in ("both", "g32"):
            s.g32 = g32_ptr if g32_ptr is not None else self.dev(a["g32"])
        if grads in ("both", "g16"):
            s.g16 = self.dev(a["g16"])
        for n, w in (("Wt_in", "W_in"), ("Wt_out", "W_out"), ("Wt_1", "W_1"), ("Wt_2", "W_2")):
            setattr(s, n, self.dev(R.tiled_weight_t(a[w])))
        s.gamma1, s.gamma2 = self.dev(a["gamma1"]), self.dev(a["gamma2"])
        s.p_attn, s.p_1, s.p_act, s.p_2 = a["p"]
        s.seed_attn, s.seed_1, s.seed_act, s.seed_2 = a["seeds"]
        used = sv["_used"] if "_used" in sv else torch.tensor([sv["used_call"]], dtype=torch.int64, device=DEV)
        self.keep.append(used)
        s.used_call = used.data_ptr()
        for n in ("qkv", "z1", "mean1", "rstd1", "u", "z2", "mean2", "rstd2"):
            setattr(s, n, self.dev(sv["lf." + n]))
        outs = {"d_f": _out("lb.d_f", (T, d)), "d_u": _out("lb.d_u", (T, ff)), "d_a": _out("lb.d_a", (T, d)), "dqkv": _out("lb.dqkv", (T, 3 * d)),
                "dx32": _out("lb.dx32", (T, d))}
        for j, n in enumerate(("dgamma2", "dbeta2", "dgamma1", "dbeta1")):
            outs[n] = Out((d,), "f32", a["dg0"][j])
        for n, o in outs.items():
            setattr(s, n, o.ptr)
        if ln_part:
            outs["part"] = Out((len(R.layer_tiles(Bn, S)), 4, 128), "f32")
            s.ln_part = outs["part"].ptr
        return s, outs

    def layer_bwd(self, a, sv, grads, ln_part):
        s, outs = self.layer_bwd_args(a, sv, grads, ln_part)
        assert self.lib.ops_tfd_encoder_layer_bwd(ctypes.byref(s), _stream()) == 0
        return {"lb." + n: _get(o) for n, o in outs.items()}

    # ---- the head ----
    def head_fwd_args(self, a):
        B, S, d, hid, C = a["case"]
        s = self.cabi.TfdHeadArgs()
        s.B, s.S, s.d, s.hid, s.C = B, S, d, hid, C
        s.y16, s.W1, s.W2 = self.dev(a["y16"]), self.dev(R.tiled_weight(a["W1"])), self.dev(R.tiled_weight(a["W2"]))
        s.b1, s.b2, s.gamma, s.beta, s.eps = self.dev(a["b1"]), self.dev(a["b2"]), self.dev(a["gamma"]), self.dev(a["beta"]), a["eps"]
        s.p_drop, s.seed = a["p"], a["seed"]
        counter, used = torch.tensor([a["call"]], dtype=torch.int64, device=DEV), torch.tensor([-1], dtype=torch.int64, device=DEV)
        s.counter, s.used_call = counter.data_ptr(), used.data_ptr()
        outs = {"a16": _out("hf.a16", (B, hid)), "mean": _out("hf.mean", (B,)), "rstd": _out("hf.rstd", (B,)), "h": _out("hf.h", (B, hid)),
                "out": _out("hf.out", (B, C))}
        parts = None
        if a["loss"] is not None:
            outs["grad"] = _out("hf.grad", (B, C))
            parts = Buf(np.full(5 * len(R.head_tiles(B)), -7.5, dtype=f64))
            s.targets, s.loss_part, s.alpha, s.box_weight = self.dev(a["targets"]), parts.ptr, self.dev(np.array([a["alpha"]], dtype=f32)), a["box_w"]
            if a["lo"] is not None:
                s.min_constraint, s.max_constraint = self.dev(np.array([a["lo"]], dtype=f32)), self.dev(np.array([a["hi"]], dtype=f32))
            if a["target_rows"] is not None:
                s.target_rows = self.dev(a["target_rows"])
        for n, o in outs.items():
            setattr(s, n, o.ptr)
        self.keep += [counter, used]
        return s, outs, dict(parts=parts, used=used)

    def head_fwd(self, a):
        s, outs, x = self.head_fwd_args(a)
        assert self.lib.ops_tfd_head_fwd(ctypes.byref(s), _stream()) == 0
        torch.cuda.synchronize()
        st = {"hf." + n: _get(o) for n, o in outs.items()}
        st["used_call"] = int(x["used"].item())
        if x["parts"] is not None:
            st["hf.parts"] = x["parts"].get().reshape(-1, 5)
            assert not st["hf.parts"][:, 3:].any(), "the two unused partial sums are zero"
        return st

    def head_bwd_args(self, a, sv, with_g2, ln_part, loss_parts=None):
        B, S, d, hid, C = a["case"]
        s = self.cabi.TfdHeadBwdArgs()
        s.B, s.S, s.d, s.hid, s.C = B, S, d, hid, C
        s.g, s.Wt2, s.Wt1, s.gamma, s.p_drop = self.dev(a["g"]), self.dev(R.tiled_weight_t(a["W2"])), self.dev(R.tiled_weight_t(a["W1"])), self.dev(a["gamma"]), a["p"]
        for n in ("a16", "mean", "rstd", "h"):
            setattr(s, n, self.dev(sv["hf." + n]))
        outs = {"d_a": _out("hb.d_a", (B, hid)), "dgamma": Out((hid,), "f32", a["dg0"][0]), "dbeta": Out((hid,), "f32", a["dg0"][1])}
        rows = Buf(np.full((B * S, d), R.SENT_BF16, dtype=np.uint16))
        s.dcls_rows = rows.ptr
        gsum = None
        if with_g2:
            gsum = _out("hf.grad", (B, C))
            s.g2, s.g_sum = self.dev(a["g2"]), gsum.ptr
        if ln_part:
            outs["part"] = Out((len(R.head_tiles(B)), 2, hid), "f32")
            s.ln_part = outs["part"].ptr
        loss = None
        if loss_parts is not None:
            loss = Buf(np.array([R.SENT_F32, R.SUM0], dtype=f32))
            s.loss_part, s.alpha, s.alpha0, s.box_weight = self.dev(np.asarray(loss_parts, dtype=f64).ravel()), self.dev(np.array([a["alpha"]], dtype=f32)), a["alpha0"], a["box_w"]
            s.loss, s.loss_sum = loss.ptr, loss.ptr + 4
        for n, o in outs.items():
            setattr(s, n, o.ptr)
        return s, outs, dict(rows=rows, gsum=gsum, loss=loss)

    def head_bwd(self, a, sv, with_g2, ln_part, loss_parts=None):
        B, S = a["case"][:2]
        s, outs, x = self.head_bwd_args(a, sv, with_g2, ln_part, loss_parts)
        rows, gsum, loss = x["rows"], x["gsum"], x["loss"]
        assert self.lib.ops_tfd_head_bwd(ctypes.byref(s), _stream()) == 0
        torch.cuda.synchronize()
        st = {"hb." + n: _get(o) for n, o in outs.items()}
        st["hb.dcls_rows"] = rows.get()
        st["hb.dcls"] = st["hb.dcls_rows"][np.arange(B) * S].copy()
        if gsum is not None:
            st["hb.gsum"] = _get(gsum)
        if loss is not None:
            st["hb.loss"], st["hb.loss_sum"] = loss.get()
        return st

    # ---- the diffusion front end ----
    def front_fwd_args(self, a):
        B, Nc, d, hid, T = a["case"]
        rows = B * Nc
        s = self.cabi.TfdFrontArgs()
        s.B, s.Nc, s.d, s.hid, s.T = B, Nc, d, hid, T
        s.alpha_cumprod, s.seed = self.dev(a["acp"]), a["seed"]
        counter = Buf(np.array([a["call"], 0], dtype=np.uint64))
        s.counter = counter.ptr
        s.W0, s.W2, s.b0, s.b2 = self.dev(R.tiled_weight(a["W0"])), self.dev(R.tiled_weight(a["W2"])), self.dev(a["b0"]), self.dev(a["b2"])
        s.cls, s.pe = self.dev(a["cls"]), self.dev(a["pe"])
        outs = {"xn16": _out("ff.xn16", (rows, d)), "h": _out("ff.h", (rows, hid)), "sa": _out("ff.sa", (rows,)), "sb": _out("ff.sb", (rows,)),
                "z": _out("ff.z", (B * (Nc + 1), d)), "z16": _out("ff.z16", (B * (Nc + 1), d)), "eps_out": Out((rows, d), "f32")}
        for n, o in outs.items():
            setattr(s, n, o.ptr)
        t_out = Buf(np.full(rows, -1, dtype=np.int64))
        s.t_out = t_out.ptr
        cursor = idx = None
        if a["own"]:
            cursor, idx = Buf(np.array([a["cursor"]], dtype=np.int64)), Buf(np.full(B, -1, dtype=np.int64))
            s.src, s.order, s.cursor, s.idx_out = self.dev(a["src"]), self.dev(a["order"]), cursor.ptr, idx.ptr
            s.sigma, s.in_seed, s.n_order = self.dev(np.array([a["sigma"]], dtype=f32)), a["in_seed"], a["n_order"]
        else:
            s.x = self.dev(a["x"])
        return s, outs, dict(counter=counter, t_out=t_out, cursor=cursor, idx=idx)

    def front_fwd(self, a):
        B, Nc, d, hid, T = a["case"]
        s, outs, x = self.front_fwd_args(a)
        counter, t_out, cursor, idx = x["counter"], x["t_out"], x["cursor"], x["idx"]
        assert self.lib.ops_tfd_front_fwd(ctypes.byref(s), _stream()) == 0
        torch.cuda.synchronize()
        st = {"ff." + n: _get(o) for n, o in outs.items() if n != "eps_out"}
        st["ff.z"], st["ff.z16"] = st["ff.z"].reshape(B, Nc + 1, d), st["ff.z16"].reshape(B, Nc + 1, d)
        st["ff.eps"], st["ff.t"] = _get(outs["eps_out"]), t_out.get()
        st["counter"] = tuple(int(v) for v in counter.get())
        if a["own"]:
            st["ff.idx"], st["cursor"] = idx.get(), int(cursor.get()[0])
        return st

    def front_bwd_args(self, a, sv, grads, with_dcls):
        B, Nc, d, hid, T = a["case"]
        rows = B * Nc
        s = self.cabi.TfdFrontBwdArgs()
        s.B, s.Nc, s.d, s.hid = B, Nc, d, hid
        if grads in ("both", "g32"):
            s.g32 = self.dev(a["g32"])
        if grads in ("both", "g16"):
            s.g16 = self.dev(a["g16"])
        s.sa, s.sb, s.h, s.Wt2 = self.dev(sv["ff.sa"]), self.dev(sv["ff.sb"]), self.dev(sv["ff.h"]), self.dev(R.tiled_weight_t(a["W2"]))
        outs = {"dm": _out("fb.dm", (rows, d)), "d_h": _out("fb.d_h", (rows, hid))}
        if with_dcls:
            outs["dcls"] = Out((d,), "f32", a["dcls0"])
        for n, o in outs.items():
            setattr(s, n, o.ptr)
        return s, outs, {}

    def front_bwd(self, a, sv, grads, with_dcls):
        s, outs, _ = self.front_bwd_args(a, sv, grads, with_dcls)
        assert self.lib.ops_tfd_front_bwd(ctypes.byref(s), _stream()) == 0
        return {"fb." + n: _get(o) for n, o in outs.items()}


@pytest.fixture()
def impl(lib):
    return GpuImpl(lib)


# ---------------------------------------------------------------------------------------------------------------------------------
# every launch against its float64 reference, stage by stage
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,drop", R.PROTOCOLS["layer"][1], ids=_ids)
def test_layer(impl, case, drop):
    check(R.layer_protocol(case, drop, impl), f"layer {case} {drop}")


@pytest.mark.parametrize("case,p", R.PROTOCOLS["head"][1], ids=_ids)
def test_head(impl, case, p):
    check(R.head_protocol(case, p, impl), f"head {case} p={p}")


@pytest.mark.parametrize("case,own", R.PROTOCOLS["front"][1], ids=_ids)
def test_front(impl, case, own):
    check(R.front_protocol(case, own, impl), f"front {case} own={own}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the pair launches: every output bit-equal to the two single launches, both directions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,ff2", R.PAIR_CASES, ids=_ids)
def test_pair_launches_are_the_two_single_launches(impl, lib, case, ff2):
    k = R.PAIR_CASES.index((case, ff2))
    drop = list(R.DROPOUTS)[(k + 1) % 3]
    la, lb_ = R.layer_inputs(case, drop), R.layer_inputs(case, drop, ff2=ff2, key=1)
    lb_ = dict(lb_, call=la["call"])
    # forward: two launches, layer b reading layer a's float32 output where it lies
    sa, oa, _, ua = impl.layer_fwd_args(la)
    sb_, ob, _, ub = impl.layer_fwd_args(lb_, x_ptr=oa["y32"].ptr)
    assert lib.ops_tfd_encoder_layer_fwd(ctypes.byref(sa), _stream()) == 0
    assert lib.ops_tfd_encoder_layer_fwd(ctypes.byref(sb_), _stream()) == 0
    single = [{n: _get(o) for n, o in outs.items()} for outs in (oa, ob)]
    pa, poa, _, pua = impl.layer_fwd_args(la)
    pb, pob, _, pub = impl.layer_fwd_args(lb_, x_ptr=poa["y32"].ptr)
    assert lib.ops_tfd_encoder_layer_pair_fwd(ctypes.byref(pa), ctypes.byref(pb), _stream()) == 0
    for outs, want in zip((poa, pob), single):
        for n, o in outs.items():
            assert np.array_equal(_get(o).view(np.uint8), want[n].view(np.uint8)), ("forward", n)
    assert int(pua.item()) == int(pub.item()) == la["call"] == int(ua.item()) == int(ub.item())
    # backward: `later` = layer b, `earlier` = layer a on the float32 dx the later one has written
    sv = [dict({"lf." + n: v for n, v in s_.items()}, used_call=la["call"]) for s_ in single]
    grads = R.GRADS[k % 3]
    for ln_part in (False, True):
        s2, o2 = impl.layer_bwd_args(lb_, sv[1], grads, ln_part)
        s1, o1 = impl.layer_bwd_args(la, sv[0], "g32", ln_part, g32_ptr=o2["dx32"].ptr)
        assert lib.ops_tfd_encoder_layer_bwd(ctypes.byref(s2), _stream()) == 0
        assert lib.ops_tfd_encoder_layer_bwd(ctypes.byref(s1), _stream()) == 0
        want = [{n: _get(o) for n, o in outs.items()} for outs in (o2, o1)]
        p2, q2 = impl.layer_bwd_args(lb_, sv[1], grads, ln_part)
        p1, q1 = impl.layer_bwd_args(la, sv[0], "g32", ln_part, g32_ptr=q2["dx32"].ptr)
        assert lib.ops_tfd_encoder_layer_pair_bwd(ctypes.byref(p2), ctypes.byref(p1), _stream()) == 0
        atomics = not ln_part and len(R.layer_tiles(case[0], case[1])) > 1
        for which, (outs, w) in enumerate(zip((q2, q1), want)):
            got = {n: _get(o) for n, o in outs.items()}
            for n in outs:
                if atomics and n.startswith(("dgamma", "dbeta")):
                    continue                                   # float atomics of several workgroups: no fixed order of the additions (below)
                assert np.array_equal(got[n].view(np.uint8), w[n].view(np.uint8)), ("backward", n, ln_part)
            if atomics:
                # ... so the pair's sums are held to the float64 reference of their stage instead, at the bound of the single launch
                lay, sv_, gr = (lb_, sv[1], grads) if which == 0 else (dict(la, g32=want[0]["dx32"]), sv[0], "g32")
                bw = {"lb." + n: v for n, v in got.items()}
                check(R._cmp([], bw, R.layer_bwd(lay, sv_, gr, False, f64, (), bw), R.PART_NAMES), f"pair bwd {case}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the host tiles are what the repack launch writes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_host_tiles_are_the_repack_launch(impl, lib):
    rng = np.random.default_rng(5)
    shapes = [(24, 8), (8, 24), (16, 120), (360, 120), (248, 48), (100, 256), (136, 40), (4, 16)]
    ent = (impl.cabi.MlpRepackEntry * len(shapes))()
    bufs = []
    for e, (N, K) in zip(ent, shapes):
        w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(f32)
        wp = Buf(np.zeros((R.ru(N, 16), R.ru(K, 32)), dtype=np.uint16))      # (the stand-alone launch writes the live elements; the padding is the caller's zeros)
        wtp = Buf(np.zeros((R.ru(K, 16), R.ru(N, 32)), dtype=np.uint16))
        e.W, e.N, e.K, e.Wp, e.ldw, e.Wtp, e.ldwt = impl.dev(w), N, K, wp.ptr, R.ru(K, 32), wtp.ptr, R.ru(N, 32)
        bufs.append((w, wp, wtp))
    assert lib.ops_mlp_repack_weights(len(shapes), ent, _stream()) == 0
    torch.cuda.synchronize()
    for (N, K), (w, wp, wtp) in zip(shapes, bufs):
        bits = R.bf16_bits(w)
        assert np.array_equal(wp.get(), R.tiled_weight(bits)), ("Wp", N, K)
        assert np.array_equal(wtp.get(), R.tiled_weight_t(bits)), ("Wtp", N, K)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: the documented error, and no output touched
# ---------------------------------------------------------------------------------------------------------------------------------
def _untouched(outs):
    torch.cuda.synchronize()
    for o in outs:
        if isinstance(o, Out):
            if o.added:
                assert np.array_equal(o.buf.cpu().numpy()[o.guard:o.guard + o.n], np.asarray(o.init_host, dtype=f32).ravel()), "a refused call wrote an output"
            else:
                o.get(untouched=True)
        else:
            assert o.unchanged(), "a refused call wrote an output"


def _sizes(**kw):
    return lambda s: [setattr(s, k, v) for k, v in kw.items()]


def _off8(field):
    return lambda s: setattr(s, field, getattr(s, field) + 8)


def _null(field):
    return lambda s: setattr(s, field, None)


LAYER_SIZE_REFUSALS = [("S=9", _sizes(S=9)), ("H=9", _sizes(H=9, dh=8, d=72)), ("dh=17, d=136", _sizes(H=8, dh=17, d=136)),
                       ("d=12", _sizes(H=1, dh=12, d=12)), ("d!=H*dh", _sizes(d=24)), ("ff=8", _sizes(ff=8)), ("ff=264", _sizes(ff=264)), ("ff=20", _sizes(ff=20))]
LAYER_FWD_PTRS = ["x32", "W_in", "b_in", "W_out", "b_out", "W_1", "b_1", "W_2", "b_2", "gamma1", "beta1", "gamma2", "beta2", "counter", "qkv", "ctx", "z1",
                  "mean1", "rstd1", "y1_16", "u", "h", "z2", "mean2", "rstd2", "y32", "y16"]
LAYER_BWD_PTRS = ["Wt_in", "Wt_out", "Wt_1", "Wt_2", "gamma1", "gamma2", "used_call", "qkv", "z1", "mean1", "rstd1", "u", "z2", "mean2", "rstd2", "d_f", "d_u",
                  "d_a", "dqkv", "dx32", "dgamma1", "dbeta1", "dgamma2", "dbeta2"]


def _remember_inits(outs):
    for o in outs:
        if isinstance(o, Out) and o.added:
            o.init_host = o.buf.cpu().numpy()[o.guard:o.guard + o.n].copy()
    return outs


def test_layer_refusals(impl, lib):
    U, I = impl.cabi.ERR_UNSUPPORTED, impl.cabi.ERR_INVALID_ARG
    a = R.layer_inputs((3, 2, 4, 10, 16), "p01")
    sv = {k: v for k, v in R.CpuImpl().layer_fwd(a).items() if k != "twin"}
    muts = [(n, m, U) for n, m in LAYER_SIZE_REFUSALS]
    fwd = muts + [(f"{w}+8", _off8(w), U) for w in ("W_in", "W_out", "W_1", "W_2")] + [(f"{p} NULL", _null(p), I) for p in LAYER_FWD_PTRS]
    for name, mut, want in fwd:
        s, outs, _, used = impl.layer_fwd_args(a)
        mut(s)
        assert lib.ops_tfd_encoder_layer_fwd(ctypes.byref(s), _stream()) == want, ("fwd", name)
        s2, outs2, _, _ = impl.layer_fwd_args(a, x_ptr=outs["y32"].ptr)
        assert lib.ops_tfd_encoder_layer_pair_fwd(ctypes.byref(s), ctypes.byref(s2), _stream()) == want, ("pair fwd, first", name)
        _untouched(list(outs.values()) + list(outs2.values()))
        assert int(used.item()) == -1
    bwd = muts + [(f"{w}+8", _off8(w), U) for w in ("Wt_in", "Wt_out", "Wt_1", "Wt_2")] + [(f"{p} NULL", _null(p), I) for p in LAYER_BWD_PTRS] + \
        [("both gradients NULL", lambda s: (setattr(s, "g32", None), setattr(s, "g16", None)), I)]
    for name, mut, want in bwd:
        s, outs = impl.layer_bwd_args(a, sv, "both", False)
        mut(s)
        _remember_inits(outs.values())
        assert lib.ops_tfd_encoder_layer_bwd(ctypes.byref(s), _stream()) == want, ("bwd", name)
        s1, outs1 = impl.layer_bwd_args(a, sv, "g32", False, g32_ptr=outs["dx32"].ptr)
        _remember_inits(outs1.values())
        assert lib.ops_tfd_encoder_layer_pair_bwd(ctypes.byref(s), ctypes.byref(s1), _stream()) == want, ("pair bwd, later", name)
        _untouched(list(outs.values()) + list(outs1.values()))
    # a pair whose second layer does not read the first one's output / gradient
    s, outs, _, _ = impl.layer_fwd_args(a)
    s2, outs2, _, _ = impl.layer_fwd_args(a)
    assert lib.ops_tfd_encoder_layer_pair_fwd(ctypes.byref(s), ctypes.byref(s2), _stream()) == I
    _untouched(list(outs.values()) + list(outs2.values()))
    s, outs = impl.layer_bwd_args(a, sv, "both", False)
    s1, outs1 = impl.layer_bwd_args(a, sv, "g32", False)
    _remember_inits(list(outs.values()) + list(outs1.values()))
    assert lib.ops_tfd_encoder_layer_pair_bwd(ctypes.byref(s), ctypes.byref(s1), _stream()) == I
    _untouched(list(outs.values()) + list(outs1.values()))


def test_head_and_front_refusals(impl, lib):
    U, I = impl.cabi.ERR_UNSUPPORTED, impl.cabi.ERR_INVALID_ARG
    a = R.head_inputs((5, 2, 24, 40, 20), 0.3, dict(rows=True, box=True, alpha0=0.5))
    sv = {k: v for k, v in R.CpuImpl().head_fwd(a).items() if k != "twin"}
    f = R.front_inputs((5, 3, 64, 72, 1000), False)
    fsv = {k: v for k, v in R.CpuImpl().front_fwd(f).items() if k != "twin"}
    sizes = [("d=136", _sizes(d=136)), ("d=12", _sizes(d=12)), ("hid=8", _sizes(hid=8)), ("hid=264", _sizes(hid=264)), ("hid=20", _sizes(hid=20))]
    head_sizes = sizes + [("C=6", _sizes(C=6)), ("C=132", _sizes(C=132))]
    nulls = lambda names: [(f"{p} NULL", _null(p), I) for p in names]      # noqa: E731
    plan = [
        ("head fwd", lib.ops_tfd_head_fwd, lambda: impl.head_fwd_args(a), [(n, m, U) for n, m in head_sizes] + [(f"{w}+8", _off8(w), U) for w in ("W1", "W2")] +
         nulls(("y16", "W1", "b1", "gamma", "beta", "W2", "b2", "counter", "a16", "mean", "rstd", "h", "out", "grad", "loss_part", "alpha"))),
        ("head bwd", lib.ops_tfd_head_bwd, lambda: impl.head_bwd_args(a, sv, True, True, sv["hf.parts"]), [(n, m, U) for n, m in head_sizes] +
         [(f"{w}+8", _off8(w), U) for w in ("Wt1", "Wt2")] +
         nulls(("g", "Wt2", "Wt1", "gamma", "a16", "mean", "rstd", "h", "d_a", "dcls_rows", "dgamma", "dbeta", "alpha", "loss"))),
        ("front fwd", lib.ops_tfd_front_fwd, lambda: impl.front_fwd_args(f), [(n, m, U) for n, m in sizes] + [(f"{w}+8", _off8(w), U) for w in ("W0", "W2")] +
         nulls(("x", "alpha_cumprod", "counter", "W0", "b0", "W2", "b2", "cls", "pe", "xn16", "h", "sa", "sb", "z", "z16"))),
        ("front bwd", lib.ops_tfd_front_bwd, lambda: impl.front_bwd_args(f, fsv, "both", True), [(n, m, U) for n, m in sizes] + [("Wt2+8", _off8("Wt2"), U)] +
         nulls(("sa", "sb", "h", "Wt2", "dm", "d_h")) + [("both gradients NULL", lambda s: (setattr(s, "g32", None), setattr(s, "g16", None)), I)]),
    ]
    for what, entry, build, muts in plan:
        for name, mut, want in muts:
            n_keep = len(impl.keep)
            s, outs, extra = build()
            written = list(outs.values()) + [b for b in extra.values() if isinstance(b, Buf)]
            _remember_inits(written)
            mut(s)
            assert entry(ctypes.byref(s), _stream()) == want, (what, name)
            _untouched(written)
            del impl.keep[n_keep:]
    # deterministic mode: the head's backward needs ln_part
    s, outs, extra = impl.head_bwd_args(a, sv, False, False)
    written = list(outs.values()) + [extra["rows"]]
    _remember_inits(written)
    impl.cabi.set_option("deterministic", 1)
    try:
        assert lib.ops_tfd_head_bwd(ctypes.byref(s), _stream()) == I
    finally:
        impl.cabi.set_option("deterministic", 0)
    _untouched(written)
    assert lib.ops_tfd_head_bwd(ctypes.byref(s), _stream()) == 0       # the same block outside that mode
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# deterministic mode: the same launch twice gives the same bits (front end's dcls in one workgroup, the partial-sum forms)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_deterministic_mode_front_dcls_is_reproducible_and_within_its_bound(impl):
    case = (16, 1, 8, 16, 10)
    a = R.front_inputs(case, False)
    fw = impl.front_fwd(a)
    impl.cabi.set_option("deterministic", 1)
    try:
        one, two = (impl.front_bwd(a, fw, "both", True) for _ in range(2))
    finally:
        impl.cabi.set_option("deterministic", 0)
    assert np.array_equal(one["fb.dcls"], two["fb.dcls"])
    ref = R.front_bwd(a, fw, "both", f64, (), one)
    check(R._cmp([], one, ref), "front bwd, deterministic")


# ---------------------------------------------------------------------------------------------------------------------------------
# the host gates never admit a size a C entry refuses
# ---------------------------------------------------------------------------------------------------------------------------------
def test_host_gates_admit_no_size_the_entries_refuse(impl, lib, monkeypatch):
    from openpystruct_amd import tfd_fused
    nn = torch.nn
    U, I = impl.cabi.ERR_UNSUPPORTED, impl.cabi.ERR_INVALID_ARG
    for sw in ("LAYER_FWD", "HEAD", "FRONT", "DRAW"):
        monkeypatch.setattr(tfd_fused, sw, True)
    rec = types.SimpleNamespace(rec=types.SimpleNamespace(b_sh=object()))
    st = types.SimpleNamespace(direct=True)

    def param(n):
        p = nn.Parameter(torch.zeros(n))
        p.grad = torch.zeros(n)
        return p

    def linear(i, o):
        m = nn.Linear(i, o)
        m._ops_prod = rec
        return m

    def accepted(entry, s):
        rc = entry(ctypes.byref(s), None)                     # every pointer NULL: a size the entry takes ends at the pointer check, nothing is launched
        assert rc in (U, I), rc
        return rc == I

    admitted = 0
    for d in (4, 8, 12, 16, 24, 64, 120, 128, 136, 144, 256):
        for H in (1, 2, 3, 7, 8, 9, 16):
            if d % H:
                continue
            for ff in (8, 16, 20, 24, 136, 256, 264, 512):
                mha = types.SimpleNamespace(embed_dim=d, num_heads=H, _ops_in_proj=rec, _ops_out_proj=rec)
                norm = lambda: types.SimpleNamespace(weight=param(d), bias=param(d))      # noqa: E731
                layer = types.SimpleNamespace(self_attn=mha, linear1=types.SimpleNamespace(out_features=ff, _ops_prod=rec), linear2=types.SimpleNamespace(_ops_prod=rec),
                                              _ops_tiles={}, norm1=norm(), norm2=norm())
                if tfd_fused._layer_fused_ok(layer, st):
                    admitted += 1
                    for S in (1, 7, 8):
                        s, b = impl.cabi.TfdLayerArgs(), impl.cabi.TfdLayerBwdArgs()
                        for q in (s, b):
                            q.Bn, q.S, q.H, q.dh, q.d, q.ff = 3, S, H, d // H, d, ff
                        assert accepted(lib.ops_tfd_encoder_layer_fwd, s) and accepted(lib.ops_tfd_encoder_layer_bwd, b), ("layer", d, H, ff, S)
        for hid in (8, 16, 20, 24, 72, 256, 264):
            for C in (2, 4, 6, 12, 100, 128, 132):
                enc = types.SimpleNamespace(_ops_extra_tiles={"fc1": 1, "fc2": 1, "mlp0": 1, "mlp2": 1})
                ln = types.SimpleNamespace(weight=param(hid), bias=param(hid))
                model = types.SimpleNamespace(fc1=linear(d, hid), fc2=linear(hid, C), norm1=ln, transformer_encoder=enc,
                                              diffusion=types.SimpleNamespace(mlp=[linear(d, hid), nn.ReLU(), linear(hid, d)]), cls_token=param(d),
                                              pos_encoder=types.SimpleNamespace(pe=torch.zeros(9, d)))
                if tfd_fused._head_fused_ok(model, st, d):
                    admitted += 1
                    s, b = impl.cabi.TfdHeadArgs(), impl.cabi.TfdHeadBwdArgs()
                    for q in (s, b):
                        q.B, q.S, q.d, q.hid, q.C = 5, 7, d, hid, C
                    assert accepted(lib.ops_tfd_head_fwd, s) and accepted(lib.ops_tfd_head_bwd, b), ("head", d, hid, C)
                if C == 4 and tfd_fused._front_fused_ok(model, st, d):
                    admitted += 1
                    s, b = impl.cabi.TfdFrontArgs(), impl.cabi.TfdFrontBwdArgs()
                    for q in (s, b):
                        q.B, q.Nc, q.d, q.hid = 5, 6, d, hid
                    s.T = 1000
                    assert accepted(lib.ops_tfd_front_fwd, s) and accepted(lib.ops_tfd_front_bwd, b), ("front", d, hid)
    assert admitted > 50            # the gates were exercised, not bypassed
