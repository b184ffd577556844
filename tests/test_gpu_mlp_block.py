"""The PINN layer-block launches of csrc/mlp_block.hip -- `ops_mlp_strip_launch` in every compiled combination and through the generic
kernel, `ops_mlp_wgrad_group[_norm]` -- ONE LAUNCH per comparison through the C ABI on torch-allocated buffers, against the float64
references of tests/mlp_block_ref.py at the protocols defined there (the same ones tests/test_mlp_block_reference.py runs in float32
on the CPU).  Every element of every output is compared (none excluded); every output is pre-filled with a sentinel between two
guards; rows 0..127 x columns 0..(N r.u. 16) - 1 of a tiled output must hold the reference in the live corner and zeros elsewhere,
every other byte of the buffer and both guards must be untouched, every input unchanged; columns of an operand past K r.u. 32 hold the
sentinel (a leading dimension 32 larger is never read past the reduction length).  After a drawing launch the call counter is
counter + 1 with a cleared tally, after any other launch it is unchanged (counters 0, 5 and 2^32 + 5 in turn).

Errors are elementwise in units of unit x 2^-24 beyond the output's slack (the half ulps of the bf16 roundings between the launch's
inputs and the output; mlp_block_ref's docstring).  "CPU": largest constant of the float32 NumPy evaluation on these inputs (bf16
outputs: of its twin without the roundings); bound = 4 x the table's entry; "MI355X": largest value seen there (the
module fixture's teardown report).

  output         CPU  bound  MI355X           output         CPU  bound  MI355X
  prod.y        0.90    4.2    0.17           bwd.y         0.79    3.6    0.02
  fwd.z         1.05    4.8    0.24           bwd.dgamma    0.26    1.2    0.11
  fwd.y         1.38    6.2    0.31           bwd.dbeta     0.31    1.4    0.08
  fwd.mean      0.88    4.0    1.39           bwd.dbias     0.45    2.0    0.45
  fwd.rstd      2.21   10.0    0.92           loss.p        1.00    4.6    0.12
  fwd.rmean     1.44    6.6    2.12           loss.grad     4.04   18.2    0.00
  fwd.rvar      1.72    7.8    1.72           loss.dbias    2.86   13.0    2.02
  st.part       1.91    8.6    1.36           loss.parts    1.32    6.0    0.55
  st.save       0.77    3.6    0.87           loss.value    1.97    9.0    0.76
  st.rmean      1.57    7.2    1.54           loss.sum      1.48    6.8    1.48
  st.rvar       0.92    4.2    0.92           wg.out        1.11    5.0    1.48
  st.bsums      0.90    4.2    0.31           wg.part       1.17    5.4    0.26
  st.dparams    0.90    4.2    0.75           wg.range      0.50    2.4    0.23

The product's a-priori ceiling (any order of the additions) is 2 (K r.u. 32) >= 64 units: every product bound above is far below it.

bf16 outputs (prod.y, fwd.z, fwd.y, bwd.y, loss.p, loss.grad) show a float32 error next to a rounding tie alone, hence their small
figures; bwd.dgamma 0.11, bwd.dbeta 0.08 and bwd.y 0.02 are those of the backward tails behind an EXACT product (small-integer
operands: no half ulp of the product in the way; bwd.dbias 0.06 there) -- behind a rounded product the three stay inside the slack.

The two paths that never ran under a comparison before, reported on their own by the teardown:
  reduction lengths of 25 and 33 steps (the second chunk reloaded, the first loaded a third time): prod.y 0.07 of a bound of 4.2, and
      every small-integer twin bit for bit, K = 769, 1025 and 1056 included;
  the generic kernel (`mlp_strip_kernel<-1, 0, 0>`: the product table, the side-job launches, the finishing launches and seven
      combinations of their own): prod.y 0.08, fwd.z 0.14, fwd.y 0.13, fwd.mean 0.79, fwd.rstd 0.92, fwd.rmean 1.16, fwd.rvar 1.42,
      st.part 1.36, st.save 0.65, st.rmean 1.54, st.rvar 0.73, st.bsums 0.29, st.dparams 0.67, bwd.dbias 0.45 -- no worse than the
      compiled forms.

Defects found with these tests: none.  No output uses more than 0.35 of its bound (fwd.mean); nothing is written outside rows 0..127 x
columns 0..(N r.u. 16) - 1, no input is changed, the call counter moves only when a launch draws.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import mlp_block_ref as R  # noqa: E402

DEV = "cuda"
WORST = {}                 # output -> largest error seen in units of unit x 2^-24
f32, f64 = np.float32, np.float64
_ids = lambda c: "-".join(map(str, c)).replace(" ", "")[:60]      # noqa: E731
GUARD, GUARD_BYTE, SENT_F64 = 256, 0xAB, -7.5


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi
    yield _cabi.load()
    for name, e in sorted(WORST.items()):
        base = name.split(" ")[0]
        print(f"\nlargest error on the GPU, {name:24s} {e:7.2f} = {e / R.bound_constant(base):5.2f} of its bound {R.bound_constant(base):.2f}", end="")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A host array on the device between two guards of 256 bytes (16-byte aligned); `get` downloads it and checks the guards."""

    def __init__(self, host):
        self.host0 = np.ascontiguousarray(host).copy()
        b = self.host0.view(np.uint8).ravel()
        self.n = b.size
        self.t = torch.full((self.n + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.t[GUARD:GUARD + self.n] = torch.from_numpy(b.copy()).to(DEV)
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def get(self):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == GUARD_BYTE).all() and (h[GUARD + self.n:] == GUARD_BYTE).all(), "a guard was written"
        return h[GUARD:GUARD + self.n].copy().view(self.host0.dtype).reshape(self.host0.shape)

    def unchanged(self):
        return np.array_equal(self.get().view(np.uint8), self.host0.view(np.uint8))


def _sent(shape, dtype):
    return np.full(shape, {np.uint16: R.SENT_BF16, f32: R.SENT_F32, f64: SENT_F64}[dtype], dtype=dtype)


class GpuImpl:
    """The launches of mlp_block_ref's protocols through the C ABI."""

    def __init__(self, lib):
        from openpystruct_amd import _cabi
        self.lib, self.cabi = lib, _cabi

    def strip_args(self, a, bufs):
        """ops_mlp_strip_args of a launch; `bufs`: name -> Buf (inputs and outputs)."""
        B, N, K, tail = a["B"], a["N"], a["K"], a["tail"]
        fwd, has_bn = tail in R.FWD_TAILS, tail in R.BN_TAILS
        s = self.cabi.MlpStripArgs()
        put = lambda name, host: bufs.setdefault(name, Buf(host)).ptr      # noqa: E731
        s.B, s.N, s.K, s.tail, s.add_mode, s.side = B, N, K, tail, a["add"], a["side"]
        s.A, s.lda = put("A", R.pack(a["A"], R.ROWS, a["lda"])), a["lda"]
        s.W, s.ldw = put("W", R.pack(a["W"], R.ru(N, 16), a["ldw"])), a["ldw"]
        s.bias = put("bias", a["bias"]) if a["bias"] is not None else None
        s.Y, s.ldy = put("Y", _sent(R.ROWS * a["ldy"], np.uint16)), a["ldy"]
        s.Yt = put("Yt", _sent(R.ru(N, 32) * R.ROWS, np.uint16))
        s.eps, s.momentum, s.slope, s.p_drop, s.seed = a["eps"], a["momentum"], a["slope"], a["p"], a["seed"]
        if has_bn:
            s.gamma, s.beta = put("gamma", a["gamma"]), put("beta", a["beta"])
            s.running_mean, s.running_var = put("rmean", a["rmean"]), put("rvar", a["rvar"])
            s.mean = put("mean", _sent(N, f32) if fwd else a["mean"])
            s.rstd = put("rstd", _sent(N, f32) if fwd else a["rstd"])
            s.Zt = put("Zt", _sent(R.ru(N, 32) * R.ROWS, np.uint16) if fwd else R.pack_t(a["Z"]))
            if not fwd:
                s.dgamma, s.dbeta = put("dgamma", _sent(N, f32)), put("dbeta", _sent(N, f32))
        s.num_batches_tracked = put("nbt", np.array([R.NBT0], dtype=np.int64))
        if tail in R.ACT_BWD:
            s.Yref_t = put("Yref_t", R.pack_t(a["Yref"]))
        if a["call"] is not None:
            s.call_counter = put("counter", np.array([a["call"], 0], dtype=np.uint64))
        s.dbias = put("dbias", _sent(N, f32))               # always offered: only the backward tails and TAIL_LOSS may write it
        if a["add"] != R.ADD_NONE or a["side"] != R.SIDE_NONE:
            No = a["No"]
            s.Ot, s.No, s.dZt = put("Ot", R.pack_t(a["O"])), No, put("dZt", R.pack_t(a["dZ"]))
            s.conv_w, s.conv_b, s.sgamma, s.sbeta = (put(k, a[k]) for k in ("cw", "cb", "sgamma", "sbeta"))
            s.seps, s.smomentum = a["seps"], a["smom"]
            s.srunning_mean, s.srunning_var = put("srm", a["srm"]), put("srv", a["srv"])
            writes_save = a["add"] == R.ADD_FWD
            s.ssave = put("ssave", _sent(2, f32) if writes_save else a["ssave"])
            nd = int(self.lib.ops_mlp_spart_doubles(No))
            assert nd == 12 * R.side_rows(No)
            sp = _sent(nd, f64)
            if a["add"] != R.ADD_NONE:
                sp[:] = np.asarray(a["spart"], dtype=f64)[:nd]
            s.spart = put("spart", sp)
            s.sdparams = put("sdparams", _sent(6, f32))
        s.snum_batches_tracked = put("snbt", np.array([R.NBT0], dtype=np.int64))
        wsn = int(self.lib.ops_mlp_loss_workspace_bytes()) // 8
        L = a if tail == R.LOSS else a["finish"]
        if L is not None:
            s.nI, s.nD, s.alpha0, s.box_weight, s.rel_penalty = L["nI"], L["nD"], L["alpha0"], L["box_w"], L["pen"]
            s.alpha = put("alpha", np.array([L["alpha"]], dtype=f32))
        if tail == R.LOSS:
            s.P, s.ldp = put("P", _sent(R.ROWS * a["ldp"], np.uint16)), a["ldp"]
            tt = _sent((N, R.ROWS), f32)                   # rows >= B are ignored: they hold the sentinel
            tt[:, :B] = a["targets"].T
            s.targets_t = put("targets_t", tt)
            s.min_constraint = put("lo", np.array([a["lo"]], dtype=f32)) if a["lo"] is not None else None
            s.max_constraint = put("hi", np.array([a["hi"]], dtype=f32)) if a["hi"] is not None else None
            s.loss_ws = put("loss_ws", _sent(wsn, f64))
        if a["finish"] is not None:
            ws = _sent(wsn, f64)
            ws[:] = np.asarray(a["loss_ws_in"], dtype=f64)[:wsn]
            s.loss_ws = put("loss_ws", ws)
            s.loss_finish_rows, s.loss_C = (L["N"] + 15) // 16, L["N"]
            s.loss, s.loss_sum = put("loss", _sent(1, f32)), put("loss_sum", np.array([a["loss_sum_in"]], dtype=f32))
        s.eval_stats = a["eval_stats"]
        return s

    def strip(self, a):
        B, N, tail = a["B"], a["N"], a["tail"]
        fwd, has_bn = tail in R.FWD_TAILS, tail in R.BN_TAILS
        bufs = {}
        s = self.strip_args(a, bufs)
        assert self.lib.ops_mlp_strip_launch(ctypes.byref(s), _stream()) == 0
        torch.cuda.synchronize()
        got = {k: b.get() for k, b in bufs.items()}
        training_bn = has_bn and fwd and not a["eval_stats"]
        written = {"Y", "Yt"} | ({"Zt"} if fwd and has_bn else set()) | ({"mean", "rstd", "rmean", "rvar", "nbt"} if training_bn else set()) | \
            ({"dgamma", "dbeta"} if has_bn and not fwd else set()) | ({"dbias"} if a["dbias"] else set()) | \
            ({"ssave", "srm", "srv", "snbt"} if a["add"] == R.ADD_FWD and not a["eval_stats"] else set()) | \
            ({"sdparams"} if a["add"] == R.ADD_BWD else set()) | ({"spart"} if a["side"] != R.SIDE_NONE else set()) | \
            ({"P", "loss_ws"} if tail == R.LOSS else set()) | ({"loss", "loss_sum"} if a["finish"] is not None else set()) | \
            ({"counter"} if tail in (R.ACT_DROP, R.BN_ACT_DROP) and a["p"] > 0 else set())
        stale = [k for k, b in bufs.items() if k not in written and not np.array_equal(got[k].view(np.uint8), b.host0.view(np.uint8))]
        assert not stale, f"buffers the launch must not write were changed: {stale}"
        raw = dict(got, intact=not stale, nbt=int(got["nbt"][0]), snbt=int(got["snbt"][0]))
        if a["side"] != R.SIDE_NONE:                      # a side job fills 2 (forward) or 12 doubles per row of partial sums, nothing else
            ns = 2 if a["side"] == R.SIDE_FWD else 12
            assert (got["spart"][ns * R.side_rows(a["No"]):] == SENT_F64).all(), "spart written past the rows of partial sums"
        if tail == R.LOSS:
            assert (got["loss_ws"][5 * ((N + 15) // 16):] == SENT_F64).all(), "loss_ws written past the strips' partial sums"
        if "counter" in got:
            assert int(got["counter"][1]) == 0, "the launch left its tally behind"
            raw["counter"] = int(got["counter"][0])
        return raw

    def wgrad(self, case, problems, ranges, norm):
        probs, B, scale, rl = case
        n = len(problems)
        wg = (self.cabi.MlpWgradProblem * n)()
        ins, outs = [], []
        for e, (N, K, extra), (At, Bt) in zip(wg, probs, problems):
            a_, b_, o_ = Buf(R.pack(At, R.ru(N, 32), R.ROWS, R.ROWS)), Buf(R.pack(Bt, R.ru(K, 32), R.ROWS, R.ROWS)), Buf(_sent((N, K + extra), f32))
            ins += [a_, b_]
            outs.append(o_)
            e.At, e.Bt, e.out, e.N, e.K, e.ldo = a_.ptr, b_.ptr, o_.ptr, N, K, K + extra
        if not norm:
            assert self.lib.ops_mlp_wgrad_group(n, wg, _stream()) == 0
            torch.cuda.synchronize()
            return dict(out=[o.get() for o in outs], intact=all(b.unchanged() for b in ins))
        rb = [Buf(r) for r in ranges]
        rp = (ctypes.c_void_p * max(1, len(rb)))(*[b.ptr for b in rb])
        rlen = (ctypes.c_int32 * max(1, len(rb)))(*[r.size for r in ranges])
        nws = int(self.lib.ops_flat_adam_workspace_bytes()) // 8
        assert nws == self.cabi.FLAT_ADAM_MAX_PARTS + 2
        ws, step, nparts = Buf(_sent(nws, f64)), Buf(np.array([R.WG_STEP0], dtype=np.int32)), ctypes.c_int32(-1)
        assert self.lib.ops_mlp_wgrad_group_norm(n, wg, len(rb), rp, rlen, scale, ws.ptr, step.ptr, R.WG_B1, R.WG_B2, ctypes.byref(nparts), _stream()) == 0
        torch.cuda.synchronize()
        w = ws.get()
        np_ = int(nparts.value)
        assert (w[np_:self.cabi.FLAT_ADAM_MAX_PARTS] == SENT_F64).all(), "the workspace was written past the partial sums"
        return dict(out=[o.get() for o in outs], intact=all(b.unchanged() for b in ins + rb), parts=w[:np_].copy(), nparts=np_, step=int(step.get()[0]),
                    corr=(float(w[self.cabi.FLAT_ADAM_MAX_PARTS]), float(w[self.cabi.FLAT_ADAM_MAX_PARTS + 1])))


def check(recs, tag=None):
    """Print every figure, then assert the records."""
    ratios, failed = R.measure(recs)
    for name, e in ratios.items():
        WORST[name] = max(WORST.get(name, 0.0), e)
        if tag:
            WORST[f"{name} {tag}"] = max(WORST.get(f"{name} {tag}", 0.0), e)
        print(f"{name}: {e:.2f} of {R.bound_constant(name):.2f}")
    assert not failed, failed
    for name, e in ratios.items():
        assert e <= R.bound_constant(name), (name, e, R.bound_constant(name))


@pytest.mark.parametrize("case", R.PRODUCT_CASES, ids=_ids)
def test_product_table_and_exact_twins(lib, case):
    """TAIL_NONE through the generic kernel at every reduction length, and the small-integer twin bit for bit."""
    steps = (case[2] + 31) // 32
    check(R.product_protocol(case, GpuImpl(lib)), "at >= 25 steps (generic kernel)" if steps >= 25 else "(generic kernel)")


@pytest.mark.parametrize("case", R.COMBO_CASES, ids=lambda c: f"{R.TAIL_NAMES[c[0]]}-add{c[1]}-eval{c[2]}-{'x'.join(map(str, R.SHAPES[c[3]]))}")
def test_every_combination_at_every_shape(lib, case):
    generic = case[:3] in R.GENERIC_ONLY
    check(R.PROTOCOLS["combo"][0](case, GpuImpl(lib)), "(generic kernel)" if generic else None)


@pytest.mark.parametrize("case", R.EXACT_BWD_CASES, ids=lambda c: f"{R.TAIL_NAMES[c[0]]}-{'x'.join(map(str, R.SHAPES[c[1]]))}")
def test_backward_tails_behind_an_exact_product(lib, case):
    """Small-integer operands: the product and its bf16 rounding are exact, so dgamma, dbeta, dbias and the gradient through the
    normalisation are held at float32 level (no half ulp of the product in the way)."""
    check(R.PROTOCOLS["bwdx"][0](case, GpuImpl(lib)), "behind an exact product")


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=lambda c: f"{R.TAIL_NAMES[c[0]]}-No{c[2]}-B{c[3]}")
def test_block_and_side_jobs_at_the_stencil_edges(lib, case):
    check(R.PROTOCOLS["block"][0](case, GpuImpl(lib)))


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=_ids)
def test_loss_tail_and_finishing_launch(lib, case):
    check(R.PROTOCOLS["loss"][0](case, GpuImpl(lib)))


@pytest.mark.parametrize("case", R.TIE_CASES, ids=_ids)
def test_dropout_keeps_the_planted_tie(lib, case):
    check(R.PROTOCOLS["tie"][0](case, GpuImpl(lib)))


@pytest.mark.parametrize("norm", (False, True), ids=("plain", "norm"))
@pytest.mark.parametrize("case", R.WG_CASES, ids=lambda c: f"{len(c[0])}prob-B{c[1]}")
def test_weight_gradients(lib, case, norm):
    check(R.wgrad_protocol(case, GpuImpl(lib), norm))


def test_evaluation_slots_equal_single_launches(lib):
    """Three slots of B = 5 holding 11 rows in one launch (grid.y) against three single launches on the same arenas, bit for bit; the
    slots' outputs are also the reference's (the single launches are held to it through the protocol)."""
    impl = GpuImpl(lib)
    B, N, K, total = 5, 17, 33, 11
    singles = [R.launch(min(B, total - B * s), N, K, R.ACT_DROP, ev=1, slope=0.01, key=600 + s) for s in range(3)]
    for a in singles[1:]:
        a["W"], a["bias"] = singles[0]["W"], singles[0]["bias"]
    want = []
    for a in singles:
        raw = impl.strip(a)
        r, _ = R.strip_records(a, raw)
        check(r)
        want.append((raw["Y"], raw["Yt"]))
    # one arena per slot: A | Y | Yt, the same layout in each
    a0 = singles[0]
    nA, nY, nYt = R.ROWS * a0["lda"], R.ROWS * a0["ldy"], R.ru(N, 32) * R.ROWS
    stride = 2 * (nA + nY + nYt)
    assert stride % 16 == 0
    arena = np.concatenate([np.concatenate([R.pack(a["A"], R.ROWS, a["lda"]).ravel(), np.full(nY + nYt, R.SENT_BF16, dtype=np.uint16)]) for a in singles])
    ab, bufs = Buf(arena), {}
    s = impl.strip_args(a0, bufs)
    s.B, s.A, s.Y, s.Yt = B, ab.ptr, ab.ptr + 2 * nA, ab.ptr + 2 * (nA + nY)
    s.n_slots, s.slot_total_rows, s.slot_stride = 3, total, stride
    assert lib.ops_mlp_strip_launch(ctypes.byref(s), _stream()) == 0
    torch.cuda.synchronize()
    out = ab.get().reshape(3, -1)
    for k, (y, yt) in enumerate(want):
        assert np.array_equal(out[k, :nA], R.pack(singles[k]["A"], R.ROWS, a0["lda"]).ravel()), "a slot's input was written"
        assert np.array_equal(out[k, nA:nA + nY], y) and np.array_equal(out[k, nA + nY:], yt), f"slot {k} differs from its single launch"
