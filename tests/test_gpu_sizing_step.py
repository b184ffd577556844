"""One optimiser epoch of the sizing loop, kernel by kernel, against the float64 reference of the same epoch
(oracle/sizing_oracle.py: sizing_step_reference -- SingleCore.py:195-219 and torch's Adam in numpy float64):
ops_beam_sizing_step_f32, ops_beam_sizing_step_vm32_f32 and every kernel behind ops_beam_sizing_epoch_f32, called through
the C ABI from arbitrary optimiser states, with waves that mix improving, waiting, stopping and finished cases.

Errors are elementwise, over the magnitude float32 round-off scales with (sizing_step_errors), in eps32 = 2^-23:

                                                      exp_avg   exp_avg_sq   I      loss
  float32 arithmetic alone, CPU (stand-alone inputs)     3.3       6.9        2.2    1.9
  ... fed with forces moved by one float32 ulp           4.5       9.2        2.4    2.8     (the fused batches)
  ... with 1 - beta formed in float32                    5.3     112.7       47.9    1.9     <- the defect this file found
  bound, stand-alone kernels                            16        16         16     16
  bound, fused epoch = 4 x 9.11                         36.5      36.5       36.5   36.5
  largest on the MI355X: not measured yet

The CPU rows are measured (and the bounds re-derived) by tests/test_sizing_step_reference.py on the inputs used here.  The
stand-alone bound leaves room for the wave-order sum; the fused one is four times what a float32 neighbour of every force
costs, since the kernel's own float64 solve may round a force to the float32 next to the reference's.  Both bounds sit far
below the 112 eps32 by which exp_avg_sq was off while the kernels formed 1.0f - (float)beta2: with that constant back, the
exp_avg_sq check fails on all three entry points.

Kernels reached (tiling, Ne, B): sizing_step_cases.FUSED_TABLE; rows that are not dense: test_fused_epoch_unaligned_rows.
"""
import ctypes
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import sizing_oracle as so  # noqa: E402
from tests import sizing_step_cases as sc  # noqa: E402

SENT_F32, SENT_F64, SENT_I32 = np.float32(-12345.678), np.float64(-98765.4321), np.int32(-77)
SHIFTS = range(5)          # every case of a batch takes every kind of sc.KINDS and every t once
HPS = {"beam": sc.beam_hp, "frame": sc.frame_hp}
DEV = "cuda"
WORST = {}                 # kernel -> largest errors seen, printed when the module is done


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi
    yield _cabi.load()
    for kernel, errs in sorted(WORST.items()):
        print(f"\nlargest error on the GPU, {kernel}: " + "  ".join(f"{k} {e:.2f}" for k, e in errs.items()), end="")


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(np.broadcast_to(np.asarray(b, dtype=a.dtype), a.shape)))


class State:
    """The device arrays of one batch: optimiser state in / out and every output buffer, pre-filled with a sentinel."""

    def __init__(self, I, m, v, st, offset_I=False):
        B, Ne = I.shape
        f32 = dict(dtype=torch.float32, device=DEV)
        buf = torch.empty(B * Ne + 2, **f32)             # the allocation is aligned to far more than 16 bytes
        self.I = buf[1:1 + B * Ne] if offset_I else buf[:B * Ne]
        self.I.copy_(_dev(I).reshape(-1))
        assert self.I.data_ptr() % 8 == (4 if offset_I else 0)
        self.exp_avg, self.exp_avg_sq = _dev(m), _dev(v)
        self.best_loss, self.patience_cnt = _dev(st.best), _dev(st.cnt)
        self.epochs_run, self.active = _dev(st.t), _dev(st.active)
        self.last_loss = torch.full((B,), float(SENT_F32), **f32)
        self.I64 = torch.full((B, Ne), float(SENT_F64), dtype=torch.float64, device=DEV)
        self.I_last = torch.full((B, Ne), float(SENT_F32), **f32)
        self.V32, self.M32 = torch.full((B, Ne), float(SENT_F32), **f32), torch.full((B, Ne), float(SENT_F32), **f32)
        self.status = torch.full((B,), int(SENT_I32), dtype=torch.int32, device=DEV)
        self.shape = (B, Ne)

    NAMES = ("I", "exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss", "I64", "I_last",
             "V32", "M32", "status")

    def snapshot(self):
        torch.cuda.synchronize()
        out = {k: getattr(self, k).cpu().numpy().copy() for k in self.NAMES}
        out["I"] = out["I"].reshape(self.shape)
        return out

    def ptrs(self, *names):
        return [getattr(self, k).data_ptr() for k in names]


def _rows(ref, mask):
    return {k: a[mask] for k, a in ref.items()}


def check_epoch(kernel, pre, post, st, ref, hp, bound, wrote=(), skip=None):
    """`post` is `pre` after one epoch of the batch whose cases are in the states `st`; `ref` the float64 reference of it.
    `wrote`: the optional outputs this entry point has (I64, I_last, V32, M32, status); `skip`: cases left out of everything."""
    B = st.kind.shape[0]
    skip = np.zeros(B, dtype=bool) if skip is None else skip
    idle, act = (st.active == 0) & ~skip, (st.active == 1) & ~skip
    stop, cont = act & ref["stop"], act & ~ref["stop"]
    # (e) and everything the entry point has no business with: bitwise untouched.  (The fused solve reports `status` per wave:
    # an idle case that shares a wave with a live one gets its 0 again.)
    for k in State.NAMES:
        if k == "status" and "status" in wrote:
            assert np.isin(post[k][idle], (0, SENT_I32)).all(), (kernel, k)
        elif k in ("I64", "I_last", "V32", "M32", "status") and k not in wrote:
            assert _same_bits(post[k], pre[k]), (kernel, k)
        else:
            assert _same_bits(post[k][idle], pre[k][idle]), (kernel, k, "an inactive case was touched")
    if not act.any():
        return
    # the numbers
    errs = so.sizing_step_errors(_rows(ref, act), pre["I"][act], pre["exp_avg"][act], pre["exp_avg_sq"][act], post["I"][act],
                                 post["exp_avg"][act], post["exp_avg_sq"][act], post["last_loss"][act], hp)
    print(kernel, pre["I"].shape, " ".join(f"{k} {e:.2f}" for k, e in errs.items()))
    w = WORST.setdefault(kernel, dict.fromkeys(errs, 0.0))
    w.update({k: max(w[k], e) for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= bound, (kernel, k, e, bound)
    clamped = act[:, None] & (ref["I_free"] < 0.5 * hp.clamp_min)         # far below the clamp: exactly float32(clamp_min)
    assert _same_bits(post["I"][clamped], np.float32(hp.clamp_min)), kernel
    # the early-stop bookkeeping, exactly
    improved = act & (ref["cnt"] == 0)
    assert _same_bits(post["best_loss"][improved], post["last_loss"][improved]), kernel
    assert _same_bits(post["best_loss"][act & ~improved], pre["best_loss"][act & ~improved]), kernel
    assert np.array_equal(post["patience_cnt"][act], ref["cnt"][act]), kernel
    assert np.array_equal(post["epochs_run"][act], st.t[act] + 1), kernel
    assert np.array_equal(post["active"][act] != 0, ~ref["stop"][act]), (kernel, st.kind, post["active"])
    if "I64" in wrote:       # refreshed for a case that goes on, frozen for one that stops in this call
        assert _same_bits(post["I64"][cont], post["I"][cont].astype(np.float64)), kernel
        assert _same_bits(post["I64"][stop], SENT_F64), kernel
    if "I_last" in wrote:    # written once, when the case stops: the inertias this last solve ran on
        assert _same_bits(post["I_last"][stop], pre["I"][stop]), kernel
        assert _same_bits(post["I_last"][cont], SENT_F32), kernel
    if "status" in wrote:
        assert (post["status"][act] == 0).all(), kernel


def check_second_call(kernel, post, post2, st, ref, skip=None):
    """The same call once more: a case that stopped (or never ran) is bitwise unchanged -- I64 not refreshed, I_last not
    rewritten -- and a case that went on ran one more epoch."""
    skip = np.zeros(st.kind.shape[0], dtype=bool) if skip is None else skip
    cont = (st.active == 1) & ~ref["stop"] & ~skip
    for k in State.NAMES:
        if k != "status":
            assert _same_bits(post2[k][~cont & ~skip], post[k][~cont & ~skip]), (kernel, k, "a finished case was touched")
    assert np.array_equal(post2["epochs_run"][cont], st.t[cont] + 2), kernel
    still = cont & (post2["active"] != 0)
    if (post["I64"] != SENT_F64).any():
        assert _same_bits(post2["I64"][still], post2["I"][still].astype(np.float64)), kernel
        assert _same_bits(post2["I64"][cont & ~still], post["I"][cont & ~still].astype(np.float64)), kernel


def _schedule(lib, hp):
    tab = np.zeros((hp.max_epochs, 2), dtype=np.float32)
    lib.ops_sizing_schedule_f32(ctypes.byref(hp), tab.ctypes.data)
    return tab


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# the stand-alone step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp_name", list(HPS))
def test_schedule_table(lib, hp_name):
    """Every row of the host table against lr gamma^t / (1 - beta1^(t+1)) and sqrt(1 - beta2^(t+1)) in float64: 2 ulp, one
    rounding each for lr_t, bc1 and their quotient."""
    hp = HPS[hp_name]()
    tab = _schedule(lib, hp).astype(np.float64)
    want = np.stack(so._schedule_f64(np.arange(hp.max_epochs), hp), axis=1)
    assert (np.abs(tab - want) <= 2 * np.spacing(want.astype(np.float32)).astype(np.float64)).all()


STEP_SHAPES = [(1, 1), (5, 63), (4, 64), (13, 65), (3, 129), (5, 511), (2, 512)]


def _run_step(lib, entry, V, M, I, m, v, st, hp, *, vm32=True, schedule=None):
    s = State(I, m, v, st)
    B, Ne = I.shape
    if entry == "ops_beam_sizing_step_f32":
        dV, dM = _dev(V), _dev(M)
        call = lambda: lib.ops_beam_sizing_step_f32(   # noqa: E731
            B, Ne, *s.ptrs("I", "I64"), dV.data_ptr(), dM.data_ptr(),
            *s.ptrs("exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss"),
            *(s.ptrs("V32", "M32") if vm32 else (None, None)), ctypes.byref(hp), _stream())
    else:
        dV, dM = _dev(V.astype(np.float32)), _dev(M.astype(np.float32))
        sched = None if schedule is None else _dev(schedule)
        call = lambda: lib.ops_beam_sizing_step_vm32_f32(   # noqa: E731
            B, Ne, *s.ptrs("I", "I64"), dV.data_ptr(), dM.data_ptr(),
            *s.ptrs("exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss"),
            ctypes.byref(hp), None if sched is None else sched.data_ptr(), _stream())
    pre = s.snapshot()
    assert call() == 0
    post = s.snapshot()
    assert call() == 0
    return pre, post, s.snapshot()


@pytest.mark.parametrize("hp_name", list(HPS))
@pytest.mark.parametrize("B,Ne", STEP_SHAPES)
def test_step_f32(lib, B, Ne, hp_name):
    """ops_beam_sizing_step_f32 (float64 forces in, rounded by the kernel) with the V32 / M32 records and without them."""
    hp = HPS[hp_name]()
    entry = "ops_beam_sizing_step_f32"
    for shift in SHIFTS:
        rng = np.random.default_rng([B, Ne, shift])
        I, m, v = sc.optimiser_state(rng, B, Ne)
        V, M = sc.random_forces(rng, B, Ne)
        st, ref = sc.reference_epoch(I, m, v, V, M, hp, shift, group=4)
        pre, post, post2 = _run_step(lib, entry, V, M, I, m, v, st, hp)
        check_epoch(entry, pre, post, st, ref, hp, sc.STEP_BOUND, wrote=("I64", "V32", "M32"))
        check_second_call(entry, post, post2, st, ref)
        act = st.active == 1
        assert _same_bits(post["V32"][act], V.astype(np.float32)[act]) and _same_bits(post["M32"][act], M.astype(np.float32)[act])
        # the clamp elements (no forces, a step of ~0.1 down from 5e-3) do clamp unless the schedule has decayed the step away
        c = sc.clamp_columns(Ne)
        big_step = act & ((st.t <= 17) | (hp.gamma == 1.0))
        assert _same_bits(post["I"][big_step][:, c], np.float32(hp.clamp_min))
        # V32 == M32 == NULL: the same state, bit for bit
        pre_n, post_n, post2_n = _run_step(lib, entry, V, M, I, m, v, st, hp, vm32=False)
        check_epoch(entry, pre_n, post_n, st, ref, hp, sc.STEP_BOUND, wrote=("I64",))
        for k in State.NAMES:
            if k not in ("V32", "M32"):
                assert _same_bits(post_n[k], post[k]) and _same_bits(post2_n[k], post2[k]), k


@pytest.mark.parametrize("hp_name", list(HPS))
@pytest.mark.parametrize("B,Ne", STEP_SHAPES)
def test_step_vm32(lib, B, Ne, hp_name):
    """ops_beam_sizing_step_vm32_f32 (float32 forces in) with the host's schedule table and with schedule = NULL (pow in the
    kernel): both within the bound of the reference, and of each other."""
    hp = HPS[hp_name]()
    entry = "ops_beam_sizing_step_vm32_f32"
    table = _schedule(lib, hp)
    for shift in SHIFTS:
        rng = np.random.default_rng([B, Ne, shift])
        I, m, v = sc.optimiser_state(rng, B, Ne)
        V, M = sc.random_forces(rng, B, Ne)
        st, ref = sc.reference_epoch(I, m, v, V, M, hp, shift, group=4)
        runs = {}
        for name, schedule in (("table", table), ("pow", None)):
            pre, post, post2 = runs[name] = _run_step(lib, entry, V, M, I, m, v, st, hp, schedule=schedule)
            check_epoch(entry, pre, post, st, ref, hp, sc.STEP_BOUND, wrote=("I64",))
            check_second_call(entry, post, post2, st, ref)
        act = st.active == 1
        if act.any():
            a, b = runs["table"][1], runs["pow"][1]
            other = dict(_rows(ref, act), I=b["I"][act].astype(np.float64), exp_avg=b["exp_avg"][act].astype(np.float64),
                         exp_avg_sq=b["exp_avg_sq"][act].astype(np.float64), loss=b["last_loss"][act].astype(np.float64))
            apart = so.sizing_step_errors(other, pre["I"][act], pre["exp_avg"][act], pre["exp_avg_sq"][act], a["I"][act],
                                          a["exp_avg"][act], a["exp_avg_sq"][act], a["last_loss"][act], hp)
            assert max(apart.values()) <= sc.STEP_BOUND, apart
            for k in ("patience_cnt", "epochs_run", "active"):
                assert np.array_equal(a[k], b[k])


# ---------------------------------------------------------------------------------------------------------------------
# the fused epoch
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_name(tiling, per_case, P, M):
    rows = tiling == 0 and not per_case and P == 16
    return f"beam_rows_sizing_kernel<{P}, {M}>" if rows else f"beam_sizing_epoch_kernel<{P}, {M}, shared={not per_case}>"


def _run_epoch(lib, c, st, hp, tiling, *, per_case, offset_I=False, fy_pad=0, fix=None, calls=2):
    """ops_beam_sizing_epoch_f32 on the beams and optimiser state of `c` (sizing_step_cases.fused_case)."""
    B, Ne = c.I.shape
    N = Ne + 1
    s = State(c.I, c.m, c.v, st, offset_I=offset_I)
    Fy = np.full((B, N + fy_pad), np.nan)
    Fy[:, :N] = c.Fy
    fix = c.fix if fix is None else fix
    dx, dE, dfix, dFy, dwy = _dev(c.x), _dev(c.E), _dev(fix, torch.uint8), _dev(Fy), _dev(c.wy)
    sched = _dev(_schedule(lib, hp))
    call = lambda: lib.ops_beam_sizing_epoch_f32(   # noqa: E731
        B, Ne, dx.data_ptr(), N if per_case else 0, dE.data_ptr(), Ne if per_case else 0, dfix.data_ptr(), N if fix.ndim == 2 else 0,
        dFy.data_ptr(), N + fy_pad, dwy.data_ptr(), Ne if per_case else 0,
        *s.ptrs("I", "I_last", "exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss"),
        ctypes.byref(hp), sched.data_ptr(), s.status.data_ptr(), tiling, _stream())
    snaps = [s.snapshot()]
    for _ in range(calls):
        assert call() == 0
        snaps.append(s.snapshot())
    return snaps


@pytest.mark.parametrize("row", range(len(sc.FUSED_TABLE)), ids=lambda r: "tiling{}-{}-P{}xM{}".format(
    sc.FUSED_TABLE[r][0], "percase" if sc.FUSED_TABLE[r][1] else "shared", *sc.FUSED_TABLE[r][2:4]))
def test_fused_epoch(lib, row):
    """ops_beam_sizing_epoch_f32, one row of sizing_step_cases.FUSED_TABLE: the forces of the float64 dense solve on the widened
    float32 inertias, then the reference epoch.  Odd and even Ne, full, ragged and all-inactive waves, mixed states in a wave."""
    tiling, per_case, P, M, shapes = sc.FUSED_TABLE[row]
    hp = sc.beam_hp()
    kernel = _kernel_name(tiling, per_case, P, M)
    for Ne, B in shapes:
        c = sc.fused_case(Ne, B, per_case)
        for shift in SHIFTS:
            st, ref = sc.reference_epoch(c.I, c.m, c.v, c.V, c.M, hp, shift, group=64 // P)
            pre, post, post2 = _run_epoch(lib, c, st, hp, tiling, per_case=per_case)
            check_epoch(kernel, pre, post, st, ref, hp, sc.FUSED_BOUND, wrote=("I_last", "status"))
            check_second_call(kernel, post, post2, st, ref)


UNALIGNED = [(0, False, 16, 7, 99, 9), (0, False, 16, 7, 100, 5), (16, False, 16, 7, 99, 9), (16, True, 16, 7, 100, 9),
             (8, False, 8, 13, 103, 17), (8, True, 8, 13, 102, 8), (32, False, 32, 4, 127, 5), (32, True, 32, 4, 126, 2),
             (64, False, 64, 2, 127, 2), (64, True, 64, 2, 112, 2), (64, False, 64, 4, 128, 2)]


@pytest.mark.parametrize("how", ["I_4_bytes_past_8", "Fy_stride_N_plus_3"])
@pytest.mark.parametrize("tiling,per_case,P,M,Ne,B", UNALIGNED)
def test_fused_epoch_unaligned_rows(lib, tiling, per_case, P, M, Ne, B, how):
    """Legal by the host checks, not dense: float32 inertias that start 4 bytes past an 8-byte boundary, load rows with a
    stride of N + 3.  beam_solve.hip's kernels take their row-by-row variant, beam_fat.hip's read unaligned pairs."""
    hp = sc.beam_hp()
    c = sc.fused_case(Ne, B, per_case)
    kernel = _kernel_name(tiling, per_case, P, M) + " unaligned"
    for shift in (0, 3):
        st, ref = sc.reference_epoch(c.I, c.m, c.v, c.V, c.M, hp, shift, group=64 // P)
        pre, post, post2 = _run_epoch(lib, c, st, hp, tiling, per_case=per_case, offset_I=how.startswith("I"),
                                      fy_pad=0 if how.startswith("I") else 3)
        check_epoch(kernel, pre, post, st, ref, hp, sc.FUSED_BOUND, wrote=("I_last", "status"))
        check_second_call(kernel, post, post2, st, ref)


@pytest.mark.parametrize("tiling,P,M,Ne,B", [(0, 16, 7, 99, 9), (8, 8, 13, 103, 17), (32, 32, 4, 127, 5)])
def test_fused_epoch_beside_an_unsupported_beam(lib, tiling, P, M, Ne, B):
    """Per-case supports, one case with none at all: its status is non-zero, and every other case of its wavefront (and batch)
    still meets the bound."""
    hp = sc.beam_hp()
    c = sc.fused_case(Ne, B, False)
    wave = np.arange(B) // (64 // P)
    for shift in SHIFTS:                    # the first batch in which some wave holds two live cases: one of them loses its supports
        st, ref = sc.reference_epoch(c.I, c.m, c.v, c.V, c.M, hp, shift, group=64 // P)
        bad = next((b for b in range(B) if st.active[b] and (st.active[wave == wave[b]] == 1).sum() > 1), None)
        if bad is not None:
            break
    fix = np.tile(c.fix, (B, 1))
    fix[bad] = 0
    skip = np.arange(B) == bad
    pre, post = _run_epoch(lib, c, st, hp, tiling, per_case=False, fix=fix, calls=1)
    assert post["status"][bad] not in (0, SENT_I32)
    check_epoch(_kernel_name(tiling or 16, False, P, M) + " beside a failed solve", pre, post, st, ref, hp,
                sc.FUSED_BOUND, wrote=("I_last", "status"), skip=skip)


def test_fused_epoch_refusals(lib):
    """No launch: the row-staged 16-lane kernel with per-case geometry, the row-staged 8-lane kernel (never a fused epoch),
    more than 128 elements."""
    from openpystruct_amd import _cabi
    hp = sc.beam_hp()

    def rc(Ne, B, per_case, tiling):
        rng = np.random.default_rng(Ne)
        x, fix, E, wy, Fy = sc.beams(rng, B, Ne, per_case)
        I, m, v = sc.optimiser_state(rng, B, Ne)
        z = np.zeros(B)
        c = types.SimpleNamespace(x=x, fix=fix, E=E, wy=wy, Fy=Fy, I=I, m=m, v=v)
        st = sc.case_states(z + 1.0, hp, 0, 4)
        s = State(I, m, v, st)
        N = Ne + 1
        dx, dE, dfix, dFy, dwy = _dev(c.x), _dev(c.E), _dev(fix, torch.uint8), _dev(Fy), _dev(c.wy)
        pre = s.snapshot()
        code = lib.ops_beam_sizing_epoch_f32(
            B, Ne, dx.data_ptr(), N if per_case else 0, dE.data_ptr(), Ne if per_case else 0, dfix.data_ptr(), N if per_case else 0,
            dFy.data_ptr(), N, dwy.data_ptr(), Ne if per_case else 0,
            *s.ptrs("I", "I_last", "exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss"),
            ctypes.byref(hp), None, s.status.data_ptr(), tiling, _stream())
        post = s.snapshot()
        assert all(_same_bits(post[k], pre[k]) for k in State.NAMES)
        return code

    assert rc(40, 5, True, 16 | sc.TILING_ROWS) == _cabi.ERR_UNSUPPORTED
    assert rc(40, 5, False, 8 | sc.TILING_ROWS) == _cabi.ERR_UNSUPPORTED
    for tiling in (0, 64, 16 | sc.TILING_ROWS):
        assert rc(129, 2, False, tiling) == _cabi.ERR_UNSUPPORTED
