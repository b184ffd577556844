"""The row-staged beam kernels take their leading arguments one by one (preloaded into SGPRs at wave launch) and the rest in a
trailing struct (csrc/beam_io.hpp, RowsHead / RowsTail).  The arithmetic is untouched (tests/test_gpu_beam_rows_bits.py); what can
break is an argument landing in the wrong slot.  Every check here is bit for bit against another call on the same data:

  strides   5 x 37 (odd rows, fixed rotation, a tail wave of one beam): I rows Ne + 3 apart and Fy rows Ne + 5 apart, poison between
            the rows, against the dense call and against beam_solve_kernel<16, 7>
  bridge    9 x 100: the forces-only entry (v, theta NULL), cached and streaming stores, against V and M of the full call
  epoch     the fused sizing epoch with its float32 inertias 8 bytes off a 16-byte boundary, against the aligned call
  bad input a row stride of 2^31 is refused before anything is launched
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import beam_rows_bits as rb  # noqa: E402

STREAM_OUT = 0x100                 # OPS_AMD_TILING_STREAM_OUT
POISON = 1.0e300                   # between the rows of a strided array: finite, so that it shows as a wrong number and not as a NaN row
OUTS = ("v", "theta", "V", "M", "status")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    import openpystruct_amd as oa
    from openpystruct_amd import _cabi
    return oa, _cabi, _cabi.load(), rb.inputs()


def _dev(z, dt):
    return torch.as_tensor(np.ascontiguousarray(z), dtype=dt).to("cuda")


def _strided(rows, stride):
    """[B, n] -> a [B, stride] device buffer with the rows in front and POISON behind them."""
    B, n = rows.shape
    buf = np.full((B, stride), POISON)
    buf[:, :n] = rows
    return _dev(buf, torch.float64)


def _solve(lib, case, tiling, I_stride=None, Fy_stride=None, forces_only=False):
    """One raw C-ABI call; every output as raw bits (v / theta of a forces-only call: the NaN they were filled with)."""
    B, Ne = case["I"].shape
    N = Ne + 1
    I_stride, Fy_stride = I_stride or Ne, Fy_stride or N
    x, E, wy = (_dev(case[k], torch.float64) for k in ("x", "E", "wy"))
    fix = _dev(case["fix"], torch.uint8)
    I, Fy = _strided(case["I"], I_stride), _strided(case["Fy"], Fy_stride)
    out = {k: torch.full((B, n), float("nan"), dtype=torch.float64, device="cuda") for k, n in (("v", N), ("theta", N), ("V", Ne), ("M", Ne))}
    out["status"] = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    head = (B, Ne, x.data_ptr(), 0, E.data_ptr(), 0, I.data_ptr(), I_stride, fix.data_ptr(), 0, Fy.data_ptr(), Fy_stride, wy.data_ptr(), 0)
    if forces_only:
        rc = lib.ops_beam_solve_forces_f64(*head, out["V"].data_ptr(), out["M"].data_ptr(), out["status"].data_ptr(), None, tiling, stream)
    else:
        rc = lib.ops_beam_solve_batched_f64(*head, *(out[k].data_ptr() for k in OUTS), tiling, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    if forces_only:
        assert torch.isnan(out["v"]).all() and torch.isnan(out["theta"]).all()      # nobody wrote where nothing was passed
    return {k: rb.bits(out[k].cpu().numpy()) for k in OUTS}


def _same(got, want, keys, what):
    for k in keys:
        diff = got[k] != want[k]
        assert not diff.any(), (what, k, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.fixture(scope="module")
def case_b_dense(env):
    oa, _, lib, cases = env
    assert oa.kernel_name(5, 37, 16 | rb.ROWS) == "beam_rows_kernel<16, 7, 3, false>"
    got = _solve(lib, cases["b"], 16 | rb.ROWS)
    assert not got["status"].any() and not np.isnan(got["v"].view(np.float64)).any()
    return got


def test_strided_rows_and_tail_wave(env, case_b_dense):
    _, _, lib, cases = env
    Ne = cases["b"]["I"].shape[1]
    got = _solve(lib, cases["b"], 16 | rb.ROWS, I_stride=Ne + 3, Fy_stride=Ne + 5)
    _same(got, case_b_dense, OUTS, "strided against dense")


def test_rows_kernel_against_beam_solve_kernel(env, case_b_dense):
    """The two 16 x 7 kernels run the same statements (profiles/beam_rows_trim_notes.md): a stride, a pointer or a count in the wrong
    slot of the row kernel cannot hide behind the dense call making the same mistake."""
    oa, _, lib, cases = env
    assert oa.kernel_name(5, 37, 16).startswith("beam_solve_kernel<16, 7")
    _same(_solve(lib, cases["b"], 16), case_b_dense, OUTS, "tiling 16 against 16 | ROWS")


@pytest.mark.parametrize("stream_out", [0, STREAM_OUT], ids=["cached", "stream_out"])
def test_forces_only_bridge(env, stream_out):
    oa, _, lib, cases = env
    assert oa.kernel_name(9, 100, 16 | rb.ROWS) == "beam_rows_kernel<16, 7, 3, false>"
    full = _solve(lib, cases["a"], 16 | rb.ROWS | stream_out)
    assert not full["status"].any()
    _same(_solve(lib, cases["a"], 16 | rb.ROWS | stream_out, forces_only=True), full, ("V", "M", "status"), "forces only against the full call")


def _epoch(lib, a, shift):
    """rb._epoch with the float32 inertias `shift` floats into their allocation."""
    from openpystruct_amd import sizing
    hp = sizing.SizingConfig().c_params()
    tab = np.zeros((hp.max_epochs, 2), dtype=np.float32)
    lib.ops_sizing_schedule_f32(ctypes.byref(hp), tab.ctypes.data)
    pre = rb.epoch_state(a)
    B, Ne = a["I"].shape
    s = {k: _dev(z, None) for k, z in pre.items()}
    room = torch.full((B * Ne + 4,), 7.0, dtype=torch.float32, device="cuda")
    s["I"] = room[shift:shift + B * Ne].view(B, Ne)
    s["I"].copy_(_dev(pre["I"], None))
    assert s["I"].data_ptr() % 16 == (4 * shift) % 16 and s["I"].data_ptr() % 8 == 0
    dx, dE, dFy, dwy = (_dev(a[k], torch.float64) for k in ("x", "E", "Fy", "wy"))
    dfix, sched = _dev(a["fix"], torch.uint8), _dev(tab, None)
    rc = lib.ops_beam_sizing_epoch_f32(
        B, Ne, dx.data_ptr(), 0, dE.data_ptr(), 0, dfix.data_ptr(), 0, dFy.data_ptr(), Ne + 1, dwy.data_ptr(), 0,
        *(s[k].data_ptr() for k in rb.EPOCH_STATE[:-1]), ctypes.byref(hp), sched.data_ptr(), s["status"].data_ptr(), 0,
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (room[:shift] == 7.0).all() and (room[shift + B * Ne:] == 7.0).all()
    return {k: rb.bits(z) for k, z in pre.items()}, {k: rb.bits(s[k].cpu().numpy()) for k in rb.EPOCH_STATE}


def test_sizing_epoch_inertias_off_16_bytes(env):
    _, _, lib, cases = env
    pre, aligned = _epoch(lib, cases["a"], 0)
    _, shifted = _epoch(lib, cases["a"], 2)
    for k in rb.EPOCH_STATE:
        assert np.array_equal(shifted[k], aligned[k]), ("beam_rows_sizing_kernel<16, 7, 3>", k)
    assert (aligned["status"].view(np.int32)[np.arange(9) != 5] == 0).all()
    assert not np.array_equal(aligned["I"], pre["I"])          # the epoch did step the live cases
    for k in rb.EPOCH_STATE[:-1]:          # case 5 had finished (active == 0): nothing of it moves
        assert np.array_equal(shifted[k][5], pre[k][5]), k


@pytest.mark.parametrize("which", ["I", "Fy"])
def test_row_stride_of_2_to_31_is_refused(env, which):
    """The row kernels take the strides as 32-bit values: the host refuses what does not fit, and launches nothing."""
    _, cabi, lib, cases = env
    case = cases["b"]
    B, Ne = 2, case["I"].shape[1]
    N = Ne + 1
    x, E, wy, I, Fy = (_dev(z, torch.float64) for z in (case["x"], case["E"], case["wy"], case["I"][:B], case["Fy"][:B]))
    fix = _dev(case["fix"], torch.uint8)
    outs = [torch.full((B, n), -3.0, dtype=torch.float64, device="cuda") for n in (N, N, Ne, Ne)]
    status = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    I_stride, Fy_stride = (1 << 31, N) if which == "I" else (Ne, 1 << 31)
    for tiling in (0, 16 | rb.ROWS, 16):
        rc = lib.ops_beam_solve_batched_f64(B, Ne, x.data_ptr(), 0, E.data_ptr(), 0, I.data_ptr(), I_stride, fix.data_ptr(), 0, Fy.data_ptr(), Fy_stride,
                                            wy.data_ptr(), 0, *(o.data_ptr() for o in outs), status.data_ptr(), tiling,
                                            torch.cuda.current_stream().cuda_stream)
        assert rc == cabi.ERR_INVALID_ARG, (tiling, rc)
    torch.cuda.synchronize()
    assert all(bool((o == -3.0).all()) for o in outs) and bool((status == -77).all())
