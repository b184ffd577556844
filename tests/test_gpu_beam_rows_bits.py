"""The row-staged beam kernels against the bits recorded before their instruction stream was trimmed
(tests/golden/beam_rows_parent_bits.npz, cases in tests/beam_rows_bits.py): what was removed multiplied by exactly 1, added
exactly 0 or subtracted 0 * y for finite y, so no beam whose status is 0 may move by a bit -- in beam_rows_kernel<16, 7, 3, false>
(plain, with a fixed rotation, beside a failed beam), in the kernels that share its headers (beam_solve_kernel<16, 7>,
beam_rows_kernel<8, 13, 2, false>) and in the fused sizing epoch, whose optimiser state is compared before and after."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import beam_rows_bits as rb  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def runs():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    spec = importlib.util.spec_from_file_location("make_beam_rows_parent_bits", os.path.join(GOLDEN, "make_beam_rows_parent_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return rb.run_all(), gen.unpack(np.load(gen.PATH))


@pytest.mark.parametrize("case", ["a", "b", "d16", "d8r"])
def test_solve_bits(runs, case):
    got, want = runs
    assert not got[case]["status"].any()
    for k in ("status", "v", "theta", "V", "M"):
        diff = got[case][k] != want[case][k]
        assert not diff.any(), (rb.KERNELS[case], k, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def test_failed_beam_and_its_wave(runs):
    """Case c: the beam with a node that has no stiffness reports status 1 and NaN rows; the three beams in its wave are bit-equal."""
    got, want = runs
    ok = np.arange(4) != rb.FAILED_BEAM
    assert got["c"]["status"].tolist() == [0, 0, 1, 0] == want["c"]["status"].tolist()
    for k in ("v", "theta", "V", "M"):
        assert np.isnan(got["c"][k][rb.FAILED_BEAM].view(np.float64)).all(), k
        diff = got["c"][k][ok] != want["c"][k][ok]
        assert not diff.any(), (k, int(diff.sum()))


def test_fused_epoch_bits(runs):
    """Case e: the same state went in, the same state comes out (the finished case 5 untouched)."""
    got, want = runs
    assert set(got["e"]) == set(want["e"])
    for k in sorted(got["e"]):
        assert np.array_equal(got["e"][k], want["e"][k]), ("beam_rows_sizing_kernel<16, 7, 3>", k)
    for k in rb.EPOCH_STATE[:-1]:
        assert np.array_equal(got["e"]["post_" + k][5], got["e"]["pre_" + k][5]), k
    assert (got["e"]["post_status"].view(np.int32)[np.arange(9) != 5] == 0).all()
