"""The five sizing loops, their dataset generators and the gradient entries beside them against the bits recorded before their host
side -- optimiser state, step-size table, loop driver, aggregate check, record fields -- was stated once
(tests/golden/sizing_loops_parent_bits.npz, cases in tests/sizing_loops_bits.py).  No launch changed and the library is built without
fast-math and without contraction, so no output may move by a bit: a wrong tensor, start value, table or loop branch would.  NaNs
are compared as NaN-ness, every other entry as bits."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import sizing_loops_bits as lb  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ([f"beam_{mode}_{run}" for mode in ("fused", "separate", "total") for run in ("graph", "record", "reuse0", "reuse1")]
         + [f"designs_{mode}_{run}" for mode in ("sum", "max") for run in ("graph", "record")]
         + ["dataset", "dataset_zero_last", "dataset_multicase", "frames_explicit", "frames_total_sway", "frames_total_loads",
            "frame_designs_shared_sum", "frame_designs_own_max", "frame_groups"] + list(lb.NOT_LOOPS))


@pytest.fixture(scope="module")
def runs():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    spec = importlib.util.spec_from_file_location("make_sizing_loops_parent_bits", os.path.join(GOLDEN, "make_sizing_loops_parent_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return lb.run_all(), gen.unpack(np.load(gen.PATH))


def test_the_cases_are_the_recorded_ones(runs):
    got, want = runs
    assert set(got) == set(want) == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_loop_bits(runs, case):
    got, want = runs
    assert set(got[case]) == set(want[case])
    for k in sorted(got[case]):
        g, w = got[case][k], want[case][k]
        assert g.shape == w.shape and g.dtype == w.dtype, (case, k)
        fw = lb.floats(k, w)
        nan_w = np.isnan(fw) if fw is not None else np.zeros(w.shape, dtype=bool)
        if fw is not None:
            assert np.array_equal(np.isnan(lb.floats(k, g)), nan_w), (case, k, "NaNs")
        diff = (g != w) & ~nan_w
        assert not diff.any(), (case, k, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    if case not in lb.NOT_LOOPS:      # what the record was made to hold: finished rows frozen while others went on past a poll
        assert all(lb.loop_condition(got[case])), (case, lb.epochs_of(got[case]).tolist())
