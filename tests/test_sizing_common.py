"""Host plumbing the sizing loops share (openpystruct_amd/sizing_common.py) and the batch-stride packing of the beam entry
points (beam._rows).  CPU only: no launch is made."""
import glob
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("poll_every, expected", [(1, 4), (3, 6), (25, 10)])
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_run_epochs_polls_every_k_and_stops_when_no_row_is_active(poll_every, expected, kind):
    """Rows stop at epochs 2 and 4 of at most 10: the loop ends at the first multiple of `poll_every` at which no row is active (or
    at n_max), and `after_epoch` runs once after every epoch."""
    from openpystruct_amd.sizing_common import run_epochs
    active = np.ones(2, dtype=np.uint8) if kind == "numpy" else torch.ones(2, dtype=torch.uint8)
    log = []

    def epoch():
        log.append("e")
        n = log.count("e")
        if n == 2:
            active[0] = 0
        if n == 4:
            active[1] = 0

    assert run_epochs(epoch, 10, poll_every, active, lambda: log.append("a")) == expected
    assert log == ["e", "a"] * expected
    # without `after_epoch`, and with rows that never stop: n_max epochs
    count = []
    assert run_epochs(lambda: count.append(1), 7, poll_every, np.ones(2, dtype=np.uint8)) == 7 and len(count) == 7
    assert run_epochs(lambda: count.append(1), 0, poll_every, active) == 0 and len(count) == 7


def test_rows_packs_the_stride_of_every_shape_the_input_check_accepts():
    """x / fix: [N] shared or [B,N]; E / wy: one element or [B,Ne] -- (pointer, batch stride), stride 0 for what the batch shares."""
    from openpystruct_amd.beam import _rows
    B, N = 2, 4
    Ne = N - 1
    f64 = torch.float64
    for t, cols, stride in ((torch.zeros(N, dtype=f64), N, 0), (torch.zeros((B, N), dtype=f64), N, N),                  # x
                            (torch.zeros(N, dtype=torch.uint8), N, 0), (torch.zeros((B, N), dtype=torch.uint8), N, N),  # fix
                            (torch.tensor(2e11, dtype=f64), Ne, 0), (torch.zeros((B, Ne), dtype=f64), Ne, Ne),          # E, wy
                            (torch.zeros(1, dtype=f64), Ne, 0), (torch.zeros((1, 1), dtype=f64), 1, 0)):                # one element, any rank
        assert _rows(t, cols) == (t.data_ptr(), stride), (tuple(t.shape), cols)


def test_checked_aggregate_refusals_and_results():
    """The three refusals, each with its message; "max" never takes weights; the name alone (C None) leaves the weights unread."""
    from openpystruct_amd import multicase
    from openpystruct_amd.sizing_common import AGGREGATES, checked_aggregate
    assert multicase.AGGREGATES is AGGREGATES and AGGREGATES == ("sum", "max")
    with pytest.raises(ValueError, match=r"aggregate must be one of \('sum', 'max'\), got 'mean'"):
        checked_aggregate("mean", None, 2)
    for C in (None, 3):
        with pytest.raises(ValueError, match='aggregate="max" takes no weights: the governing case is the largest unweighted penalty'):
            checked_aggregate("max", (1.0, 1.0, 1.0), C)
    for bad in ((1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, float("inf"), 1.0)):
        with pytest.raises(ValueError, match="weights must be 3 finite non-negative numbers"):
            checked_aggregate("sum", bad, 3)
        assert checked_aggregate("sum", bad) == (0, bad)
    assert checked_aggregate("sum", None, 3) == (0, None) and checked_aggregate("max", None, 3) == (1, None)


def test_checked_aggregate_takes_a_list_an_array_and_a_tensor():
    from openpystruct_amd.sizing_common import checked_aggregate
    w = [0.5, 0.0, 2.0]
    got = [checked_aggregate("sum", v, 3) for v in (w, tuple(w), np.array(w, dtype=np.float32), torch.tensor(w), torch.tensor(w, dtype=torch.float64)[:, None])]
    for index, weights in got:
        assert index == 0 and weights.dtype == np.float64 and weights.shape == (3,) and weights.tolist() == w


def test_optimiser_state_arms_in_place():
    """The start values of all seven tensors, their shapes and dtypes; re-arming after an epoch's worth of scribbling restores them
    where they are (a captured graph points at them)."""
    from openpystruct_amd.sizing_common import OptimiserState, arm_optimiser_state, new_optimiser_state
    rows, n_vars = 3, 5
    s = new_optimiser_state(rows, n_vars, "cpu")
    assert OptimiserState._fields == ("exp_avg", "exp_avg_sq", "best", "patience_cnt", "epochs", "active", "last")      # the step entry points' order
    want = dict(exp_avg=(torch.float32, (rows, n_vars), 0.0), exp_avg_sq=(torch.float32, (rows, n_vars), 0.0), best=(torch.float32, (rows,), float("inf")),
                patience_cnt=(torch.int32, (rows,), 0), epochs=(torch.int32, (rows,), 0), active=(torch.uint8, (rows,), 1), last=(torch.float32, (rows,), 0.0))
    where = [t.data_ptr() for t in s]
    for scribble in (False, True):
        if scribble:
            for t in s:
                t.fill_(7)
        assert arm_optimiser_state(s) is s
        for name, (dtype, shape, value) in want.items():
            t = getattr(s, name)
            assert t.dtype == dtype and tuple(t.shape) == shape and bool((t == value).all()), name
        assert [t.data_ptr() for t in s] == where


def test_history_callback_and_the_recorded_history_of_the_driver():
    """The callback appends copies of `last`; the driver's eager branch stacks them to [epochs, rows], [0, rows] when no epoch ran,
    and returns no history when none is asked for (and no graph: nothing is captured without `use_graph`)."""
    from openpystruct_amd.sizing_common import history_callback, run_sizing_loop
    last, active = torch.zeros(4), torch.ones(4, dtype=torch.uint8)
    assert history_callback(None, last) is None
    hist = []
    after_epoch = history_callback(hist, last)
    for e in range(3):
        last.fill_(e)
        after_epoch()
    assert [h[0].item() for h in hist] == [0.0, 1.0, 2.0]          # copies, not views of `last`

    def epoch():
        last.add_(1.0)
        if last[0] == 7.0:
            active.zero_()

    graph, got = run_sizing_loop(epoch, 9, 2, active, last, "cpu", use_graph=False, record=True)      # 2.0 -> 7.0 at epoch 5, polled at 6
    assert graph is None and tuple(got.shape) == (6, 4) and got[:, 1].tolist() == [3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    graph, empty = run_sizing_loop(epoch, 0, 2, active, last, "cpu", use_graph=False, record=True)
    assert graph is None and tuple(empty.shape) == (0, 4) and empty.dtype == torch.float32
    assert run_sizing_loop(epoch, 3, 2, torch.ones(4, dtype=torch.uint8), last, "cpu", use_graph=False) == (None, None)


def test_the_step_size_table_is_stated_in_one_module():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hits = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(root, "openpystruct_amd", "*.py"))) if "ops_sizing_schedule_f32" in open(p).read()]
    assert hits == ["sizing_common.py"]
