"""Host plumbing the two sizing loops share (openpystruct_amd/sizing_common.py) and the batch-stride packing of the beam entry
points (beam._rows).  CPU only: no launch is made."""
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
