"""The streaming kernels around the frame solve against the bits recorded before their node walk, end-node contraction and launch
were each stated once (tests/golden/frame_stream_parent_bits.npz, cases in tests/frame_stream_bits.py).  The library is built
without fast-math and without contraction, so every output is a function of the source-level order of operations, which that
change kept: no entry may move by a bit.  The NaN rows of failed frames are compared as NaN-ness, every other entry -- the rows
that must not be written included -- as bits."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import frame_stream_bits as fb  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATUS_ARRAYS = ("grad_contract_all", "grad_contract_gM", "load_vjp_all", "load_vjp_gM", "sizing_grad")


@pytest.fixture(scope="module")
def runs():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    spec = importlib.util.spec_from_file_location("make_frame_stream_parent_bits", os.path.join(GOLDEN, "make_frame_stream_parent_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return fb.run_all(), gen.unpack(np.load(gen.PATH))


@pytest.mark.parametrize("case", fb.CASES)
def test_stream_bits(runs, case):
    got, want = runs
    assert set(got[case]) == set(want[case])
    for k in sorted(got[case]):
        g, w = got[case][k], want[case][k]
        assert g.shape == w.shape, (case, k)
        if k == "replicas":
            continue
        nan_g, nan_w = np.isnan(g.view(np.float64)), np.isnan(w.view(np.float64))
        assert np.array_equal(nan_g, nan_w), (case, k, "NaN rows")
        diff = (g != w) & ~nan_w
        assert not diff.any(), (case, k, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("case", fb.CASES)
def test_rows_of_failed_and_inactive_frames(runs, case):
    """A frame that failed in either solve has NaN rows where the entry takes a status, and only there; the failed forward keeps the
    forces it had; an inactive frame's sizing rows are zeros (the right-hand side) or were not written (gradient, loss_extra)."""
    got, _ = runs
    f = {k: z.view(np.float64) for k, z in got[case].items() if k != "replicas"}
    bad = np.zeros(fb.B, dtype=bool)
    bad[[fb.FAILED_FWD, fb.FAILED_ADJ]] = True
    for k, z in f.items():
        rows = np.isnan(z.reshape(fb.B, -1)).all(axis=1)
        expect = bad if k in STATUS_ARRAYS else np.zeros(fb.B, dtype=bool)
        if k == "sizing_grad":
            expect = expect & (np.arange(fb.B) != fb.INACTIVE)
        assert rows.tolist() == expect.tolist(), (case, k)
        assert not np.isnan(z.reshape(fb.B, -1)[~expect]).any(), (case, k)
    want_forces = fb.inputs("g10x6" if case == "big" else case, fb.NODES[case], f["sizing_grad"].shape[1])["forces"][fb.FAILED_FWD]
    for v in ("pf", "sh"):
        assert np.array_equal(f["load_forces_" + v][fb.FAILED_FWD], want_forces), (case, v)
        assert (f["load_V_" + v][fb.FAILED_FWD] == fb.SENTINEL).all() and (f["load_M_" + v][fb.FAILED_FWD] == fb.SENTINEL).all()
    assert (f["sizing_grad"][fb.INACTIVE] == fb.SENTINEL).all() and f["sizing_extra_hinge"][fb.INACTIVE] == fb.SENTINEL
    assert (f["sizing_rhs_hinge"][fb.INACTIVE] == 0.0).all() and (f["sizing_rhs_plain"][fb.INACTIVE] == 0.0).all()


def test_every_replica_of_the_large_batch_equals_the_first(runs):
    """B = 7000 is more than one pass of the grid: the rows of the later passes (the grid-stride loop of the shared launch) hold
    what the first pass's hold."""
    got, want = runs
    assert got["big"]["replicas"].tolist() == [0] == want["big"]["replicas"].tolist()
