"""The multi-load-case sizing mode on the GPU: ops_beam_sizing_step_multicase_f32 against its float64 reference
(tests/sizing_multicase_ref.py) with the bounds and the early-stop states of the single-case step tests, its bit equalities (C = 1
is ops_beam_sizing_step_grad_f32; a design does not depend on its launch), the worst-case mode on constructed penalties, NaN
containment, refusals, and `optimize_designs` against the project's own CPU oracle of the loop
(tests/golden/sizing_multicase_reference.npz, tests/golden/make_sizing_multicase_golden.py).

Step errors (tests.test_gpu_sizing_step: in eps32, over the magnitude float32 round-off scales with), bound sc.STEP_BOUND = 16;
largest on the MI355X over all shapes: exp_avg 1.14, exp_avg_sq 1.69, I 1.83, loss 2.20 (the weighted sum of 16 cases).

Trajectory tolerances: at most 5 x the deviations one MI355X run recorded (profiles/sizing_multicase_deviation.json), the practice of
tests/test_gpu_sizing_total.py; stop epochs may differ by at most `patience`."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import sizing_multicase_ref as mr  # noqa: E402
from tests import sizing_step_cases as sc  # noqa: E402
from tests.test_gpu_sizing_step import SENT_F32, SENT_F64, SENT_I32, State, _same_bits, check_epoch, check_second_call  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
MODES = {"sum": (mr.SUM, False), "sum+weights": (mr.SUM, True), "max": (mr.MAX, False)}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi
    return _cabi.load()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _weights(C):
    return 0.25 + 1.5 * np.random.default_rng(C).uniform(size=C)


class DesignState(State):
    """The device arrays of one launch: the design state of `State` [G, ...] plus the rows [G*C, ...] and the optional outputs,
    pre-filled with sentinels; `active_rows` as the loop keeps it (0 in the rows of an inactive design)."""

    def __init__(self, I, m, v, st, C):
        super().__init__(I, m, v, st)
        G, Ne = I.shape
        self.C = C
        self.I64_rows = torch.full((G * C, Ne), float(SENT_F64), dtype=torch.float64, device=DEV)
        self.active_rows = _dev(np.repeat(st.active, C))
        self.case_penalty = torch.full((G * C,), float(SENT_F32), dtype=torch.float32, device=DEV)
        self.governing = torch.full((G,), int(SENT_I32), dtype=torch.int32, device=DEV)

    def snapshot(self):
        out = super().snapshot()          # I64, I_last, V32, M32, status: State's sentinel buffers, which no launch here is given
        G, Ne = self.shape
        out["I64_rows"] = self.I64_rows.cpu().numpy().reshape(G, self.C, Ne)
        out["I64"] = out["I64_rows"][:, 0].copy()            # check_epoch reads the first row; the others are compared with it
        out["active_rows"] = self.active_rows.cpu().numpy().reshape(G, self.C)
        out["case_penalty"] = self.case_penalty.cpu().numpy().reshape(G, self.C)
        out["governing"] = self.governing.cpu().numpy()
        return out


def _call(lib, s, n_designs, n_cases, n_elem, dV, dM, dg, de, dw, aggregate, params, sched, optional=True, **override):
    a = dict(G=n_designs, C=n_cases, Ne=n_elem, I=s.I.data_ptr(), I64_rows=s.I64_rows.data_ptr(), V=dV.data_ptr(), M=dM.data_ptr(), grad=dg.data_ptr(),
             loss_extra=None if de is None else de.data_ptr(), weights=None if dw is None else dw.data_ptr(), aggregate=aggregate,
             exp_avg=s.exp_avg.data_ptr(), exp_avg_sq=s.exp_avg_sq.data_ptr(), best_loss=s.best_loss.data_ptr(),
             patience_cnt=s.patience_cnt.data_ptr(), epochs_run=s.epochs_run.data_ptr(), active=s.active.data_ptr(),
             active_rows=s.active_rows.data_ptr(), last_loss=s.last_loss.data_ptr(),
             case_penalty=s.case_penalty.data_ptr() if optional else None, governing=s.governing.data_ptr() if optional else None,
             hp=ctypes.byref(params), schedule=None if sched is None else sched.data_ptr(), stream=_stream())
    a.update(override)
    return lib.ops_beam_sizing_step_multicase_f32(*a.values())


def _run(lib, I, m, v, V, M, grad, extra, weights, aggregate, st, hp, schedule=None, optional=True, calls=2):
    G, C, Ne = V.shape
    s = DesignState(I, m, v, st, C)
    dV, dM, dg = _dev(V.reshape(G * C, Ne)), _dev(M.reshape(G * C, Ne)), _dev(grad.reshape(G * C, Ne))
    de = None if extra is None else _dev(extra.reshape(G * C))
    dw = None if weights is None else _dev(weights)
    sched = None if schedule is None else _dev(schedule)
    snaps = [s.snapshot()]
    for _ in range(calls):
        assert _call(lib, s, G, C, Ne, dV, dM, dg, de, dw, aggregate, hp, sched, optional) == 0
        snaps.append(s.snapshot())
    return snaps


def _schedule(lib, hp):
    tab = np.zeros((hp.max_epochs, 2), dtype=np.float32)
    lib.ops_sizing_schedule_f32(ctypes.byref(hp), tab.ctypes.data)
    return tab


def check_rows(kernel, pre, post, st, ref, C, optional=True):
    """What `check_epoch` does not know of: all C rows of a design, the optional outputs."""
    idle, act = st.active == 0, st.active == 1
    stop, cont = act & ref["stop"], act & ~ref["stop"]
    for k in ("I64_rows", "active_rows", "case_penalty", "governing"):
        assert _same_bits(post[k][idle], pre[k][idle]), (kernel, k, "an inactive design was touched")
    # the widened inertias in ALL C rows of a design that goes on, none of one that stops
    assert _same_bits(post["I64_rows"][cont], np.repeat(post["I"][cont].astype(np.float64)[:, None, :], C, axis=1)), kernel
    assert _same_bits(post["I64_rows"][stop], SENT_F64), kernel
    assert (post["active_rows"][cont] == 1).all() and (post["active_rows"][stop] == 0).all(), kernel
    if not optional:
        assert _same_bits(post["case_penalty"], SENT_F32) and _same_bits(post["governing"], SENT_I32), kernel
        return
    if act.any():
        P = ref["case_penalty"][act]
        err = np.abs(post["case_penalty"][act].astype(np.float64) - P) / np.abs(P)
        assert err.max() <= sc.STEP_BOUND * sc.EPS32, (kernel, "case_penalty", err.max() / sc.EPS32)
        assert np.array_equal(post["governing"][act], ref["governing"][act]), kernel


def _score_margin(ref, weights):
    """Least ratio of the largest to the second largest w_c P_c: the governing case of these inputs is no matter of round-off."""
    s = np.sort(ref["case_penalty"] * (1.0 if weights is None else weights[None, :]), axis=1)
    return np.inf if s.shape[1] == 1 else float((s[:, -1] / s[:, -2]).min())


# ---------------------------------------------------------------------------------------------------------------------
# the step kernel against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
STEP_NE = [1, 64, 65, 100, 512]      # one lane; both sides of the first per-lane boundary; the workload's; the limit
STEP_C = [1, 2, 6, 16]
STEP_G = [1, 3, 9]                   # one design; a ragged block; with designs 4..7 inactive, a whole block of finished designs


@pytest.mark.parametrize("G", STEP_G)
@pytest.mark.parametrize("C", STEP_C)
@pytest.mark.parametrize("Ne", STEP_NE)
def test_step_multicase(lib, Ne, C, G):
    hp = sc.beam_hp()
    kernel = "ops_beam_sizing_step_multicase_f32"
    table = _schedule(lib, hp)
    for shift in range(5):
        I, m, v, V, M, grad, extra = mr.design_inputs(G, C, Ne, shift)
        for mode, (aggregate, weighted) in MODES.items():
            w = _weights(C) if weighted else None
            ex = extra if (shift + len(mode)) % 2 else None          # with and without the deflection term's value
            st, ref = mr.design_epoch(I, m, v, V, M, grad, ex, w, aggregate, hp, shift)
            assert _score_margin(ref, w) >= 1.0 + 1e-4
            for schedule in ((table, None) if shift in (0, 3) else (table,)):      # the table; pow() in the kernel
                pre, post, post2 = _run(lib, I, m, v, V, M, grad, ex, w, aggregate, st, hp, schedule=schedule)
                name = f"{kernel} {mode}"
                check_epoch(name, pre, post, st, ref, hp, sc.STEP_BOUND, wrote=("I64",))
                check_rows(name, pre, post, st, ref, C)
                check_second_call(name, post, post2, st, ref)
                cont = (st.active == 1) & ~ref["stop"]
                still = cont & (post2["active"] != 0)
                assert _same_bits(post2["I64_rows"][still], np.repeat(post2["I"][still].astype(np.float64)[:, None, :], C, axis=1))
                assert (post2["active_rows"] == np.repeat(post2["active"][:, None], C, axis=1)).all()
            # case_penalty == governing == NULL: the same state, bit for bit
            pre_n, post_n = _run(lib, I, m, v, V, M, grad, ex, w, aggregate, st, hp, schedule=table, optional=False, calls=1)
            check_rows(kernel, pre_n, post_n, st, ref, C, optional=False)
            for k in State.NAMES + ("I64_rows", "active_rows"):
                assert _same_bits(post_n[k], post[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# bit equalities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("G,Ne", [(1, 1), (5, 64), (9, 65), (9, 100), (3, 129), (5, 257), (2, 512)])
def test_one_case_is_the_single_case_step_bit_for_bit(lib, G, Ne, with_extra):
    """C = 1, the sum, no weights: every state field equals ops_beam_sizing_step_grad_f32's on the same inputs and I64_rows its I64,
    for every elements-per-lane instantiation (1, 2, 4, 8), with the schedule table and with pow()."""
    from tests import test_gpu_sizing_total as tt
    hp = sc.beam_hp()
    table = _schedule(lib, hp)
    for shift in range(5):
        I, m, v, V, M, grad, extra = mr.design_inputs(G, 1, Ne, shift)
        ex = extra if with_extra else None
        st, ref = mr.design_epoch(I, m, v, V, M, grad, ex, None, mr.SUM, hp, shift)
        for schedule in (table, None):
            one = tt._run_step_grad(lib, V[:, 0], M[:, 0], grad[:, 0], None if ex is None else ex[:, 0], I, m, v, st, hp, vm32=False,
                                    schedule=schedule)
            many = _run(lib, I, m, v, V, M, grad, ex, None, mr.SUM, st, hp, schedule=schedule)
            for a, b in zip(one, many):
                for k in ("I", "exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss", "I64"):
                    assert _same_bits(b[k], a[k]), (k, shift)
                assert _same_bits(b["I64_rows"][:, 0], a["I64"]) and np.array_equal(b["active_rows"][:, 0], a["active"])


@pytest.mark.parametrize("mode", list(MODES))
def test_a_design_does_not_depend_on_its_launch(lib, mode):
    """Design 0 alone (G = 1) equals design 0 of the G = 9 launch, in every bit; so does design 8, alone in the third block."""
    hp = sc.beam_hp()
    aggregate, weighted = MODES[mode]
    G, C, Ne = 9, 6, 100
    w = _weights(C) if weighted else None
    table = _schedule(lib, hp)
    I, m, v, V, M, grad, extra = mr.design_inputs(G, C, Ne, 0)
    st, ref = mr.design_epoch(I, m, v, V, M, grad, extra, w, aggregate, hp, 0)
    _, post = _run(lib, I, m, v, V, M, grad, extra, w, aggregate, st, hp, schedule=table, calls=1)
    for g in (0, 8):
        assert st.active[g] == 1
        sel = slice(g, g + 1)
        st1 = type(st)(**{k: a[sel] for k, a in vars(st).items()})
        _, alone = _run(lib, I[sel], m[sel], v[sel], V[sel], M[sel], grad[sel], extra[sel], w, aggregate, st1, hp, schedule=table, calls=1)
        for k in State.NAMES + ("I64_rows", "active_rows", "case_penalty", "governing"):
            assert _same_bits(alone[k], post[k][sel]), (k, g)


# ---------------------------------------------------------------------------------------------------------------------
# the worst-case mode on constructed penalties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales,governing", [((0.5, 0.7, 1.0), 2), ((0.5, 1.0, 0.7), 1), ((1.0, 0.5, 1.0), 0), ((0.5, 1.0, 1.0), 1)],
                         ids=["last", "middle", "tie-first-and-last", "tie-middle-and-last"])
def test_worst_case_governing(lib, scales, governing):
    """Every case of a design carries one row of forces scaled by `scales`: P_c grows with the scale, equal scales tie EXACTLY (the
    same float32 operations on the same numbers) and the lowest index governs.  The step then follows the governing row's gradient."""
    hp = sc.beam_hp()
    G, C, Ne = 5, 3, 65
    I, m, v, V, M, grad, _ = mr.design_inputs(G, C, Ne, 2)
    for c in range(C):
        V[:, c], M[:, c] = scales[c] * V[:, 0] / scales[0], scales[c] * M[:, 0] / scales[0]
    st, ref = mr.design_epoch(I, m, v, V, M, grad, None, None, mr.MAX, hp, 0)
    assert (ref["governing"] == governing).all()
    pre, post, post2 = _run(lib, I, m, v, V, M, grad, None, None, mr.MAX, st, hp, schedule=_schedule(lib, hp))
    check_epoch("worst case", pre, post, st, ref, hp, sc.STEP_BOUND, wrote=("I64",))
    check_rows("worst case", pre, post, st, ref, C)
    check_second_call("worst case", post, post2, st, ref)
    act = st.active == 1
    assert (post["governing"][act] == governing).all()
    ties = [c for c in range(C) if scales[c] == scales[governing]]
    for c in ties:
        assert _same_bits(post["case_penalty"][act][:, c], post["case_penalty"][act][:, governing])
    # the moments moved by the governing row's gradient, not by another row's: exp_avg = beta1 m + (1 - beta1) g to float32 round-off
    others = [c for c in range(C) if c != governing]
    want = hp.beta1 * m[act].astype(np.float64) + (1.0 - hp.beta1) * grad[act][:, governing].astype(np.float32).astype(np.float64)
    assert np.abs(post["exp_avg"][act] - want).max() <= 4 * sc.EPS32 * np.abs(want).max()
    for c in others:
        wrong = hp.beta1 * m[act].astype(np.float64) + (1.0 - hp.beta1) * grad[act][:, c].astype(np.float32).astype(np.float64)
        assert np.abs(post["exp_avg"][act] - wrong).max() > 1e-3 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------
# NaN containment, refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_a_nan_gradient_row_stays_in_its_design(lib, mode):
    hp = sc.beam_hp()
    aggregate, weighted = MODES[mode]
    G, C, Ne = 9, 3, 65
    w = _weights(C) if weighted else None
    I, m, v, V, M, grad, extra = mr.design_inputs(G, C, Ne, 0)
    st, ref = mr.design_epoch(I, m, v, V, M, grad, extra, w, aggregate, hp, 0)
    bad = 2
    assert st.active[bad] == 1 and st.active[[0, 3]].all()            # it shares its block with live designs
    _, clean = _run(lib, I, m, v, V, M, grad, extra, w, aggregate, st, hp, calls=1)
    g2 = grad.copy()
    g2[bad, int(ref["governing"][bad])] = np.nan
    _, dirty = _run(lib, I, m, v, V, M, g2, extra, w, aggregate, st, hp, calls=1)
    others = np.arange(G) != bad
    for k in State.NAMES + ("I64_rows", "active_rows", "case_penalty", "governing"):
        assert _same_bits(dirty[k][others], clean[k][others]), k
    assert np.isnan(dirty["exp_avg"][bad]).all()


def test_refusals_write_nothing(lib):
    from openpystruct_amd import _cabi
    hp = sc.beam_hp()
    G, C, Ne = 3, 2, 5
    I, m, v, V, M, grad, extra = mr.design_inputs(G, C, Ne, 0)
    st, _ = mr.design_epoch(I, m, v, V, M, grad, extra, None, mr.SUM, hp, 0)
    s = DesignState(I, m, v, st, C)
    dV, dM, dg, de, dw = _dev(V.reshape(G * C, Ne)), _dev(M.reshape(G * C, Ne)), _dev(grad.reshape(G * C, Ne)), _dev(extra.reshape(-1)), _dev(_weights(C))
    pre = s.snapshot()
    call = lambda **kw: _call(lib, s, G, C, Ne, dV, dM, dg, de, kw.pop("dw", None), kw.pop("agg", 0), hp, None, **kw)   # noqa: E731
    for k in ("I", "I64_rows", "V", "M", "grad", "exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active",
              "active_rows", "last_loss", "hp"):
        assert call(**{k: None}) == _cabi.ERR_INVALID_ARG, k
    for kw in ({"G": -1}, {"C": 0}, {"Ne": 0}, {"agg": 2}, {"agg": -1}, {"agg": 1, "dw": dw}):
        assert call(**kw) == _cabi.ERR_INVALID_ARG, kw
    assert call(Ne=513) == _cabi.ERR_UNSUPPORTED
    assert call(C=lib.ops_beam_sizing_multicase_max_cases() + 1) == _cabi.ERR_UNSUPPORTED
    assert call(G=0) == _cabi.OK
    post = s.snapshot()
    for k, a in pre.items():
        assert _same_bits(post[k], a), k


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden", "sizing_multicase_reference.npz")
TAGS = ("sum", "sum_defl", "max")
# at most 5 x the worst deviation of the recorded MI355X run (profiles/sizing_multicase_deviation.json): loss of the first 20 epochs
# 1.7e-7 (sum), 1.9e-7 (sum_defl), 1.3e-7 (max); final I over a design's largest inertia 1.4e-7, 1.6e-7, 2.6e-7; stop epochs and
# governing cases equal in all three runs
TOL_LOSS_20 = {"sum": 8.5e-7, "sum_defl": 9e-7, "max": 6e-7}
TOL_I = {"sum": 6.5e-7, "sum_defl": 7.5e-7, "max": 1.3e-6}


def fixture_run(tag, **kw):
    """optimize_designs on the fixture's cases of this run -> (fixture, cfg, cases, state)."""
    from openpystruct_amd import multicase
    from tests.golden import make_sizing_multicase_golden as mk
    z = np.load(GOLDEN)
    cfg, cases = mk.fixture_cases(tag)
    assert np.array_equal(cases.Fy.numpy(), z[f"{tag}_Fy"]) and np.array_equal(cases.fix.numpy(), z[f"{tag}_fix"]), "another case draw than the fixture's"
    alpha, limit = (float(t) for t in z[f"{tag}_objective"])
    gpu = type(cases)(*(t.to(DEV) for t in cases.tensors()))
    st = multicase.optimize_designs(gpu, cfg, DEV, int(z["C"]), aggregate=("sum", "max")[int(z[f"{tag}_aggregate"])],
                                    alpha_deflection=alpha, deflection_limit=limit if alpha > 0 else None, **kw)
    return z, cfg, cases, st


def _snapshot(st):
    torch.cuda.synchronize()
    return {k: getattr(st, k).cpu().numpy().copy() for k in ("I", "epochs_run", "V32", "M32", "last_loss", "I64_rows", "active",
                                                              "active_rows", "case_penalty", "governing", "best_loss")} | \
        {"v": st.sol.v.cpu().numpy().copy(), "theta": st.sol.theta.cpu().numpy().copy(), "status": st.sol.status.cpu().numpy().copy()}


def trajectory_deviation(z, tag, snap, hist):
    """The HIP loop against the fixture: worst relative deviation of the design loss over the first 20 epochs, worst deviation of
    the final I over a design's largest inertia (designs whose stop epochs coincide), the stop epochs."""
    ep, ref_ep = snap["epochs_run"], z[f"{tag}_epochs"]
    ref20 = z[f"{tag}_loss"][:, :20].astype(np.float64)
    same = ep == ref_ep
    dI = np.abs(snap["I"].astype(np.float64) - z[f"{tag}_I"]).max(-1) / z[f"{tag}_I"].max(-1)
    return {"loss_first20": float((np.abs(hist[:20].T.astype(np.float64) - ref20) / np.abs(ref20)).max()),
            "I_rel_to_max": float(dI[same].max()) if same.any() else None,
            "epochs": ep.tolist(), "epochs_fixture": ref_ep.tolist(),
            "governing": snap["governing"].tolist(), "governing_fixture": z[f"{tag}_governing"].tolist()}


@pytest.mark.parametrize("tag", TAGS)
def test_loop_against_the_cpu_oracle(lib, tag):
    z, cfg, cases, st = fixture_run(tag, record_loss=True)
    eager = _snapshot(st)
    hist = st.loss_history.cpu().numpy()
    dev = trajectory_deviation(z, tag, eager, hist)
    print(tag, dev)
    assert (eager["status"] == 0).all() and int(st.active.sum()) == 0 and int(st.active_rows.sum()) == 0
    assert (np.abs(eager["epochs_run"] - z[f"{tag}_epochs"]) <= cfg.patience).all(), dev
    assert dev["loss_first20"] <= TOL_LOSS_20[tag], dev
    assert dev["I_rel_to_max"] is not None and dev["I_rel_to_max"] <= TOL_I[tag], dev
    assert dev["governing"] == dev["governing_fixture"]
    C = int(z["C"])
    assert _same_bits(eager["I64_rows"].reshape(-1, C, st.Ne), np.repeat(eager["I64_rows"].reshape(-1, C, st.Ne)[:, :1], C, axis=1))
    # the captured graph: the same bits
    _, _, _, st_g = fixture_run(tag)
    graph = _snapshot(st_g)
    for k, a in eager.items():
        assert _same_bits(graph[k], a), ("graph", k)


@pytest.mark.parametrize("deflection", [False, True])
def test_one_load_case_is_the_total_mode_bit_for_bit(lib, deflection):
    """optimize_designs with C = 1 against optimize_cases(gradient="total") on the same cases."""
    from openpystruct_amd import multicase, sizing
    from tests.golden import make_sizing_multicase_golden as mk
    cfg, cases = mk.fixture_cases("sum")
    cfg = sizing.SizingConfig(**{**vars(cfg), "max_e": 40})
    gpu = type(cases)(*(t.to(DEV) for t in cases.tensors()))
    kw = dict(alpha_deflection=100.0, deflection_limit=0.01) if deflection else {}
    one = sizing.optimize_cases(gpu, cfg, DEV, gradient="total", **kw)
    many = multicase.optimize_designs(gpu, cfg, DEV, 1, **kw)
    torch.cuda.synchronize()
    for k in ("I", "epochs_run", "V32", "M32", "last_loss", "best_loss"):
        assert _same_bits(getattr(many, k).cpu().numpy(), getattr(one, k).cpu().numpy()), k
    assert _same_bits(many.I64_rows.cpu().numpy(), one.I64.cpu().numpy())
    assert _same_bits(many.sol.v.cpu().numpy(), one.sol.v.cpu().numpy())


def test_generate_multicase_dataset(lib):
    from openpystruct_amd import dataprep, multicase, sizing
    G, C = 4, 6
    cfg = sizing.SizingConfig(max_e=60)
    rec = multicase.generate_multicase_dataset(G, C, cfg, device=DEV)
    assert set(sizing.RECORD_KEYS) <= set(rec)
    Ne = cfg.num_elements
    assert rec["I_values"].shape == (G * C, Ne) and rec["I_values"].dtype == torch.float32
    for k in ("shear_forces", "bending_moments", "I_solved"):
        assert rec[k].shape == (G * C, Ne), k
    for k in ("deflections", "rotations", "node_positions"):
        assert rec[k].shape == (G * C, Ne + 1), k
    assert int(rec["status"].abs().sum()) == 0 and rec["status"].shape == (G * C,)
    assert rec["design_ids"].tolist() == [g for g in range(G) for _ in range(C)]
    assert rec["governing_case"].shape == (G,) and rec["case_penalty"].shape == (G, C) and rec["epochs_run"].shape == (G,)
    assert bool(((rec["governing_case"] >= 0) & (rec["governing_case"] < C)).all())
    assert torch.equal(rec["case_penalty"].argmax(dim=1).int(), rec["governing_case"])
    I = rec["I_values"].reshape(G, C, Ne)
    assert bool((I == I[:, :1]).all())
    # the C load cases of a design differ: its forces are C different solves on one I
    assert not torch.equal(rec["shear_forces"][0], rec["shear_forces"][1])
    d = dataprep.prepare(rec, kind="fnn", n_cases=C, perm=torch.arange(G), train_split=0.75)
    sy = d.scalers_Y["I"]
    labels = torch.cat([sy.inverse_transform(d.Y_train[:, :Ne]), sy.inverse_transform(d.Y_val[:, :Ne])]).cpu().numpy()
    design = I[:, 0].cpu().numpy()
    # (the bound of tests/test_sizing_multicase_host.py::test_dataprep_labels_grouped_records_with_the_design)
    assert np.abs(labels.astype(np.float64) - design).max() <= 32 * sc.EPS32 * float(design.max())
