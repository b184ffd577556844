"""Frame sizing with linked member groups on the GPU: ops_frame_group_step_f32 with the identity table bit for bit
against ops_frame_design_step_f32; its segment sum bit for bit against an explicit left-to-right host sum of the ungrouped entry's
gradient on the expanded state; Adam by group against the float64 reference; failed rows, idle designs, independence of the launch;
`frame_group_gradient` against autograd with one leaf per group; `optimize_grouped_frame_designs` bit for bit against
`optimize_frame_designs` (identity groups) and against the CPU oracle of the grouped loop (tests/golden/frame_groups_reference.npz,
tests/golden/make_frame_groups_golden.py); `evaluate_frame_designs` against the dense float64 objective; the catalogue step.

Helpers and tolerances are those of tests/test_gpu_frame_designs.py: the grouped loop adds a float64 sum to that arithmetic."""
import ctypes
import functools
import importlib.util
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import frame_dense as fd  # noqa: E402
from tests import frame_designs_ref as dr  # noqa: E402
from tests import frame_groups_ref as gr  # noqa: E402
from tests import frame_sizing_total_ref as ft  # noqa: E402
from tests import sizing_multicase_ref as mr  # noqa: E402
from tests import sizing_step_cases as sc  # noqa: E402
from tests import sizing_total_ref as tr  # noqa: E402
from tests import test_gpu_frame_designs as tdes  # noqa: E402
from tests.test_gpu_frame_designs import (DEV, MODES, SENT, STEP_FRAMES, StepRun, TOL_I, TOL_LOSS_20, _gpu, _kw, _ptr, _same, _states,  # noqa: E402,F401
                                          _stream, _table, _topology, _tuned_kernels_for_every_batch, _weights, case_gradients_numpy, lib,
                                          step_inputs, trajectory_deviation)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_groups_reference.npz")
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52


def tables(name):
    """kind -> labels of a frame: story, one, random, and on 15 x 16 a random table of 130 groups (a lane owns several)."""
    topo = _topology(name)
    out = {k: gr.group_table(topo, k) for k in ("story", "one", "random")}
    if name == "15x16":
        out["random130"] = gr.group_table(topo, "random", n_groups=130)
        assert out["random130"].max() + 1 == 130
    return out


def grouped_inputs(name, G, C, seed, labels):
    """`step_inputs` with linked variables: X, mX, vX [G,Ng] are the state of every group's first element, and I = X[labels]."""
    x = step_inputs(name, G, C, seed)
    ptr, elems = gr.csr(labels)
    first = elems[ptr[:-1]]
    x.labels, x.Ng = np.asarray(labels, dtype=np.int32), len(first)
    x.X, x.mX, x.vX = x.I[:, first].copy(), x.m[:, first].copy(), x.v[:, first].copy()
    x.I = x.X[:, labels].copy()
    x.I64 = x.I.astype(np.float64)
    return x


class GroupRun(StepRun):
    """The device arrays of one launch of ops_frame_group_step_f32 from `grouped_inputs`."""

    def __init__(self, x, st, extra, weights, status=None):
        super().__init__(x, st, extra, weights, status)
        self.X, self.exp_avg, self.exp_avg_sq = (_gpu(a, torch.float32) for a in (x.X, x.mX, x.vX))

    def groups(self, lib, hp, aggregate, schedule, optional=True):
        from openpystruct_amd import frame_groups, frames
        topo = self.x.topo
        adj = frames._adjoint_tables(topo)
        mg = frame_groups.member_groups(topo, self.x.labels)
        self.I64 = _gpu(self.x.I64)
        self.grad_out = torch.full((self.G, mg.Ng), SENT, dtype=torch.float64, device=DEV)
        rc = lib.ops_frame_group_step_f32(
            self.G, self.C, topo.Nn, topo.Ne, mg.Ng, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(),
            mg.d_elem_group.data_ptr(), mg.d_group_ptr.data_ptr(), mg.d_group_elems.data_ptr(), self.X.data_ptr(), self.I.data_ptr(),
            self.I64.data_ptr(), self.disp.data_ptr(), self.V.data_ptr(), self.M.data_ptr(), self.lam.data_ptr(), _ptr(self.extra),
            self.st_fwd.data_ptr(), self.st_adj.data_ptr(), _ptr(self.weights), aggregate,
            *(getattr(self, k).data_ptr() for k in self.STATE[1:8]), *(getattr(self, k).data_ptr() if optional else None for k in self.STATE[8:]),
            self.grad_out.data_ptr() if optional else None, ctypes.byref(hp), _ptr(schedule), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        return self


def _fresh(G):
    return types.SimpleNamespace(best=np.full(G, np.inf, dtype=np.float32), cnt=np.zeros(G, dtype=np.int32), t=np.zeros(G, dtype=np.int32),
                                 active=np.ones(G, dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# 1. identity is the design step, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(STEP_FRAMES))
def test_identity_groups_are_the_design_step_bit_for_bit(lib, name):
    """C = 1, 3 x G = 1, 5 x the three modes, with and without loss_extra, with the schedule table and with pow(); the designs of a
    launch take every early-stop state of `_states`."""
    topo = _topology(name)
    labels = gr.group_table(topo, "identity")
    hp = sc.frame_hp()
    table = _table(lib, hp)
    n = 0
    for C in (1, 3):
        for G in (1, 5):
            x = grouped_inputs(name, G, C, 0, labels)
            assert np.array_equal(x.X, x.I)
            for mode, (aggregate, weighted) in MODES.items():
                shift = (n := n + 1) % 5
                w = _weights(C) if weighted else None
                extra = x.extra if n % 2 else None
                st = _states(lib, x, extra, w, aggregate, hp, shift)
                for schedule in (table, None):
                    a = StepRun(x, st, extra, w).designs(lib, hp, aggregate, schedule)
                    b = GroupRun(x, st, extra, w).groups(lib, hp, aggregate, schedule)
                    for k in StepRun.STATE + ("I64", "grad_out"):
                        assert _same(getattr(b, k), getattr(a, k)), (name, C, G, mode, schedule is None, k)
                    assert _same(b.X, b.I)
                if G == 5:
                    assert set(st.kind) == set(sc.KINDS)
                o = GroupRun(x, st, extra, w).groups(lib, hp, aggregate, table, optional=False)      # the optional outputs NULL: the same state
                for k in StepRun.STATE[:8] + ("I64", "X"):
                    assert _same(getattr(o, k), getattr(b if schedule is table else GroupRun(x, st, extra, w).groups(lib, hp, aggregate, table), k)), k
                assert bool((o.case_penalty == SENT).all()) and bool((o.governing == -77).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. the segment sum, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(STEP_FRAMES))
def test_segment_sum_is_the_left_to_right_sum_of_the_ungrouped_gradient(lib, name):
    hp = sc.frame_hp()
    table = _table(lib, hp)
    G, C = 5, 3
    n = 0
    for kind, labels in tables(name).items():
        x = grouped_inputs(name, G, C, 1, labels)
        for mode, (aggregate, weighted) in MODES.items():
            shift = (n := n + 1) % 5
            w = _weights(C) if weighted else None
            extra = x.extra if n % 2 else None
            st = _states(lib, x, extra, w, aggregate, hp, shift)
            a = StepRun(x, st, extra, w).designs(lib, hp, aggregate, table)       # the ungrouped entry on the expanded state
            b = GroupRun(x, st, extra, w).groups(lib, hp, aggregate, table)
            what = (name, kind, mode)
            act = st.active == 1
            want = gr.segment_sum(a.grad_out.cpu().numpy()[act], labels)
            got = b.grad_out.cpu().numpy()
            assert np.array_equal(got[act].view(np.int64), want.view(np.int64)), what
            assert (got[~act] == SENT).all(), what
            for k in ("governing", "case_penalty", "last_loss", "best_loss", "patience_cnt", "epochs_run", "active"):
                assert _same(getattr(b, k), getattr(a, k)), what + (k,)
            idx = torch.as_tensor(labels.astype(np.int64), device=DEV)
            assert _same(b.I, b.X[:, idx].contiguous()), what
            assert bool(torch.isfinite(b.X).all())
            on = torch.as_tensor(act, device=DEV)
            went_on = on & b.active.bool()
            assert bool(went_on.any()) or G == 1
            assert _same(b.I64[went_on], b.I[went_on].double()) and _same(b.I64[~went_on], _gpu(x.I64)[~went_on]), what
            moved = (b.X[on] != _gpu(x.X, torch.float32)[on]).float().mean()
            assert float(moved) > 0.5, what


# ---------------------------------------------------------------------------------------------------------------------
# 3. Adam by group against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["story", "random"])
@pytest.mark.parametrize("name", ["4x2", "15x16"])
def test_group_step_against_the_float64_reference(lib, name, kind):
    """A numpy float64 step on the Ng variables (tests/sizing_total_ref.step_grad_reference) fed the host segment sum of the ungrouped
    entry's gradient; loss, penalties and the early stop from the design reference on the expanded state.  The bound (16 eps32) and
    the scales of tests/test_gpu_frame_designs.test_step_against_the_float64_reference."""
    from oracle import sizing_oracle as so
    hp = sc.frame_hp()
    G, C = 9, 3
    labels = tables(name)[kind]
    worst = {}
    for shift in range(3):
        x = grouped_inputs(name, G, C, 10 + shift, labels)
        grads = case_gradients_numpy(x, hp)
        for mode, (aggregate, weighted) in MODES.items():
            w = _weights(C) if weighted else None
            extra = x.extra if shift % 2 == 0 else None
            st, ref = mr.design_epoch(x.I, x.m, x.v, x.V, x.M, grads, extra, w, aggregate, hp, shift)
            table = _table(lib, hp)
            gX = gr.segment_sum(StepRun(x, st, extra, w).designs(lib, hp, aggregate, table).grad_out.cpu().numpy(), labels)
            act = st.active == 1
            zero = np.zeros_like(x.X, dtype=np.float64)
            adam = tr.step_grad_reference(x.X[act], x.mX[act], x.vX[act], zero[act], zero[act], gX[act], None, st.t[act], st.best[act], st.cnt[act], hp)
            want = dict({k: adam[k] for k in ("I", "exp_avg", "exp_avg_sq", "mag", "upd")}, loss=ref["loss"][act])
            b = GroupRun(x, st, extra, w).groups(lib, hp, aggregate, table)
            got = {k: getattr(b, k).cpu().numpy() for k in StepRun.STATE + ("X", "I64")}
            errs = so.sizing_step_errors(want, x.X[act], x.mX[act], x.vX[act], got["X"][act], got["exp_avg"][act], got["exp_avg_sq"][act],
                                         got["last_loss"][act], hp)
            P = ref["case_penalty"][act]
            errs["case_penalty"] = float((np.abs(got["case_penalty"][act] - P) / np.abs(P)).max() / sc.EPS32)
            print(name, kind, mode, shift, {k: round(e, 2) for k, e in errs.items()})
            for k, e in errs.items():
                worst[k] = max(worst.get(k, 0.0), e)
                assert e <= sc.STEP_BOUND, (mode, shift, k, e)
            assert np.array_equal(got["governing"][act], ref["governing"][act])
            assert np.array_equal(got["patience_cnt"][act], ref["cnt"][act]) and np.array_equal(got["active"][act] != 0, ~ref["stop"][act])
            assert np.array_equal(got["epochs_run"][act], st.t[act] + 1)
    print(f"{name} {kind}: worst errors in eps32 " + " ".join(f"{k} {e:.2f}" for k, e in worst.items()))


# ---------------------------------------------------------------------------------------------------------------------
# 4. failed rows and idle designs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_a_failed_row_gives_nan_exactly_as_the_ungrouped_entry_does(lib, mode):
    """One row with a non-zero forward status, another with a non-zero adjoint status (a status path: nothing is provoked on the
    device).  Under "sum" both designs are NaN; under "max" a design is NaN when the failed row governs it."""
    hp = sc.frame_hp()
    aggregate, weighted = MODES[mode]
    G, C = 5, 3
    labels = tables("4x2")["story"]
    x = grouped_inputs("4x2", G, C, 2, labels)
    w = _weights(C) if weighted else None
    z = _fresh(G)
    clean = GroupRun(x, z, x.extra, w).groups(lib, hp, aggregate, None)
    gov = clean.governing.cpu().numpy()
    status = np.zeros((2, G, C), dtype=np.int32)
    status[0, 1, gov[1]] = 1
    status[1, 3, (gov[3] + 1) % C] = 2
    a = StepRun(x, z, x.extra, w, status).designs(lib, hp, aggregate, None)
    b = GroupRun(x, z, x.extra, w, status).groups(lib, hp, aggregate, None)
    for k in ("governing", "case_penalty", "last_loss", "best_loss", "patience_cnt", "epochs_run", "active"):
        assert _same(getattr(b, k), getattr(a, k)), k
    nan_rows = [1, 3] if aggregate == mr.SUM else [1]
    for g in range(G):
        assert bool(torch.isnan(a.grad_out[g]).all()) == (g in nan_rows)
        for k in ("grad_out", "exp_avg", "exp_avg_sq"):
            assert bool(torch.isnan(getattr(b, k)[g]).all()) == (g in nan_rows), (g, k)
    assert _same(b.I[nan_rows], a.I[nan_rows])          # (fmaxf(NaN, clamp_min) is the clamp, in both entries)
    others = [g for g in range(G) if g not in nan_rows]
    for k in StepRun.STATE + ("X", "I64", "grad_out"):
        assert _same(getattr(b, k)[others], getattr(clean, k)[others]), k


@pytest.mark.parametrize("mode", list(MODES))
def test_a_design_does_not_depend_on_the_launch_and_idle_designs_write_nothing(lib, mode):
    """7 designs x 3 cases repeated 3000 times are bit-equal to the 7; the idle ones keep every bit of X, I, I64 and both moments and
    leave a sentinel-filled grad_out untouched."""
    hp = sc.frame_hp()
    aggregate, weighted = MODES[mode]
    G, C, reps = 7, 3, 3000
    labels = tables("4x2")["random"]
    x = grouped_inputs("4x2", G, C, 3, labels)
    w = _weights(C) if weighted else None
    st = _states(lib, x, x.extra, w, aggregate, hp, 1)
    assert (st.active == 0).any() and (st.active == 1).sum() >= 4
    small = GroupRun(x, st, x.extra, w).groups(lib, hp, aggregate, None)
    rep = lambda a: np.concatenate([a] * reps, axis=0)      # noqa: E731
    xb = types.SimpleNamespace(topo=x.topo, G=G * reps, C=C, labels=x.labels, Ng=x.Ng,
                               **{k: rep(getattr(x, k)) for k in ("I", "m", "v", "I64", "V", "M", "disp", "lam", "extra", "X", "mX", "vX")})
    stb = types.SimpleNamespace(**{k: rep(getattr(st, k)) for k in ("best", "cnt", "t", "active", "kind")})
    big = GroupRun(xb, stb, xb.extra, w).groups(lib, hp, aggregate, None)
    for k in StepRun.STATE + ("X", "I64", "grad_out"):
        s, b = getattr(small, k), getattr(big, k)
        assert _same(b.reshape((reps,) + tuple(s.shape)), s.unsqueeze(0).expand((reps,) + tuple(s.shape)).contiguous()), k
    idle = torch.as_tensor(st.active == 0, device=DEV)
    pre = GroupRun(x, st, x.extra, w)
    for k in StepRun.STATE + ("X",):
        assert _same(getattr(small, k)[idle], getattr(pre, k)[idle]), k
    assert _same(small.I64[idle], _gpu(x.I64)[idle]) and bool((small.grad_out[idle] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. frame_group_gradient
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grouped_designs(name, G=4, C=3):
    """`tests.test_gpu_frame_designs._designs` with story groups: X per group, I = X[groups], and the scales and kappa at that I."""
    d = tdes._designs(name, G, C)
    labels = gr.group_table(d.topo, "story")
    ptr, elems = gr.csr(labels)
    X = d.I[:, elems[ptr[:-1]]].copy()
    I = X[:, labels].copy()
    loads, w = d.loads.cpu().numpy(), d.w.cpu().numpy()
    rows = lambda obj: dr.rows_gradient(d.case, np.repeat(I, C, axis=0), loads.reshape(G * C, d.topo.Nn, 3),      # noqa: E731
                                        w.reshape(G * C, d.topo.Ne, 2), d.hp, obj)
    free = rows(ft.objective())
    hinged_obj = ft.objective(3.0, 0.5 * np.abs(free.outs[0][..., 0]).max(), 2.0, 0.5 * np.abs(free.outs[0][..., 1]).max())
    hinged = rows(hinged_obj)
    kappa = max(fd.cond_free(d.case, I[g]) for g in range(min(G, 3)))
    return types.SimpleNamespace(topo=d.topo, case=d.case, labels=labels, X=X, I=I, loads=d.loads, w=d.w, loads_np=loads, w_np=w, hp=d.hp,
                                 kappa=kappa, G=G, C=C, free=(ft.objective(), ft.grad_scale(d.case, free, free.lam)),
                                 hinged=(hinged_obj, ft.grad_scale(d.case, hinged, hinged.lam)))


@pytest.mark.parametrize("hinges", [False, True])
@pytest.mark.parametrize("name", ["2x3", "4x2"])
def test_group_gradient_matches_autograd_with_one_leaf_per_group(lib, name, hinges):
    import openpystruct_amd as oa
    d = _grouped_designs(name)
    obj, scale = d.hinged if hinges else d.free
    I = _gpu(d.I)
    factor = oa.frame_factor(d.topo, I)
    sol = oa.frame_resolve(factor, d.loads, d.w)
    assert int(sol.status.abs().sum()) == 0
    before = [t.clone() for t in (I, sol.disp, sol.V, sol.M, sol.forces, sol.status)]
    tol = max(1e-8, 4e-16 * d.kappa)
    for aggregate, weights in (("sum", None), ("sum", (1.0, 1.0, 0.5)), ("max", None)):
        agg = mr.MAX if aggregate == "max" else mr.SUM
        want = gr.group_gradient(d.case, d.X, d.labels, d.loads_np, d.w_np, d.hp, obj, agg, weights)
        grad, extra, gov = oa.frame_group_gradient(factor, sol, d.labels, d.hp, aggregate=aggregate, weights=weights, **_kw(obj))
        torch.cuda.synchronize()
        assert tuple(grad.shape) == d.X.shape and grad.dtype == torch.float64
        err = float(np.linalg.norm(grad.cpu().numpy() - want.grad) / max(np.linalg.norm(want.grad), scale))
        print(f"{name} hinges {hinges} {aggregate} {weights}: group gradient error {err:.3e} (bound {tol:.3e}, kappa {d.kappa:.3e})")
        assert err < tol, (err, tol)
        assert np.array_equal(gov.cpu().numpy(), want.governing)
        assert (extra is None) == (not hinges) and (extra is None or tuple(extra.shape) == (d.G, d.C))
    for t, b in zip((I, sol.disp, sol.V, sol.M, sol.forces, sol.status), before):
        assert _same(t, b)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the loop
# ---------------------------------------------------------------------------------------------------------------------
FRAMES = ("2x3", "4x2")
TAGS = ("sum", "weighted", "max")


def _generator():
    spec = importlib.util.spec_from_file_location("make_frame_groups_golden", os.path.join(ROOT, "tests", "golden", "make_frame_groups_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def _bits(r, hist):
    s = r.solution
    return (r.X, r.I, r.epochs, r.governing, r.case_penalty, s.disp, s.V, s.M, s.forces, s.status, hist)


@pytest.mark.parametrize("tag", TAGS)
def test_loop_with_identity_groups_is_optimize_frame_designs(lib, tag):
    """The 2 x 3 fixture of frame_sizing_designs_reference.npz: every result field and the loss history, bit for bit."""
    import openpystruct_amd as oa
    z, r, hist = tdes.run_loop(tag, "2x3", 10)
    cfg, obj, max_epochs, aggregate, weights = tdes._generator().runs("2x3")[tag]
    topo = _topology("2x3")
    h = []
    q = oa.optimize_grouped_frame_designs(topo, np.arange(topo.Ne), _gpu(z["2x3_loads"]), _gpu(z["2x3_w"]), cfg=cfg,
                                          X0=_gpu(z["2x3_I0"], torch.float32), aggregate=aggregate, weights=weights, max_epochs=max_epochs,
                                          poll_every=10, loss_history=h, **_kw(obj))
    assert q.discrete is None and _same(q.X, q.I)
    for a, b in zip(_bits(q, torch.stack(h))[1:], tdes._result_bits(r, hist)):
        assert _same(a, b)


def run_group_loop(tag, frame, poll_every):
    """optimize_grouped_frame_designs on the fixture's designs with the fixture's configuration -> (fixture, result, losses [epochs, G])."""
    import openpystruct_amd as oa
    mk = _generator()
    z = np.load(GOLDEN)
    cfg, obj, max_epochs, aggregate, weights = mk.runs(frame)[tag]
    p = f"{tag}_{frame}_"
    assert int(z[p + "max_epochs"]) == max_epochs and int(z[p + "aggregate"]) == ("sum", "max").index(aggregate)
    assert np.array_equal(z[p + "objective"], [obj.alpha_sway, obj.sway_limit, obj.alpha_deflection, obj.deflection_limit])
    assert np.array_equal(z[p + "weights"], [] if weights is None else weights)
    topo = _topology(frame)
    assert np.array_equal(z[f"{frame}_groups"], oa.story_groups(topo))
    hist = []
    r = oa.optimize_grouped_frame_designs(topo, z[f"{frame}_groups"], _gpu(z[f"{frame}_loads"]), _gpu(z[f"{frame}_w"]), cfg=cfg,
                                          X0=_gpu(z[f"{frame}_X0"], torch.float32), aggregate=aggregate, weights=weights, max_epochs=max_epochs,
                                          poll_every=poll_every, loss_history=hist, **_kw(obj))
    assert int(r.solution.status.abs().sum()) == 0
    return z, r, torch.stack(hist)


@pytest.mark.parametrize("tag", TAGS)
def test_grouped_loop_against_the_cpu_oracle(lib, tag):
    """Story groups, both frames, poll_every = 1 and 10 (the same bits); TOL_LOSS_20 and TOL_I of the ungrouped loop."""
    left_out, worst_I = [], 0.0
    for frame in FRAMES:
        z, r, hist = run_group_loop(tag, frame, 1)
        _, r10, hist10 = run_group_loop(tag, frame, 10)
        n = min(len(hist), len(hist10))
        for a, b in zip(_bits(r, hist[:n]), _bits(r10, hist10[:n])):
            assert _same(a, b)
        idx = torch.as_tensor(z[f"{frame}_groups"].astype(np.int64), device=DEV)
        assert _same(r.I, r.X[:, idx].contiguous())
        dev = trajectory_deviation(z, tag, frame, r, hist)
        print(tag, frame, dev)
        assert dev["loss_first20"] <= TOL_LOSS_20[tag], dev
        assert dev["governing"] == dev["governing_fixture"], dev
        for g in range(len(dev["epochs"])):
            if dev["epochs"][g] != dev["epochs_fixture"][g]:
                left_out.append((frame, g, dev["epochs"][g], dev["epochs_fixture"][g]))
            else:
                worst_I = max(worst_I, dev["I_rel_to_max"][g])
                assert dev["I_rel_to_max"][g] <= TOL_I[tag], (frame, g, dev)
    print(f"{tag}: left out of the final-X comparison (stop epoch differs): {left_out}; worst X deviation of the others {worst_I:.3e}")
    assert len(left_out) <= 1, left_out


# ---------------------------------------------------------------------------------------------------------------------
# 7. catalogue and evaluation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x3", "4x2"])
def test_evaluate_frame_designs_against_the_dense_objective(lib, name):
    import openpystruct_amd as oa
    d = tdes._designs(name)
    assert d.kappa * EPS64 < EPS32 / 100        # the solve's error cannot hide in the bound
    hp = d.hp
    I32 = d.I.astype(np.float32)
    loads, w = d.loads.cpu().numpy(), d.w.cpu().numpy()
    for obj in (d.free[0], d.hinged[0]):
        for aggregate, weights in (("sum", None), ("sum", (1.0, 1.0, 0.5)), ("max", None)):
            agg = mr.MAX if aggregate == "max" else mr.SUM
            L, P = dr.design_objective(d.case, torch.tensor(I32.astype(np.float64)), loads, w, hp, obj, agg, weights)
            L, P = L.numpy(), P.numpy()
            ev = oa.evaluate_frame_designs(d.topo, _gpu(I32, torch.float32), d.loads, d.w, aggregate=aggregate, weights=weights, **_kw(obj))
            assert int(ev.status.abs().sum()) == 0 and ev.value.dtype == torch.float32 and tuple(ev.case_penalty.shape) == (d.G, d.C)
            e_L = float((np.abs(ev.value.cpu().numpy() - L) / np.abs(L)).max() / EPS32)
            e_P = float((np.abs(ev.case_penalty.cpu().numpy() - P) / np.abs(P)).max() / EPS32)
            print(f"{name} {aggregate} {weights} hinges {obj.alpha_sway > 0}: value {e_L:.2f} case_penalty {e_P:.2f} eps32")
            assert e_L <= sc.STEP_BOUND and e_P <= sc.STEP_BOUND
            score = P if (agg == mr.MAX or weights is None) else P * np.asarray(weights)[None, :]
            assert np.array_equal(ev.governing.cpu().numpy(), np.argmax(score, axis=1))


def test_catalogue_step_and_the_dataset(lib):
    import openpystruct_amd as oa
    z = np.load(GOLDEN)
    frame = "4x2"
    topo = _topology(frame)
    groups = z[f"{frame}_groups"]
    loads, w, X0 = _gpu(z[f"{frame}_loads"]), _gpu(z[f"{frame}_w"]), _gpu(z[f"{frame}_X0"], torch.float32)
    kw = dict(aggregate="sum", weights=(1.0, 1.0, 0.5), alpha_sway=1.0, sway_limit=2e-3)
    free = oa.optimize_grouped_frame_designs(topo, groups, loads, w, X0=X0, max_epochs=60, **kw)
    assert free.discrete is None
    # 12 entries, geometric, spanning the run's own inertias -- but for the largest, which is above the catalogue
    catalogue = np.geomspace(float(free.X.min()) * 0.9, float(free.X.max()) * 0.98, 12)
    r = oa.optimize_grouped_frame_designs(topo, groups, loads, w, X0=X0, catalogue=catalogue, max_epochs=60, **kw)
    assert _same(r.X, free.X) and _same(r.I, free.I)
    d = r.discrete
    cat32 = torch.as_tensor(catalogue.astype(np.float32), device=DEV)
    assert d.X.dtype == torch.float32 and d.section.dtype == torch.int32 and d.clipped.dtype == torch.bool
    assert bool(torch.isin(d.X, cat32).all()) and _same(d.X, cat32[d.section.long()])
    assert bool(((d.X >= r.X) | d.clipped).all()) and bool(d.clipped.any()) and not bool(d.clipped.all())
    assert bool((d.X[d.clipped] == cat32[-1]).all()) and bool((r.X[d.clipped] > cat32[-1]).all())
    below = (d.section > 0) & ~d.clipped
    assert bool((cat32[(d.section.long() - 1).clamp(min=0)][below] < r.X[below]).all())      # "up": the entry below is below x
    idx = torch.as_tensor(groups.astype(np.int64), device=DEV)
    assert _same(d.I, d.X[:, idx].contiguous()) and _same(r.I, r.X[:, idx].contiguous())
    assert _same(d.value, oa.evaluate_frame_designs(topo, d.I, loads, w, **kw).value)
    assert _same(d.value_continuous, oa.evaluate_frame_designs(topo, r.I, loads, w, **kw).value)
    assert bool(torch.isfinite(d.value).all()) and not _same(d.value, d.value_continuous)
    near = oa.optimize_grouped_frame_designs(topo, groups, loads, w, X0=X0, catalogue=catalogue, snap="nearest", max_epochs=60, **kw)
    assert _same(near.X, r.X) and bool((near.discrete.X <= d.X).all()) and bool((near.discrete.X < d.X).any())
    # the dataset generator: the same fields on CPU tensors
    G, C = 3, 2
    rec = oa.generate_grouped_frame_design_dataset(4, 2, G, C, catalogue=catalogue, max_epochs=8, aggregate="max")
    Nn, Ne, Ng = topo.Nn, topo.Ne, 4
    shapes = dict(X=(G, Ng), groups=(Ne,), I=(G, Ne), lateral=(G, C), vertical=(G, C), V=(G, C, Ne), M=(G, C, Ne), disp=(G, C, Nn, 3),
                  epochs=(G,), status=(G, C), governing=(G,), case_penalty=(G, C), discrete_X=(G, Ng), discrete_section=(G, Ng),
                  discrete_I=(G, Ne), discrete_value=(G,), discrete_value_continuous=(G,), discrete_clipped=(G, Ng))
    assert {k: tuple(v.shape) for k, v in rec.items()} == shapes and all(not v.is_cuda for v in rec.values())
    assert np.array_equal(rec["groups"].numpy(), groups) and rec["epochs"].tolist() == [8] * G
    from openpystruct_amd import frames
    lat, ver = frames.frame_dataset_draws(G * C)
    ld, wd = frames.grid_load_cases(topo, lat, ver)
    direct = oa.optimize_grouped_frame_designs(topo, groups, ld.reshape(G, C, Nn, 3), wd.reshape(G, C, Ne, 2), catalogue=catalogue,
                                               max_epochs=8, aggregate="max")
    assert _same(direct.X.cpu(), rec["X"]) and _same(direct.discrete.X.cpu(), rec["discrete_X"])
    assert _same(direct.discrete.value.cpu(), rec["discrete_value"]) and _same(direct.discrete.I.cpu(), rec["discrete_I"])
    plain = oa.generate_grouped_frame_design_dataset(4, 2, G, C, max_epochs=8, aggregate="max")
    assert set(plain) == {k for k in shapes if not k.startswith("discrete_")} and _same(plain["X"], rec["X"])
