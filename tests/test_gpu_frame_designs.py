"""Multi-load-case frame sizing on the GPU: ops_frame_design_rhs_f64 bit for bit against ops_frame_sizing_rhs_f64 on
the repeated rows; ops_frame_design_step_f32 bit for bit against the chain ops_frame_sizing_grad_f64 ->
ops_beam_sizing_step_multicase_f32, against the float64 reference of the design step (tests/sizing_multicase_ref.py), independent
of the launch; `frame_design_gradient` against autograd of the design objective with ONE leaf I (tests/frame_designs_ref.py) and
against central differences of the GPU forward; `optimize_frame_designs` against the project's own CPU oracle of the loop
(tests/golden/frame_sizing_designs_reference.npz, tests/golden/make_frame_sizing_designs_golden.py), against the rows path at C = 1,
and beside an explicit run of `optimize_frames`.

Trajectory tolerances: at most 5 x the deviations one MI355X run recorded (profiles/frame_designs_deviation.json), the practice of
tests/test_gpu_frame_sizing_total.py."""
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
from tests import frame_sizing_total_ref as ft  # noqa: E402
from tests import sizing_multicase_ref as mr  # noqa: E402
from tests import sizing_step_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_sizing_designs_reference.npz")
DEV = "cuda"
SENT = -98765.4321
MODES = {"sum": (mr.SUM, False), "sum+weights": (mr.SUM, True), "max": (mr.MAX, False)}


@pytest.fixture(autouse=True)
def _tuned_kernels_for_every_batch():
    """As tests/test_gpu_frame_sizing_total.py: library option frame_latency_batch = 0 (the tuned kernels for every batch); options
    are process-wide and put back after each test."""
    from openpystruct_amd import _cabi
    _cabi.set_option("frame_latency_batch", 0)
    yield
    _cabi.set_option("frame_latency_batch", -1)
    _cabi.set_option("frame_pack", 1)
    _cabi.set_option("frame_coop", 1)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi
    return _cabi.load()


def _gpu(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32}.get(t.element_size(), t.dtype)) if t.is_floating_point() else t


def _same(a, b):
    """Bit equality of two device tensors (NaN payloads included)."""
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def _topology(name):
    from openpystruct_amd import frames
    if name == "hub":
        return fd.hub_frame(DEV)
    bays, stories = (int(v) for v in name.split("x"))
    return frames.grid_frame(bays, stories, device=DEV)


def _cobj(obj):
    from openpystruct_amd import _cabi
    return _cabi.FrameSizingObjective(alpha_sway=obj.alpha_sway, sway_limit=obj.sway_limit, alpha_deflection=obj.alpha_deflection,
                                      deflection_limit=obj.deflection_limit)


def _weights(C):
    return 0.25 + 1.5 * np.random.default_rng(C).uniform(size=C)


# ---------------------------------------------------------------------------------------------------------------------
# the rhs entry: bit-equal to ops_frame_sizing_rhs_f64 on the repeated rows
# ---------------------------------------------------------------------------------------------------------------------
def _rhs_inputs(name, G, C):
    """Kernel inputs of G designs x C cases (not solutions of anything), in the style of tests/test_gpu_frame_sizing_total._synthetic."""
    topo = _topology(name)
    rng = np.random.default_rng([sum(map(ord, name)), G, C])
    I = fd.random_inertias(rng, G, topo.Ne)
    disp = rng.standard_normal((G, C, topo.Nn, 3)) * 1e-3
    disp[:, :, topo.fix3.all(axis=1)] = 0.0
    V, M = rng.standard_normal((G, C, topo.Ne)) * 1e4, rng.standard_normal((G, C, topo.Ne)) * 1e4
    return topo, tuple(_gpu(a) for a in (I, disp, V, M))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("name", ["1x1", "hub"])
def test_rhs_is_the_rows_entry_on_the_repeated_rows(lib, name, C, G, masked):
    from openpystruct_amd import frames
    topo, (I, disp, V, M) = _rhs_inputs(name, G, C)
    adj = frames._adjoint_tables(topo)
    hp, obj = ft.frame_hp(), _cobj(ft.objective(3.0, 5e-4, 2.0, 4e-4))
    active = _gpu((np.arange(G) % 2 == 0) if G > 1 else np.zeros(1), torch.uint8) if masked else None
    out = {}
    for which in ("rows", "designs"):
        rhs = torch.full((G, C, topo.Nn, 3), SENT, dtype=torch.float64, device=DEV)
        extra = torch.full((G, C), SENT, dtype=torch.float64, device=DEV)
        head = (topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr())
        tail = (disp.data_ptr(), V.data_ptr(), M.data_ptr(), ctypes.byref(hp), ctypes.byref(obj))
        if which == "rows":
            I_rows = I.repeat_interleave(C, 0).contiguous()
            act = None if active is None else active.repeat_interleave(C).contiguous()
            rc = lib.ops_frame_sizing_rhs_f64(G * C, *head, I_rows.data_ptr(), *tail, _ptr(act), rhs.data_ptr(), extra.data_ptr(), _stream())
        else:
            rc = lib.ops_frame_design_rhs_f64(G, C, *head, I.data_ptr(), *tail, _ptr(active), rhs.data_ptr(), extra.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        out[which] = (rhs, extra)
    assert _same(out["designs"][0], out["rows"][0]) and _same(out["designs"][1], out["rows"][1])
    rhs, extra = out["designs"]
    on = torch.ones(G, dtype=torch.bool, device=DEV) if active is None else active.bool()
    assert not bool((rhs == SENT).any()) and not bool((extra[on] == SENT).any())
    assert bool((rhs[~on] == 0.0).all()) and bool((extra[~on] == SENT).all())
    if bool(on.any()):
        assert bool((extra[on] > 0).any()) and bool((rhs[on] != 0.0).any())


# ---------------------------------------------------------------------------------------------------------------------
# the step entry
# ---------------------------------------------------------------------------------------------------------------------
def step_inputs(name, G, C, seed):
    """Seeded inputs of one design step of G designs x C cases on a frame: the optimiser state of sc.optimiser_state, forces of
    sc.random_forces per row, end displacements ~1e-3 and adjoint displacements ~1e-7 (per-case gradients of order 1 to 100), hinge
    values U(0, 50).  Numpy; I64 is the widened float32 design, as the loop keeps it."""
    topo = _topology(name)
    rng = np.random.default_rng([sum(map(ord, name)), G, C, seed, 5])
    I, m, v = sc.optimiser_state(rng, G, topo.Ne)
    V, M = sc.random_forces(rng, G * C, topo.Ne)
    disp = rng.standard_normal((G, C, topo.Nn, 3)) * 1e-3
    disp[:, :, topo.fix3.all(axis=1)] = 0.0
    lam = rng.standard_normal((G, C, topo.Nn, 3)) * 1e-7
    extra = rng.uniform(0.0, 50.0, size=(G, C))
    return types.SimpleNamespace(topo=topo, G=G, C=C, I=I, m=m, v=v, I64=I.astype(np.float64), V=V.reshape(G, C, topo.Ne),
                                 M=M.reshape(G, C, topo.Ne), disp=disp, lam=lam, extra=extra)


def case_gradients_numpy(x, hp):
    """fs_elem_grad of every (design, case, element) in numpy float64: explicit part + (g_f - lambda) . (K_b u)."""
    topo = x.topo
    L, c, s = (topo.d_geo.cpu().numpy()[:, k] for k in range(3))
    E, conn = topo.E, topo.conn
    I = x.I64[:, None, :]
    qV, qM = x.V / (hp.G * hp.area_coef * np.sqrt(I)), x.M / (2.0 * hp.E * I + hp.bend_eps)
    gf = np.zeros(x.V.shape + (6,))
    gf[..., 1], gf[..., 2] = 2.0 * hp.alpha_shear * qV, 2.0 * hp.alpha_moment * qM
    explicit = 1.0 - hp.alpha_moment * 2.0 * hp.E * qM ** 2 - hp.alpha_shear * (0.5 * x.V * qV) / I
    ends = lambda a: np.concatenate([a[:, :, conn[:, 0]], a[:, :, conn[:, 1]]], axis=-1)      # noqa: E731  [G,C,Ne,6]
    u, lam = ends(x.disp), ends(x.lam)
    ul = [c * u[..., 0] + s * u[..., 1], -s * u[..., 0] + c * u[..., 1], u[..., 2], c * u[..., 3] + s * u[..., 4], -s * u[..., 3] + c * u[..., 4], u[..., 5]]
    rL = 1.0 / L
    chord, b2 = (ul[4] - ul[1]) * rL, 2.0 * E * rL
    q1 = 2.0 * b2 * (ul[2] - chord) + b2 * (ul[5] - chord)
    q2 = b2 * (ul[2] - chord) + 2.0 * b2 * (ul[5] - chord)
    sh = (q1 + q2) * rL
    y = np.stack([-s * sh, c * sh, q1, s * sh, -c * sh, q2], axis=-1)
    return explicit + ((gf - lam) * y).sum(-1)


class StepRun:
    """The device arrays of one launch of either path, from the same numpy inputs."""

    def __init__(self, x, st, extra, weights, status=None):
        G, C, Ne = x.G, x.C, x.topo.Ne
        f32, f64, i32 = (lambda a, t=t: _gpu(a, t) for t in (torch.float32, torch.float64, torch.int32))
        self.x, self.G, self.C, self.Ne = x, G, C, Ne
        self.I, self.exp_avg, self.exp_avg_sq = f32(x.I), f32(x.m), f32(x.v)
        self.best_loss, self.patience_cnt, self.epochs_run = f32(st.best), i32(st.cnt), i32(st.t)
        self.active = _gpu(st.active, torch.uint8)
        self.last_loss = torch.full((G,), SENT, dtype=torch.float32, device=DEV)
        self.case_penalty = torch.full((G, C), SENT, dtype=torch.float32, device=DEV)
        self.governing = torch.full((G,), -77, dtype=torch.int32, device=DEV)
        self.V, self.M, self.disp, self.lam = f64(x.V), f64(x.M), f64(x.disp), f64(x.lam)
        self.extra = None if extra is None else f64(extra)
        self.weights = None if weights is None else f64(weights)
        self.st_fwd = i32(np.zeros((G, C)) if status is None else status[0])
        self.st_adj = i32(np.zeros((G, C)) if status is None else status[1])

    STATE = ("I", "exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss", "case_penalty", "governing")

    def designs(self, lib, hp, aggregate, schedule, optional=True):
        """ops_frame_design_step_f32; I64 [G,Ne] and grad_out end up in self.I64 / self.grad_out."""
        from openpystruct_amd import frames
        topo = self.x.topo
        adj = frames._adjoint_tables(topo)
        self.I64 = _gpu(self.x.I64)
        self.grad_out = torch.full((self.G, self.Ne), SENT, dtype=torch.float64, device=DEV)
        rc = lib.ops_frame_design_step_f32(
            self.G, self.C, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(), self.I.data_ptr(),
            self.I64.data_ptr(), self.disp.data_ptr(), self.V.data_ptr(), self.M.data_ptr(), self.lam.data_ptr(), _ptr(self.extra),
            self.st_fwd.data_ptr(), self.st_adj.data_ptr(), _ptr(self.weights), aggregate,
            *(getattr(self, k).data_ptr() for k in self.STATE[1:8]), *(getattr(self, k).data_ptr() if optional else None for k in self.STATE[8:]),
            self.grad_out.data_ptr() if optional else None, ctypes.byref(hp), _ptr(schedule), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        return self

    def chain(self, lib, hp, aggregate, schedule):
        """ops_frame_sizing_grad_f64 on the G * C rows with I repeated, then ops_beam_sizing_step_multicase_f32."""
        from openpystruct_amd import frames
        topo = self.x.topo
        adj = frames._adjoint_tables(topo)
        G, C = self.G, self.C
        self.I64_rows = _gpu(np.repeat(self.x.I64, C, axis=0))
        self.active_rows = self.active.repeat_interleave(C).contiguous()
        self.grad_rows = torch.zeros((G * C, self.Ne), dtype=torch.float64, device=DEV)
        rc = lib.ops_frame_sizing_grad_f64(G * C, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(),
                                           self.I64_rows.data_ptr(), self.disp.data_ptr(), self.V.data_ptr(), self.M.data_ptr(),
                                           self.lam.data_ptr(), ctypes.byref(hp), self.active_rows.data_ptr(), self.st_fwd.data_ptr(),
                                           self.st_adj.data_ptr(), self.grad_rows.data_ptr(), _stream())
        assert rc == 0
        rc = lib.ops_beam_sizing_step_multicase_f32(
            G, C, self.Ne, self.I.data_ptr(), self.I64_rows.data_ptr(), self.V.data_ptr(), self.M.data_ptr(), self.grad_rows.data_ptr(),
            _ptr(self.extra), _ptr(self.weights), aggregate, *(getattr(self, k).data_ptr() for k in self.STATE[1:7]),
            self.active_rows.data_ptr(), self.last_loss.data_ptr(), self.case_penalty.data_ptr(), self.governing.data_ptr(),
            ctypes.byref(hp), _ptr(schedule), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        self.I64 = self.I64_rows.reshape(G, C, self.Ne)[:, 0].contiguous()
        return self


def _table(lib, hp):
    tab = np.zeros((hp.max_epochs, 2), dtype=np.float32)
    lib.ops_sizing_schedule_f32(ctypes.byref(hp), tab.ctypes.data)
    return _gpu(tab, torch.float32)


def _states(lib, x, extra, weights, aggregate, hp, shift):
    """Early-stop states of the designs (sc.case_states: improving, idle, stopping by patience, stopping by max_epochs, not improving;
    t = 0, 1, 17 and max_epochs - 1), every decision 2e-3 away from its threshold: placed from the chain's own loss of a first epoch."""
    G = x.G
    z = types.SimpleNamespace(best=np.full(G, np.inf, dtype=np.float32), cnt=np.zeros(G, dtype=np.int32), t=np.zeros(G, dtype=np.int32),
                              active=np.ones(G, dtype=np.uint8))
    loss = StepRun(x, z, extra, weights).chain(lib, hp, aggregate, None).last_loss.cpu().numpy().astype(np.float64)
    return sc.case_states(loss, hp, shift, 4)


def _compare(a, b, what):
    """Every field of the design step's state, and I64, bit for bit."""
    for k in StepRun.STATE + ("I64",):
        assert _same(getattr(a, k), getattr(b, k)), (what, k)


# frame -> elements per lane of the step kernel (Ne: 3, 18, 75, 210, 496)
STEP_FRAMES = {"1x1": 1, "4x2": 1, "7x5": 2, "10x10": 4, "15x16": 8}


@pytest.mark.parametrize("name", list(STEP_FRAMES))
def test_step_is_the_chain_bit_for_bit(lib, name):
    """C = 1, 2, 3 x G = 1, 5, 9 x both aggregates, with and without weights and loss_extra, with the schedule table and with pow();
    the designs of a launch take every early-stop state (one stops by patience, one by max_epochs, one is idle) and t = 0 and t > 0."""
    topo = _topology(name)
    K = 1 if topo.Ne <= 64 else 2 if topo.Ne <= 128 else 4 if topo.Ne <= 256 else 8
    assert K == STEP_FRAMES[name]
    hp = sc.frame_hp()
    table = _table(lib, hp)
    n = 0
    for C in (1, 2, 3):
        for G in (1, 5, 9):
            x = step_inputs(name, G, C, 0)
            for mode, (aggregate, weighted) in MODES.items():
                shift = (n := n + 1) % 5
                w = _weights(C) if weighted else None
                extra = x.extra if n % 2 else None
                st = _states(lib, x, extra, w, aggregate, hp, shift)
                for schedule in ((table, None) if n % 3 == 0 else (table,)):
                    a = StepRun(x, st, extra, w).chain(lib, hp, aggregate, schedule)
                    b = StepRun(x, st, extra, w).designs(lib, hp, aggregate, schedule)
                    _compare(b, a, (name, C, G, mode, schedule is None))
                    act = torch.as_tensor(st.active, device=DEV).bool()
                    assert bool(torch.isfinite(b.I).all()) and not bool((b.grad_out[act] == SENT).any()) and bool((b.grad_out[~act] == SENT).all())
                    if G == 5:      # the launch held a design that stops by patience, one by max_epochs, an idle one and two that go on
                        assert set(st.kind) == set(sc.KINDS) and int(b.active.sum()) == 2
                    went_on = act & b.active.bool()
                    assert _same(b.I64[went_on], b.I[went_on].double()) and _same(b.I64[~went_on], _gpu(x.I64)[~went_on])
                # the optional outputs NULL: the same state
                o = StepRun(x, st, extra, w).designs(lib, hp, aggregate, table, optional=False)
                ref = StepRun(x, st, extra, w).designs(lib, hp, aggregate, table)
                for k in StepRun.STATE[:8] + ("I64",):
                    assert _same(getattr(o, k), getattr(ref, k)), k
                assert bool((o.case_penalty == SENT).all()) and bool((o.governing == -77).all())


def test_step_sixty_four_cases(lib):
    hp = sc.frame_hp()
    x = step_inputs("1x1", 5, 64, 1)
    for mode, (aggregate, weighted) in MODES.items():
        w = _weights(64) if weighted else None
        st = _states(lib, x, x.extra, w, aggregate, hp, 0)
        _compare(StepRun(x, st, x.extra, w).designs(lib, hp, aggregate, None), StepRun(x, st, x.extra, w).chain(lib, hp, aggregate, None), mode)


@pytest.mark.parametrize("mode", list(MODES))
def test_a_failed_row_gives_nan_exactly_as_the_chain_does(lib, mode):
    """One row with a non-zero forward status, another with a non-zero adjoint status (a status path: nothing is provoked on the
    device).  Under "sum" both designs are NaN; under "max" a design is NaN when the failed row governs it."""
    hp = sc.frame_hp()
    aggregate, weighted = MODES[mode]
    G, C = 5, 3
    x = step_inputs("4x2", G, C, 2)
    w = _weights(C) if weighted else None
    z = types.SimpleNamespace(best=np.full(G, np.inf, dtype=np.float32), cnt=np.zeros(G, dtype=np.int32), t=np.zeros(G, dtype=np.int32),
                              active=np.ones(G, dtype=np.uint8))
    clean = StepRun(x, z, x.extra, w).designs(lib, hp, aggregate, None)
    gov = clean.governing.cpu().numpy()
    status = np.zeros((2, G, C), dtype=np.int32)
    status[0, 1, gov[1]] = 1                       # the governing row of design 1: NaN under either aggregate
    status[1, 3, (gov[3] + 1) % C] = 2             # a row that does not govern design 3: NaN under "sum" only
    a = StepRun(x, z, x.extra, w, status).chain(lib, hp, aggregate, None)
    b = StepRun(x, z, x.extra, w, status).designs(lib, hp, aggregate, None)
    _compare(b, a, mode)
    nan_rows = [1, 3] if aggregate == mr.SUM else [1]
    for g in range(G):
        assert bool(torch.isnan(b.exp_avg[g]).all()) == (g in nan_rows) and bool(torch.isnan(b.grad_out[g]).all()) == (g in nan_rows), g
    others = [g for g in range(G) if g not in nan_rows]
    for k in StepRun.STATE:
        assert _same(getattr(b, k)[others], getattr(clean, k)[others]), k


@pytest.mark.parametrize("name", ["4x2", "7x5", "15x16"])
def test_step_against_the_float64_reference(lib, name):
    """tests/sizing_multicase_ref.design_step_reference fed the float64 per-case gradients of fs_elem_grad formed in numpy: the
    bound (16 eps32) and the scales of tests/test_gpu_sizing_multicase.py."""
    from oracle import sizing_oracle as so
    hp = sc.frame_hp()
    G, C = 9, 3
    worst = {}
    for shift in range(3):
        x = step_inputs(name, G, C, 10 + shift)
        grads = case_gradients_numpy(x, hp)
        for mode, (aggregate, weighted) in MODES.items():
            w = _weights(C) if weighted else None
            extra = x.extra if shift % 2 == 0 else None
            st, ref = mr.design_epoch(x.I, x.m, x.v, x.V, x.M, grads, extra, w, aggregate, hp, shift)
            s = np.sort(ref["case_penalty"] * (1.0 if w is None else w[None, :]), axis=1)
            assert (s[:, -1] / s[:, -2]).min() >= 1.0 + 1e-4
            b = StepRun(x, st, extra, w).designs(lib, hp, aggregate, _table(lib, hp))
            act = st.active == 1
            got = {k: getattr(b, k).cpu().numpy() for k in StepRun.STATE + ("grad_out", "I64")}
            errs = so.sizing_step_errors({k: a[act] for k, a in ref.items()}, x.I[act], x.m[act], x.v[act], got["I"][act], got["exp_avg"][act],
                                         got["exp_avg_sq"][act], got["last_loss"][act], hp)
            P = ref["case_penalty"][act]
            errs["case_penalty"] = float((np.abs(got["case_penalty"][act] - P) / np.abs(P)).max() / sc.EPS32)
            want_g = mr.group_gradient(grads, w, aggregate, ref["governing"])[act]
            errs["grad_out"] = float(np.abs(got["grad_out"][act] - want_g).max() / np.abs(want_g).max() / 2.0 ** -52)      # in eps64
            for k, e in errs.items():
                worst[k] = max(worst.get(k, 0.0), e)
            for k in ("exp_avg", "exp_avg_sq", "I", "loss", "case_penalty"):
                assert errs[k] <= sc.STEP_BOUND, (mode, shift, k, errs[k])
            assert errs["grad_out"] <= 1e4, errs                                   # float64 round-off of a sum of terms of mixed sign
            assert np.array_equal(got["governing"][act], ref["governing"][act])
            assert np.array_equal(got["patience_cnt"][act], ref["cnt"][act]) and np.array_equal(got["active"][act] != 0, ~ref["stop"][act])
            assert np.array_equal(got["epochs_run"][act], st.t[act] + 1)
    print(f"{name}: worst errors in eps32 (grad_out in eps64) " + " ".join(f"{k} {e:.2f}" for k, e in worst.items()))


@pytest.mark.parametrize("mode", list(MODES))
def test_a_design_does_not_depend_on_the_launch_and_idle_designs_write_nothing(lib, mode):
    """7 designs x 3 cases repeated 3000 times (21 000 designs, 5250 blocks) are bit-equal to the 7; the idle ones keep every bit."""
    hp = sc.frame_hp()
    aggregate, weighted = MODES[mode]
    G, C, reps = 7, 3, 3000
    x = step_inputs("1x1", G, C, 3)
    w = _weights(C) if weighted else None
    st = _states(lib, x, x.extra, w, aggregate, hp, 1)
    assert (st.active == 0).any() and (st.active == 1).sum() >= 4
    small = StepRun(x, st, x.extra, w).designs(lib, hp, aggregate, None)
    rep = lambda a: np.concatenate([a] * reps, axis=0)      # noqa: E731
    xb = types.SimpleNamespace(topo=x.topo, G=G * reps, C=C, **{k: rep(getattr(x, k)) for k in ("I", "m", "v", "I64", "V", "M", "disp", "lam", "extra")})
    stb = types.SimpleNamespace(**{k: rep(getattr(st, k)) for k in ("best", "cnt", "t", "active", "kind")})
    big = StepRun(xb, stb, xb.extra, w).designs(lib, hp, aggregate, None)
    for k in StepRun.STATE + ("I64", "grad_out"):
        s, b = getattr(small, k), getattr(big, k)
        assert _same(b.reshape((reps,) + tuple(s.shape)), s.unsqueeze(0).expand((reps,) + tuple(s.shape)).contiguous()), k
    idle = torch.as_tensor(st.active == 0, device=DEV)
    pre = StepRun(x, st, x.extra, w)
    for k in StepRun.STATE:
        assert _same(getattr(small, k)[idle], getattr(pre, k)[idle]), k
    assert _same(small.I64[idle], _gpu(x.I64)[idle]) and bool((small.grad_out[idle] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# frame_design_gradient
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _designs(name, G=4, C=3):
    """G designs x C cases of a frame (wind from either side with gravity, 1.5 x gravity alone) and their dense-model rows, once."""
    from openpystruct_amd import frames
    topo = _topology(name)
    case = fd.case_of(topo)
    rng = np.random.default_rng(sum(map(ord, name)) + G)
    I = fd.random_inertias(rng, G, topo.Ne)
    H, q = rng.uniform(0.5e4, 2e4, size=G), rng.uniform(-2e4, -0.5e4, size=G)
    loads, w = frames.grid_load_cases(topo, np.stack([H, -H, 0 * H], 1).reshape(-1), np.stack([q, q, 1.5 * q], 1).reshape(-1))
    loads, w = loads.reshape(G, C, topo.Nn, 3), w.reshape(G, C, topo.Ne, 2)
    hp = ft.frame_hp()
    rows = lambda obj: dr.rows_gradient(case, np.repeat(I, C, axis=0), loads.cpu().numpy().reshape(G * C, topo.Nn, 3),      # noqa: E731
                                        w.cpu().numpy().reshape(G * C, topo.Ne, 2), hp, obj)
    free = rows(ft.objective())
    hinged_obj = ft.objective(3.0, 0.5 * np.abs(free.outs[0][..., 0]).max(), 2.0, 0.5 * np.abs(free.outs[0][..., 1]).max())
    hinged = rows(hinged_obj)
    kappa = max(fd.cond_free(case, I[g]) for g in range(min(G, 3)))
    return types.SimpleNamespace(topo=topo, case=case, I=I, loads=loads, w=w, hp=hp, kappa=kappa, G=G, C=C,
                                 free=(ft.objective(), ft.grad_scale(case, free, free.lam)),
                                 hinged=(hinged_obj, ft.grad_scale(case, hinged, hinged.lam)))


def _kw(obj):
    return {} if obj.alpha_sway + obj.alpha_deflection == 0.0 else dict(alpha_sway=obj.alpha_sway, sway_limit=obj.sway_limit,
                                                                         alpha_deflection=obj.alpha_deflection, deflection_limit=obj.deflection_limit)


@pytest.mark.parametrize("hinges", [False, True])
@pytest.mark.parametrize("name", ["2x3", "4x2"])
def test_design_gradient_matches_autograd_with_one_leaf(lib, name, hinges):
    """On the GPU's own factor and re-solve; the bound of tests/test_gpu_frame_sizing_total.py, relative to the size of the terms
    the rows' gradients are sums of.  The caller's tensors keep every bit."""
    import openpystruct_amd as oa
    d = _designs(name)
    obj, scale = d.hinged if hinges else d.free
    I = _gpu(d.I)
    factor = oa.frame_factor(d.topo, I)
    sol = oa.frame_resolve(factor, d.loads, d.w)
    assert int(sol.status.abs().sum()) == 0
    before = [t.clone() for t in (I, sol.disp, sol.V, sol.M, sol.forces, sol.status)]
    tol = max(1e-8, 4e-16 * d.kappa)
    for aggregate, weights in (("sum", None), ("sum", (1.0, 1.0, 0.5)), ("max", None)):
        agg = mr.MAX if aggregate == "max" else mr.SUM
        want = dr.design_gradient(d.case, d.I, d.loads.cpu().numpy(), d.w.cpu().numpy(), d.hp, obj, agg, weights)
        grad, extra, gov = oa.frame_design_gradient(factor, sol, d.hp, aggregate=aggregate, weights=weights, **_kw(obj))
        torch.cuda.synchronize()
        err = float(np.linalg.norm(grad.cpu().numpy() - want.grad) / max(np.linalg.norm(want.grad), scale))
        print(f"{name} hinges {hinges} {aggregate} {weights}: gradient error {err:.3e} (bound {tol:.3e}, kappa {d.kappa:.3e})")
        assert err < tol, (err, tol)
        assert np.array_equal(gov.cpu().numpy(), want.governing)
        assert (extra is None) == (not hinges) and (extra is None or tuple(extra.shape) == (d.G, d.C))
    for t, b in zip((I, sol.disp, sol.V, sol.M, sol.forces, sol.status), before):
        assert _same(t, b)


def test_design_gradient_matches_central_differences_of_the_gpu_forward(lib):
    """Independent of the dense model: L through `frame_solve_cases`, 2 x 3 frame, both hinges, "sum" with weights; step 1e-4 relative
    and bound 2e-5 as in tests/test_gpu_frame_sizing_total.py."""
    import openpystruct_amd as oa
    d = _designs("2x3")
    obj, _ = d.hinged
    weights = (1.0, 1.0, 0.5)
    I = _gpu(d.I)
    factor = oa.frame_factor(d.topo, I)
    sol = oa.frame_resolve(factor, d.loads, d.w)
    grad, extra, _ = oa.frame_design_gradient(factor, sol, d.hp, aggregate="sum", weights=weights, **_kw(obj))
    assert bool((extra > 0).any())

    def L(Iv):
        s = oa.frame_solve_cases(d.topo, Iv.contiguous(), d.loads, d.w)
        P = dr.case_penalties(Iv.cpu()[:, None, :], s.disp.cpu(), s.V.cpu(), s.M.cpu(), d.hp, obj)
        return float((Iv.cpu().sum(-1) + (torch.tensor(weights, dtype=torch.float64) * P).sum(-1)).sum())

    rng = np.random.default_rng(5)
    h = 1e-4
    for _ in range(3):
        v = _gpu(rng.standard_normal(d.I.shape) * d.I)
        quot = (L(I + h * v) - L(I - h * v)) / (2 * h)
        print(f"design gradient vs differences {abs(quot - float((grad * v).sum())) / abs(quot):.3e}")
        assert abs(quot - float((grad * v).sum())) <= 2e-5 * abs(quot)


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
FRAMES = ("2x3", "4x2")
TAGS = ("sum", "weighted", "max")
# at most 5 x the worst deviation of the recorded MI355X run (profiles/frame_designs_deviation.json): loss of the first 20 epochs
# 2.5e-7 (sum), 2.4e-7 (weighted), 3.4e-7 (max); final I over a design's largest inertia 4.2e-7, 3.2e-7, 5.1e-7; stop epochs and
# governing cases equal in all six runs.  None exceeds what the single-case loop recorded (3.5e-7 and 1.7e-6).
TOL_LOSS_20 = {"sum": 1.2e-6, "weighted": 1.2e-6, "max": 1.7e-6}
TOL_I = {"sum": 2.0e-6, "weighted": 1.6e-6, "max": 2.5e-6}


def _generator():
    spec = importlib.util.spec_from_file_location("make_frame_sizing_designs_golden", os.path.join(ROOT, "tests", "golden", "make_frame_sizing_designs_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def run_loop(tag, frame, poll_every):
    """optimize_frame_designs on the fixture's designs with the fixture's configuration -> (fixture, result, losses [epochs, G])."""
    import openpystruct_amd as oa
    mk = _generator()
    z = np.load(GOLDEN)
    cfg, obj, max_epochs, aggregate, weights = mk.runs(frame)[tag]
    p = f"{tag}_{frame}_"
    assert int(z[p + "max_epochs"]) == max_epochs and int(z[p + "aggregate"]) == ("sum", "max").index(aggregate)
    assert np.array_equal(z[p + "objective"], [obj.alpha_sway, obj.sway_limit, obj.alpha_deflection, obj.deflection_limit])
    assert np.array_equal(z[p + "weights"], [] if weights is None else weights)
    hist = []
    r = oa.optimize_frame_designs(_topology(frame), _gpu(z[f"{frame}_loads"]), _gpu(z[f"{frame}_w"]), cfg=cfg, I0=_gpu(z[f"{frame}_I0"], torch.float32),
                                  aggregate=aggregate, weights=weights, max_epochs=max_epochs, poll_every=poll_every, loss_history=hist, **_kw(obj))
    assert int(r.solution.status.abs().sum()) == 0
    return z, r, torch.stack(hist)


def trajectory_deviation(z, tag, frame, r, hist):
    """The HIP loop against the fixture: worst relative deviation of the design loss over the first 20 epochs, per design the
    deviation of the final I over the design's largest inertia, the stop epochs and the governing cases."""
    p = f"{tag}_{frame}_"
    ref20 = z[p + "loss"][:, :20].astype(np.float64)
    dI = np.abs(r.I.cpu().numpy().astype(np.float64) - z[p + "I"]).max(-1) / z[p + "I"].max(-1)
    return {"loss_first20": float((np.abs(hist[:20].T.cpu().numpy().astype(np.float64) - ref20) / np.abs(ref20)).max()),
            "I_rel_to_max": dI.tolist(), "epochs": r.epochs.cpu().numpy().tolist(), "epochs_fixture": z[p + "epochs"].tolist(),
            "governing": r.governing.cpu().numpy().tolist(), "governing_fixture": z[p + "governing"].tolist(),
            "case_penalty_rel": float((np.abs(r.case_penalty.cpu().numpy().astype(np.float64) - z[p + "case_penalty"]) / np.abs(z[p + "case_penalty"])).max())}


def _result_bits(r, hist):
    s = r.solution
    return (r.I, r.epochs, r.governing, r.case_penalty, s.disp, s.V, s.M, s.forces, s.status, hist)


@pytest.mark.parametrize("tag", TAGS)
def test_loop_against_the_cpu_oracle(lib, tag):
    """Both frames of a run with poll_every = 1 and 10 (the same bits: polling only ends the loop), twice in one process."""
    left_out, worst_I = [], 0.0
    for frame in FRAMES:
        z, r, hist = run_loop(tag, frame, 1)
        _, r10, hist10 = run_loop(tag, frame, 10)
        n = min(len(hist), len(hist10))
        for a, b in zip(_result_bits(r, hist[:n]), _result_bits(r10, hist10[:n])):      # a stopped design repeats its last loss
            assert _same(a, b)
        _, r2, hist2 = run_loop(tag, frame, 1)
        for a, b in zip(_result_bits(r, hist), _result_bits(r2, hist2)):
            assert _same(a, b)
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
    print(f"{tag}: left out of the final-I comparison (stop epoch differs): {left_out}; worst I deviation of the others {worst_I:.3e}")
    assert len(left_out) <= 1, left_out


def test_one_case_agrees_with_the_rows_path(lib):
    """C = 1, "sum", no weights against optimize_frames(gradient="total", loads=, element_loads=) on the same rows: other kernels (the
    kept factor's solve, the step's own gradient), so not bit for bit -- within the loop tolerances above."""
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    z = np.load(GOLDEN)
    mk = _generator()
    for tag in ("sum", "weighted"):
        for frame in FRAMES:
            cfg, obj, max_epochs, _, _ = mk.runs(frame)[tag]
            topo = _topology(frame)
            loads, w = _gpu(z[f"{frame}_loads"][:, :1]), _gpu(z[f"{frame}_w"][:, :1])
            I0 = _gpu(z[f"{frame}_I0"], torch.float32)
            G = I0.shape[0]
            h1, hC = [], []
            I_rows, sol_rows, ep_rows = frames.optimize_frames(topo, G, cfg, I0=I0, max_epochs=max_epochs, poll_every=10, loss_history=h1,
                                                               gradient="total", loads=loads[:, 0].contiguous(),
                                                               element_loads=w[:, 0].contiguous(), **_kw(obj))
            r = oa.optimize_frame_designs(topo, loads, w, cfg=cfg, I0=I0, max_epochs=max_epochs, poll_every=10, loss_history=hC, **_kw(obj))
            assert torch.equal(r.epochs, ep_rows) and bool((r.governing == 0).all())
            a, b = torch.stack(hC)[:20].double(), torch.stack(h1)[:20].double()
            d_loss = float(((a - b).abs() / b.abs()).max())
            d_I = float(((r.I.double() - I_rows.double()).abs().max(-1).values / I_rows.double().max(-1).values).max())
            d_V = float((r.solution.V[:, 0] - sol_rows.V).abs().max() / sol_rows.V.abs().max())
            print(f"C = 1 against the rows path, {tag} {frame}: loss {d_loss:.3e} I {d_I:.3e} (last solve's V {d_V:.3e})")
            assert d_loss <= TOL_LOSS_20[tag] and d_I <= TOL_I[tag]


def test_explicit_mode_is_untouched_by_a_designs_run_in_the_same_process(lib):
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    topo = _topology("4x2")
    z = np.load(GOLDEN)

    def explicit():
        hist = []
        I, sol, ep = frames.optimize_frames(topo, 3, max_epochs=30, poll_every=10, loss_history=hist)
        return I, ep, sol.disp, sol.V, sol.M, torch.stack(hist)

    before = explicit()
    r = oa.optimize_frame_designs(topo, _gpu(z["4x2_loads"]), _gpu(z["4x2_w"]), max_epochs=30, poll_every=10, alpha_sway=1.0, sway_limit=1e-4)
    after = explicit()
    for a, b in zip(before, after):
        assert _same(a, b)
    assert not _same(r.I, before[0])


def test_shared_loads_and_the_dataset(lib):
    """Loads shared by the designs ([C,Nn,3], [C,Ne,2]) give the bits of the same loads repeated per design; the dataset generator's
    shapes, and its designs against a direct call on the same draws."""
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    z = np.load(GOLDEN)
    topo = _topology("4x2")
    loads, w = _gpu(z["4x2_loads"][0]), _gpu(z["4x2_w"][0])
    I0 = _gpu(z["4x2_I0"], torch.float32)
    G = I0.shape[0]
    a = oa.optimize_frame_designs(topo, loads, w, I0=I0, max_epochs=12, aggregate="max")
    b = oa.optimize_frame_designs(topo, loads.expand(G, *loads.shape).contiguous(), w.expand(G, *w.shape).contiguous(), I0=I0, max_epochs=12, aggregate="max")
    for s, t in zip(_result_bits(a, a.I), _result_bits(b, b.I)):
        assert _same(s, t)
    c = oa.optimize_frame_designs(topo, loads, n_designs=2, max_epochs=3)          # the topology's own element loads in every case
    assert tuple(c.I.shape) == (2, topo.Ne) and _same(c.I[0], c.I[1]) and int(c.solution.status.abs().sum()) == 0
    G, C = 3, 2
    rec = oa.generate_frame_design_dataset(4, 2, G, C, max_epochs=8, aggregate="max")
    Nn, Ne = topo.Nn, topo.Ne
    shapes = dict(I=(G, Ne), lateral=(G, C), vertical=(G, C), V=(G, C, Ne), M=(G, C, Ne), disp=(G, C, Nn, 3), epochs=(G,), status=(G, C),
                  governing=(G,), case_penalty=(G, C))
    assert {k: tuple(v.shape) for k, v in rec.items()} == shapes and all(not v.is_cuda for v in rec.values())
    assert rec["I"].dtype == torch.float32 and int(rec["status"].abs().sum()) == 0 and rec["epochs"].tolist() == [8] * G
    assert torch.equal(rec["case_penalty"].argmax(dim=1).int(), rec["governing"])
    lat, ver = frames.frame_dataset_draws(G * C)
    assert np.array_equal(rec["lateral"].numpy().reshape(-1), lat) and np.array_equal(rec["vertical"].numpy().reshape(-1), ver)
    ld, wd = frames.grid_load_cases(topo, lat, ver)
    direct = oa.optimize_frame_designs(topo, ld.reshape(G, C, Nn, 3), wd.reshape(G, C, Ne, 2), max_epochs=8, aggregate="max")
    assert _same(direct.I.cpu(), rec["I"]) and _same(direct.solution.V.cpu(), rec["V"])
