"""The exact-gradient ("total") sizing mode on the GPU: ops_beam_sizing_grad_f64 against autograd of the float64
objective through the dense model, ops_beam_sizing_step_grad_f32 against its float64 reference and against the explicit step
it shares the loss with, and optimize_cases(gradient="total") against the project's own CPU oracle of the loop
(tests/golden/sizing_total_reference.npz, tests/golden/make_sizing_total_golden.py).

Trajectory tolerances: at most 5 x the deviations one MI355X run recorded (profiles/sizing_total_deviation.json), the practice of
tests/test_sizing_golden.py; stop epochs may differ by at most `patience`."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import sizing_step_cases as sc  # noqa: E402
from tests import sizing_total_ref as tr  # noqa: E402
from tests.beam_dense import cond_free, random_case  # noqa: E402
from tests.test_gpu_sizing_step import SENT_F64, SENT_I32, State, _same_bits, check_epoch, check_second_call  # noqa: E402
from tests.test_sizing_grad_emulation import grad_error, median_limit  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
HPS = {"beam": sc.beam_hp, "frame": sc.frame_hp}
ERR_INVALID_ARG = None      # read from the header by the fixture


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi
    global ERR_INVALID_ARG
    ERR_INVALID_ARG = _cabi.ERR_INVALID_ARG
    return _cabi.load()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# the gradient kernel
# ---------------------------------------------------------------------------------------------------------------------
# every tiling (16x7 up to Ne = 111, 32x4 to 127, 64x4 to 255, 64x8 to 511, 64x16 beyond) and both sides of each boundary
GRAD_NE = [1, 2, 5, 13, 100, 111, 112, 127, 128, 255, 256, 511, 512, 1023]
GRAD_B = [1, 3, 9]       # one beam; a ragged wave at four beams per wave; with cases 4..7 inactive, a whole wave of finished cases
B_REF = max(GRAD_B)
ALPHA_D = 100.0


@functools.lru_cache(maxsize=None)
def _grad_reference(Ne):
    """Inputs and float64 references (no deflection term / with it) of the B_REF-beam batch of this Ne, computed once: smaller
    batches are its first beams.  Per-beam x / fix and per-element E / wy for every other Ne of the list."""
    per_beam = GRAD_NE.index(Ne) % 2 == 1
    rng = np.random.default_rng([Ne, 20250307])
    x, fix, I, Fy = random_case(rng, B_REF, Ne, per_beam=per_beam)
    E = rng.uniform(1.5e11, 2.5e11, size=(B_REF, Ne)) if per_beam else np.float64(2e11)
    wy = rng.uniform(-2e3, 0, size=(B_REF, Ne)) if per_beam else np.float64(-750.0)
    hp = sc.beam_hp()
    fwd = tr.dense_forward(x, E, I, fix, Fy, wy)
    free = tr.objective_gradient(fwd, hp, tr.objective(), retain_graph=True)
    obj = tr.objective(ALPHA_D, median_limit(free.outs[0], fix))
    defl = tr.objective_gradient(fwd, hp, obj)
    kappa = cond_free(x[0] if per_beam else x, E[0] if per_beam else E, I[0], fix[0] if per_beam else fix)   # as the emulation test
    return types.SimpleNamespace(per_beam=per_beam, x=x, fix=fix, I=I, Fy=Fy, E=E, wy=wy, hp=hp, obj=obj, free=free, defl=defl,
                                 kappa=kappa, tol=max(1e-8, 4e-16 * kappa))


def _first(a, B, per_beam):
    return a[:B] if per_beam else a


def _call_grad(lib, c, B, obj, *, I=None, active=None, with_extra=True, override=None):
    """beam_solve on the GPU, then ops_beam_sizing_grad_f64 on its outputs, into sentinel-filled buffers.  `override`: replaces
    named arguments of the C call (the refusal tests).  Returns rc and the host copies of grad, loss_extra, status, v."""
    import openpystruct_amd as oa
    from openpystruct_amd import _cabi
    Ne = c.I.shape[1]
    N = Ne + 1
    pb = c.per_beam
    x, fix = _dev(_first(c.x, B, pb)), _dev(_first(c.fix, B, pb), torch.uint8)
    E, wy = _dev(_first(c.E, B, pb)), _dev(_first(c.wy, B, pb))
    Id, Fy = _dev(c.I[:B] if I is None else I), _dev(c.Fy[:B])
    sol = oa.beam_solve(x, E, Id, fix, Fy, wy)
    grad = torch.full((B, Ne), float(SENT_F64), dtype=torch.float64, device=DEV)
    extra = torch.full((B,), float(SENT_F64), dtype=torch.float64, device=DEV)
    status = torch.full((B,), int(SENT_I32), dtype=torch.int32, device=DEV)
    act = None if active is None else _dev(active, torch.uint8)
    cobj = _cabi.SizingObjective(alpha_deflection=obj.alpha_deflection, deflection_limit=obj.deflection_limit)
    a = dict(B=B, Ne=Ne, x=x.data_ptr(), x_bs=N if pb else 0, E=E.data_ptr(), E_bs=Ne if pb else 0, I=Id.data_ptr(), I_bs=Ne,
             fix=fix.data_ptr(), fix_bs=N if pb else 0, wy=wy.data_ptr(), wy_bs=Ne if pb else 0, v=sol.v.data_ptr(),
             theta=sol.theta.data_ptr(), V=sol.V.data_ptr(), M=sol.M.data_ptr(), hp=ctypes.byref(c.hp), obj=ctypes.byref(cobj),
             active=None if act is None else act.data_ptr(), grad=grad.data_ptr(), extra=extra.data_ptr() if with_extra else None,
             status=status.data_ptr(), stream=_stream())
    a.update(override or {})
    rc = lib.ops_beam_sizing_grad_f64(*a.values())
    torch.cuda.synchronize()
    return rc, grad.cpu().numpy(), extra.cpu().numpy(), status.cpu().numpy(), sol.v.cpu().numpy(), sol.status.cpu().numpy()


def _defl_term(v, obj):
    ex = np.maximum(np.abs(v) - obj.deflection_limit, 0.0) / obj.deflection_limit
    return obj.alpha_deflection * (ex ** 2).sum(-1)


@pytest.mark.parametrize("deflection", [False, True])
@pytest.mark.parametrize("B", GRAD_B)
@pytest.mark.parametrize("Ne", GRAD_NE)
def test_gradient_kernel_matches_autograd_of_the_objective(lib, Ne, B, deflection):
    """The gradient to the emulation test's bound.  loss_extra: the kernel's input is the GPU forward's v, not the dense model's,
    so the 1e-12 of the emulation test is asked of the term evaluated on that v (measured on the MI355X: 3.7e-16 at worst), and
    the dense reference's value is matched within what the forward's rounding of v moves it by (measured deviations from it:
    1e-14 at Ne = 2, 3e-8 at Ne = 100, 4e-5 at Ne = 512, 4e-4 at Ne = 1023, where cond(K) is 3e13)."""
    c = _grad_reference(Ne)
    r = c.defl if deflection else c.free
    obj = c.obj if deflection else tr.objective()
    active = None
    if B == 9:
        active = np.ones(B, dtype=np.uint8)
        active[4:8] = 0
    rc, grad, extra, status, v, st_fwd = _call_grad(lib, c, B, obj, active=active, with_extra=deflection)
    assert rc == 0 and (st_fwd == 0).all()
    on = np.ones(B, dtype=bool) if active is None else active != 0
    assert (status[on] == 0).all()
    rb = types.SimpleNamespace(grad=r.grad[:B][on], outs=tuple(o[:B][on] for o in r.outs), cot=tuple(None if g is None else g[:B][on] for g in r.cot))
    pb = c.per_beam
    err = grad_error(grad[on], rb, c.x[:B][on] if pb else c.x, c.I[:B][on], c.wy[:B][on] if pb else c.wy)
    print(f"Ne {Ne} B {B} deflection {deflection}: gradient error {err:.3e} (bound {c.tol:.3e})")
    assert err < c.tol, (err, c.tol)
    if deflection:
        # the term is a function of the kernel's own input v: held to the float64 evaluation of that v, and (through the dense
        # model's v, which differs by the forward's rounding) to the reference
        want = _defl_term(v[on], obj)
        assert (np.abs(extra[on] - want) <= 1e-12 * want).all(), (extra[on], want)
        # against the reference: its v and the GPU forward's differ by the forward's rounding, pinned by tests/test_gpu_beam_grad.py
        # to max(1e-10, 4e-16 cond) of |v|; the term moves by at most |gv| . |dv| with it
        fwd = max(1e-10, 4e-16 * c.kappa)
        slack = fwd * np.linalg.norm(r.cot[0][:B][on], axis=-1) * np.linalg.norm(r.outs[0][:B][on], axis=-1)
        pos = r.loss_extra[:B][on] > 0
        if pos.any():
            print(f"Ne {Ne} B {B}: loss_extra against the dense reference, worst relative deviation "
                  f"{float((np.abs(extra[on] - r.loss_extra[:B][on])[pos] / r.loss_extra[:B][on][pos]).max()):.3e}; against the term of the "
                  f"kernel's own v {float((np.abs(extra[on] - want)[pos] / want[pos]).max()):.3e}")
        assert (np.abs(extra[on] - r.loss_extra[:B][on]) <= 1e-12 * r.loss_extra[:B][on] + slack).all(), (extra[on], r.loss_extra[:B][on])
        assert (r.loss_extra > 0).any() or Ne == 1
    else:
        assert _same_bits(extra, SENT_F64)
    # rows of inactive cases keep the sentinel, bit for bit
    assert _same_bits(grad[~on], SENT_F64) and _same_bits(status[~on], SENT_I32)
    if deflection:
        assert _same_bits(extra[~on], SENT_F64)


@pytest.mark.parametrize("Ne", [100, 128])
def test_a_failed_beam_is_nan_and_leaves_its_wave_neighbours_alone(lib, Ne):
    """One beam's inertias made non-positive: status != 0 and NaN in its row and its loss_extra; every other beam -- the ones
    sharing its wavefront included -- bit-equal to the same call without the defect."""
    c = _grad_reference(Ne)
    B, bad_row = 9, 2
    rc, g0, e0, s0, _, _ = _call_grad(lib, c, B, c.obj)
    I = c.I[:B].copy()
    I[bad_row] = -I[bad_row]
    rc1, g1, e1, s1, _, _ = _call_grad(lib, c, B, c.obj, I=I)
    assert rc == 0 and rc1 == 0 and (s0 == 0).all()
    assert s1[bad_row] != 0 and np.isnan(g1[bad_row]).all() and np.isnan(e1[bad_row])
    others = np.arange(B) != bad_row
    assert (s1[others] == 0).all()
    assert _same_bits(g1[others], g0[others]) and _same_bits(e1[others], e0[others])


def test_gradient_kernel_refuses_bad_arguments_and_writes_nothing(lib):
    c = _grad_reference(13)
    B, Ne = 3, 13
    ok = _call_grad(lib, c, B, c.obj)
    assert ok[0] == 0
    refusals = [{k: None} for k in ("x", "E", "I", "fix", "wy", "v", "theta", "V", "M", "hp", "obj", "grad", "extra")]
    refusals += [{"I_bs": Ne - 1}, {"x_bs": Ne}, {"fix_bs": 1}, {"E_bs": Ne - 1}, {"wy_bs": -1}, {"B": -1}, {"Ne": 0}]
    for override in refusals:
        rc, grad, extra, status, _, _ = _call_grad(lib, c, B, c.obj, override=override)
        assert rc == ERR_INVALID_ARG, (override, rc)
        assert _same_bits(grad, SENT_F64) and _same_bits(extra, SENT_F64) and _same_bits(status, SENT_I32), override
    for bad in (tr.objective(ALPHA_D, 0.0), tr.objective(ALPHA_D, -0.01), tr.objective(-1.0, 0.01)):
        rc, grad, extra, status, _, _ = _call_grad(lib, c, B, bad)
        assert rc == ERR_INVALID_ARG, (bad, rc)
        assert _same_bits(grad, SENT_F64) and _same_bits(extra, SENT_F64) and _same_bits(status, SENT_I32)
    # loss_extra == NULL is fine without the term; B == 0 is fine and writes nothing
    assert _call_grad(lib, c, B, tr.objective(), with_extra=False)[0] == 0
    rc, grad, extra, status, _, _ = _call_grad(lib, c, B, c.obj, override={"B": 0})
    assert rc == 0 and _same_bits(grad, SENT_F64)


def test_public_wrapper_matches_the_c_entry(lib):
    import openpystruct_amd as oa
    c = _grad_reference(100)
    B = 3
    _, grad, extra, _, _, _ = _call_grad(lib, c, B, c.obj)
    x, fix, E, wy = _dev(c.x), _dev(c.fix, torch.uint8), _dev(c.E), _dev(c.wy)
    sol = oa.beam_solve(x, E, _dev(c.I[:B]), fix, _dev(c.Fy[:B]), wy)
    g, e, s = oa.beam_sizing_gradient(x, E, _dev(c.I[:B]), fix, wy, sol, c.hp, ALPHA_D, c.obj.deflection_limit)
    assert _same_bits(g.cpu().numpy(), grad) and _same_bits(e.cpu().numpy(), extra) and int(s.abs().sum()) == 0
    g0, e0, _ = oa.beam_sizing_gradient(x, E, _dev(c.I[:B]), fix, wy, sol, c.hp)
    assert e0 is None and np.isfinite(g0.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------
# the gradient-fed step
# ---------------------------------------------------------------------------------------------------------------------
STEP_NE = [1, 2, 5, 100, 512]
STEP_B = [1, 5, 9]


def _grad_epoch(I, m, v, V, M, grad, extra, hp, shift, group=4):
    """sc.reference_epoch for the gradient-fed step: states placed from the reference's loss, then the reference of the epoch."""
    B = I.shape[0]
    z = np.zeros(B, dtype=np.int64)
    loss = tr.step_grad_reference(I, m, v, V, M, grad, extra, z, np.full(B, np.inf), z, hp)["loss"]
    st = sc.case_states(loss, hp, shift, group)
    ref = tr.step_grad_reference(I, m, v, V, M, grad, extra, st.t, st.best, st.cnt, hp)
    assert (np.abs(st.best.astype(np.float64) - hp.tolerance - ref["loss"]) >= 1e-3 * np.abs(ref["loss"] + hp.tolerance))[st.kind != "e"].all()
    want_stop = (st.kind == "c") | (st.kind == "d")
    assert (ref["stop"][st.kind != "e"] == want_stop[st.kind != "e"]).all()
    return st, ref


def _run_step_grad(lib, V, M, grad, extra, I, m, v, st, hp, *, vm32=True, schedule=None, explicit=False):
    s = State(I, m, v, st)
    B, Ne = I.shape
    dV, dM, dg = _dev(V), _dev(M), _dev(grad)
    de = None if extra is None else _dev(extra)
    sched = None if schedule is None else _dev(schedule)
    if explicit:
        call = lambda: lib.ops_beam_sizing_step_f32(   # noqa: E731
            B, Ne, *s.ptrs("I", "I64"), dV.data_ptr(), dM.data_ptr(),
            *s.ptrs("exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss"),
            *s.ptrs("V32", "M32"), ctypes.byref(hp), _stream())
    else:
        call = lambda: lib.ops_beam_sizing_step_grad_f32(   # noqa: E731
            B, Ne, *s.ptrs("I", "I64"), dV.data_ptr(), dM.data_ptr(), dg.data_ptr(), None if de is None else de.data_ptr(),
            *s.ptrs("exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss"),
            *(s.ptrs("V32", "M32") if vm32 else (None, None)), ctypes.byref(hp), None if sched is None else sched.data_ptr(), _stream())
    pre = s.snapshot()
    assert call() == 0
    post = s.snapshot()
    assert call() == 0
    return pre, post, s.snapshot()


def _step_inputs(B, Ne, shift):
    rng = np.random.default_rng([B, Ne, shift, 5])
    I, m, v = sc.optimiser_state(rng, B, Ne)
    V, M = sc.random_forces(rng, B, Ne)
    grad = rng.standard_normal((B, Ne)) * np.exp(rng.uniform(np.log(1e-2), np.log(1e2), size=(B, Ne)))
    extra = rng.uniform(0.0, 50.0, size=B)
    return I, m, v, V, M, grad, extra


@pytest.mark.parametrize("hp_name", list(HPS))
@pytest.mark.parametrize("B", STEP_B)
@pytest.mark.parametrize("Ne", STEP_NE)
def test_step_grad(lib, B, Ne, hp_name):
    hp = HPS[hp_name]()
    entry = "ops_beam_sizing_step_grad_f32"
    table = np.zeros((hp.max_epochs, 2), dtype=np.float32)
    lib.ops_sizing_schedule_f32(ctypes.byref(hp), table.ctypes.data)
    for shift in range(5):
        I, m, v, V, M, grad, extra = _step_inputs(B, Ne, shift)
        # with the deflection term's value, with the schedule table and with pow() in the kernel
        st, ref = _grad_epoch(I, m, v, V, M, grad, extra, hp, shift)
        for schedule in (table, None):
            pre, post, post2 = _run_step_grad(lib, V, M, grad, extra, I, m, v, st, hp, schedule=schedule)
            check_epoch(entry, pre, post, st, ref, hp, sc.STEP_BOUND, wrote=("I64", "V32", "M32"))
            check_second_call(entry, post, post2, st, ref)
        act = st.active == 1
        assert _same_bits(post["V32"][act], V.astype(np.float32)[act]) and _same_bits(post["M32"][act], M.astype(np.float32)[act])
        # V32 == M32 == NULL: the same state, bit for bit
        pre_n, post_n, _ = _run_step_grad(lib, V, M, grad, extra, I, m, v, st, hp, vm32=False)
        check_epoch(entry, pre_n, post_n, st, ref, hp, sc.STEP_BOUND, wrote=("I64",))
        for k in State.NAMES:
            if k not in ("V32", "M32"):
                assert _same_bits(post_n[k], post[k]), k
        # loss_extra == NULL: the loss expression is the explicit step's -- everything that follows from it is bit-equal to
        # what ops_beam_sizing_step_f32 writes from the same inputs
        st0, ref0 = _grad_epoch(I, m, v, V, M, grad, None, hp, shift)
        pre0, post0, _ = _run_step_grad(lib, V, M, grad, None, I, m, v, st0, hp)
        check_epoch(entry, pre0, post0, st0, ref0, hp, sc.STEP_BOUND, wrote=("I64", "V32", "M32"))
        _, post_x, _ = _run_step_grad(lib, V, M, grad, None, I, m, v, st0, hp, explicit=True)
        for k in ("last_loss", "best_loss", "patience_cnt", "epochs_run", "active", "V32", "M32"):
            assert _same_bits(post0[k], post_x[k]), k


def test_step_grad_refuses_bad_arguments(lib):
    hp = sc.beam_hp()
    I, m, v, V, M, grad, extra = _step_inputs(3, 5, 0)
    st, _ = _grad_epoch(I, m, v, V, M, grad, extra, hp, 0)
    s = State(I, m, v, st)
    dV, dM, dg = _dev(V), _dev(M), _dev(grad)
    args = [3, 5, *s.ptrs("I", "I64"), dV.data_ptr(), dM.data_ptr(), dg.data_ptr(), None,
            *s.ptrs("exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss", "V32", "M32"),
            ctypes.byref(hp), None, _stream()]
    pre = s.snapshot()
    from openpystruct_amd import _cabi
    for k in (2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 17):     # each required pointer; V32 without M32
        bad = list(args)
        bad[k] = None
        assert lib.ops_beam_sizing_step_grad_f32(*bad) == _cabi.ERR_INVALID_ARG, k
    bad = list(args)
    bad[1] = 513
    assert lib.ops_beam_sizing_step_grad_f32(*bad) == _cabi.ERR_UNSUPPORTED
    post = s.snapshot()
    for k in State.NAMES:
        assert _same_bits(post[k], pre[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden", "sizing_total_reference.npz")
# at most 5 x the worst deviation of the recorded MI355X run (profiles/sizing_total_deviation.json): loss of the first 20 epochs
# 1.9e-7 in both runs, final I over a case's largest inertia 4.5e-7 (free) and 3.1e-7 (defl); stop epochs equal in all 8 runs
TOL_LOSS_20 = {"free": 9e-7, "defl": 9e-7}
TOL_I = {"free": 2.2e-6, "defl": 1.5e-6}


def _fixture_cases():
    from openpystruct_amd import sizing
    z = np.load(GOLDEN)
    cfg = sizing.SizingConfig()
    cases = sizing.make_cases(int(z["n_cases"]), cfg, seed=int(z["seed"]), device="cpu")
    assert np.array_equal(cases.Fy.numpy(), z["Fy"]) and np.array_equal(cases.fix.numpy(), z["fix"]), "another case draw than the fixture's"
    return z, cfg, cases


def _objective_kwargs(z, tag):
    alpha, limit = (float(t) for t in z[f"{tag}_objective"])
    return dict(gradient="total", alpha_deflection=alpha, deflection_limit=limit if alpha > 0 else None)


def _snapshot(st):
    torch.cuda.synchronize()
    return {k: getattr(st, k).cpu().numpy().copy() for k in ("I", "epochs_run", "V32", "M32", "last_loss")} | \
        {"v": st.sol.v.cpu().numpy().copy(), "theta": st.sol.theta.cpu().numpy().copy(), "status": st.sol.status.cpu().numpy().copy()}


def trajectory_deviation(z, tag, snap, hist):
    """The HIP loop against the fixture: worst relative deviation of the loss over the first 20 epochs, worst deviation of the
    final I over a case's largest inertia (cases whose stop epochs coincide), the stop epochs."""
    ep, ref_ep = snap["epochs_run"], z[f"{tag}_epochs"]
    ref20 = z[f"{tag}_loss"][:, :20].astype(np.float64)
    same = ep == ref_ep
    dI = np.abs(snap["I"].astype(np.float64) - z[f"{tag}_I"]).max(-1) / z[f"{tag}_I"].max(-1)
    return {"loss_first20": float((np.abs(hist[:20].T.astype(np.float64) - ref20) / np.abs(ref20)).max()),
            "I_rel_to_max": float(dI[same].max()) if same.any() else None,
            "epochs": ep.tolist(), "epochs_fixture": ref_ep.tolist(),
            "max_abs_v": np.abs(snap["v"]).max(-1).tolist(), "max_abs_v_fixture": z[f"{tag}_vmax"].tolist()}


def run_total(tag, **kw):
    """optimize_cases(gradient="total") on the fixture's cases with this objective -> (fixture, cfg, snapshot, state)."""
    from openpystruct_amd import sizing
    z, cfg, cases = _fixture_cases()
    st = sizing.optimize_cases(cases, cfg, DEV, **_objective_kwargs(z, tag), **kw)
    return z, cfg, _snapshot(st), st


@pytest.mark.parametrize("tag", ["free", "defl"])
def test_total_loop_against_the_cpu_oracle(lib, tag):
    from openpystruct_amd import sizing
    z, cfg, eager, st = run_total(tag, record_loss=True)
    hist = st.loss_history.cpu().numpy()
    assert (eager["status"] == 0).all() and int(st.active.sum()) == 0
    dev = trajectory_deviation(z, tag, eager, hist)
    print(tag, dev)
    assert (np.abs(eager["epochs_run"] - z[f"{tag}_epochs"]) <= cfg.patience).all(), dev
    assert dev["loss_first20"] <= TOL_LOSS_20[tag], dev
    assert dev["I_rel_to_max"] is not None and dev["I_rel_to_max"] <= TOL_I[tag], dev
    limit = 0.01
    vmax = np.abs(eager["v"]).max(-1)
    if tag == "defl":
        assert float(z["defl_objective"][1]) == limit
        assert (vmax <= 1.10 * limit).all(), vmax        # the limit is met ...
    else:
        assert (vmax > 1.5 * limit).sum() >= 2, vmax     # ... and binding: the unconstrained designs of the same cases exceed it
    # the captured graph and reuse=True across two shards: the same bits
    _, _, graph, _ = run_total(tag)
    _, _, cases = _fixture_cases()
    kw = _objective_kwargs(z, tag)
    halves = [_snapshot(sizing.optimize_cases(cases.slice(lo, lo + 2), cfg, DEV, reuse=True, **kw)) for lo in (0, 2)]
    for k, a in eager.items():
        assert _same_bits(graph[k], a), ("graph", k)
        assert _same_bits(np.concatenate([h[k] for h in halves]), a), ("reuse", k)


def test_explicit_mode_is_untouched_by_a_total_run_in_the_same_process(lib):
    from openpystruct_amd import sizing
    z, cfg, cases = _fixture_cases()
    before = _snapshot(sizing.optimize_cases(cases, cfg, DEV, reuse=True))
    total = _snapshot(sizing.optimize_cases(cases, cfg, DEV, reuse=True, **_objective_kwargs(z, "defl")))
    cached = list(sizing._EPOCH_GRAPHS.values())[-1][0]
    assert cached.objective == ("total", 100.0, 0.01)          # the explicit state and its graph were dropped, not re-armed
    after = _snapshot(sizing.optimize_cases(cases, cfg, DEV, reuse=True))
    assert list(sizing._EPOCH_GRAPHS.values())[-1][0].objective == ("explicit", 0.0, 0.0)
    for k, a in before.items():
        assert _same_bits(after[k], a), k
    assert not np.array_equal(total["I"], before["I"])
    with pytest.raises(ValueError):
        sizing.optimize_cases(cases, cfg, DEV, gradient="explicit", alpha_deflection=100.0, deflection_limit=0.01)
    with pytest.raises(ValueError):
        sizing.optimize_cases(cases, cfg, DEV, gradient="total", alpha_deflection=100.0)


def test_reuse_rearms_the_two_launch_epoch_like_a_fresh_state(lib, monkeypatch):
    """The separate path (solve, then step: OPS_AMD_SIZING_FUSED=0) under reuse=True: the second shard runs on the first one's
    re-armed state and captured graph, and the two shards carry the bits of one fresh run of all four cases."""
    from openpystruct_amd import sizing
    monkeypatch.setattr(sizing, "_FUSED_EPOCH", False)
    monkeypatch.setattr(sizing, "_EPOCH_GRAPHS", {})           # (this test's state is not left behind for a later one to re-arm)
    cfg = sizing.SizingConfig(num_nodes=41, roller_nodes=(10, 30), max_e=6)
    cases = sizing.make_cases(4, cfg, seed=41)
    fresh = _snapshot(sizing.optimize_cases(cases, cfg, DEV, poll_every=2))
    assert (fresh["status"] == 0).all() and (fresh["epochs_run"] == 6).all()
    states, halves = [], []
    for lo in (0, 2):
        states.append(sizing.optimize_cases(cases.slice(lo, lo + 2), cfg, DEV, poll_every=2, reuse=True))
        halves.append(_snapshot(states[-1]))
    assert states[1] is states[0] and not states[0]._fused and states[0].objective == ("explicit", 0.0, 0.0)
    for k, a in fresh.items():
        assert _same_bits(np.concatenate([h[k] for h in halves]), a), k


def test_generate_dataset_in_total_mode_returns_the_record_schema(lib):
    from openpystruct_amd import sizing
    rec = sizing.generate_dataset(8, device=DEV, gradient="total")
    assert set(sizing.RECORD_KEYS) <= set(rec)
    assert rec["I_values"].shape == (8, 100) and rec["I_values"].dtype == torch.float32
    assert rec["deflections"].shape == (8, 101) and int(rec["status"].abs().sum()) == 0
    con = sizing.generate_dataset(8, device=DEV, gradient="total", alpha_deflection=100.0, deflection_limit=0.01)
    assert set(sizing.RECORD_KEYS) <= set(con) and int(con["status"].abs().sum()) == 0
    assert float(con["deflections"].abs().max()) <= float(rec["deflections"].abs().max())
