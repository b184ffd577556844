"""Gradients through the batched frame solve on the GPU: the two streaming kernels of csrc/frame_vjp.hip around a second
(adjoint) call of the solve, `frames.frame_solve_vjp`, the operators `openpystruct_amd::frame_solve` / `frame_solve_vjp` and
their autograd formula (torch_op.py), checked against autograd of a dense float64 model (tests/frame_dense.py), against central
differences of the GPU forward, and for the exact gradient of the reference's frame loss.

Bit-for-bit comparisons use the 4 x 2 frame (18 elements): the assembly of the solve adds element contributions with LDS atomics
in the order of the plan's entries, and a plan of more than 64 elements is filled by several wavefronts in an order that may
differ from one build of the plan to the next (tests/test_gpu_frames.py, the two-streams test)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import frame_dense as fd  # noqa: E402
from tests.helpers import relerr  # noqa: E402


@pytest.fixture(autouse=True)
def _tuned_kernels_for_every_batch():
    """As tests/test_gpu_frames.py: library option frame_latency_batch = 0 (the tuned kernels for every batch) unless a test takes
    `dispatch`; options are process-wide and put back after each test."""
    from openpystruct_amd import _cabi
    _cabi.set_option("frame_latency_batch", 0)
    yield
    _cabi.set_option("frame_latency_batch", -1)
    _cabi.set_option("frame_pack", 1)
    _cabi.set_option("frame_coop", 1)


@pytest.fixture(params=["tuned", "default"])
def dispatch(request):
    if request.param == "default":
        from openpystruct_amd import _cabi
        _cabi.set_option("frame_latency_batch", -1)      # the library's own dispatch: small batches take a workgroup per frame
    return request.param


@pytest.fixture(scope="module")
def oa():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    import openpystruct_amd
    from openpystruct_amd import torch_op  # noqa: F401
    return openpystruct_amd


def _gpu(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _nrel(a, b, scale=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), scale, 1e-300))


def _topology(name):
    from openpystruct_amd import frames
    if name == "general":
        return fd.custom_frame(2, 2, True, True, "cuda")       # one pinned support line, one brace per story
    if name == "hub":
        return fd.hub_frame("cuda")
    bays, stories = (int(v) for v in name.split("x"))
    return frames.grid_frame(bays, stories)


def _cotangents(rng, B, Nn, Ne):
    """Sizes that let every cotangent matter: displacements are ~1e-3, forces ~1e4."""
    return [rng.standard_normal((B, Nn, 3)) * 1e6, rng.standard_normal((B, Ne, 6)), rng.standard_normal((B, Ne)),
            rng.standard_normal((B, Ne))]


@functools.lru_cache(maxsize=None)
def _reference(name, B, shared_loads=False):
    """One case and its dense-model answers (CPU, float64), computed once and shared by the tests and dispatches that use it."""
    topo = _topology(name)
    case = fd.case_of(topo)
    rng = np.random.default_rng(sum(map(ord, name)) + B)
    I = fd.random_inertias(rng, B, topo.Ne)
    if shared_loads:
        loads = topo.nodal_loads * 1.5 + rng.standard_normal((topo.Nn, 3)) * 1e3
    else:
        loads = np.broadcast_to(topo.nodal_loads, (B, topo.Nn, 3)) * rng.uniform(0.5, 2.0, size=(B, 1, 1)) + rng.standard_normal((B, topo.Nn, 3)) * 1e3
    cot = _cotangents(rng, B, topo.Nn, topo.Ne)
    It = torch.tensor(I, requires_grad=True)
    Lt = torch.tensor(np.broadcast_to(loads, (B, topo.Nn, 3)).copy(), requires_grad=True)      # per frame: its gradient is lambda
    outs = fd.dense_frame_solve(case, It, Lt)
    loss = sum((o * torch.tensor(c)).sum() for o, c in zip(outs, cot))
    gI, lam = (g.numpy() for g in torch.autograd.grad(loss, [It, Lt]))
    gL = lam.sum(0) if shared_loads else lam               # one load set for the batch takes the sum over the frames
    outs = [o.detach().numpy() for o in outs]
    kappa = max(fd.cond_free(case, I[b]) for b in range(min(B, 3)))
    sI = fd.gI_term_scale(case, outs[0], lam, fd.fold(B, topo.Ne, *cot[1:]))
    for a in (I, loads, gI, gL, *cot, *outs):
        a.setflags(write=False)
    return dict(topo=topo, I=I, loads=loads, cot=cot, outs=outs, gI=gI, gL=gL, kappa=kappa, sI=sI)


def _op_grads(oa, r):
    I, loads = _gpu(r["I"]).requires_grad_(True), _gpu(r["loads"]).requires_grad_(True)
    s = oa.differentiable_frame_solve(r["topo"], I, loads)
    assert int(s.status.abs().sum()) == 0
    L = sum((o * _gpu(c)).sum() for o, c in zip(s[:4], r["cot"]))
    gI, gL = torch.autograd.grad(L, [I, loads])
    return s, gI, gL


def _check_against_dense(oa, r):
    s, gI, gL = _op_grads(oa, r)
    B = r["I"].shape[0]
    # the test's model is the forward: pinned first, at the tolerances of tests/test_gpu_frames.py
    assert relerr(s.disp.detach().cpu().numpy().reshape(B, -1), r["outs"][0].reshape(B, -1)) < 1e-8
    assert relerr(s.forces.detach().cpu().numpy().reshape(B, -1), r["outs"][1].reshape(B, -1)) < 1e-7
    assert torch.equal(s.V, s.forces[..., 1]) and torch.equal(s.M, s.forces[..., 2])
    tol = max(1e-8, 4e-16 * r["kappa"])
    eI, eL = _nrel(gI.cpu().numpy(), r["gI"], r["sI"]), _nrel(gL.cpu().numpy(), r["gL"])
    print(f"gI {eI:.3e} g_loads {eL:.3e} tol {tol:.3e} kappa {r['kappa']:.3e}")
    assert gI.shape == r["gI"].shape and gL.shape == r["gL"].shape
    assert eI < tol and eL < tol


@pytest.mark.parametrize("name,B", [("1x1", 1), ("2x3", 5), ("4x2", 5), ("7x5", 5), ("10x10", 3), ("general", 5), ("hub", 5)])
def test_vjp_matches_dense_autograd(oa, dispatch, name, B):
    _check_against_dense(oa, _reference(name, B))


@pytest.mark.parametrize("latency_batch", [-1, 256])
def test_vjp_matches_dense_autograd_beyond_one_frame_per_cu(oa, latency_batch):
    """300 frames of 4 x 2.  -1, the library's default dispatch: more than one frame per CU (256, the least the latency threshold
    is); the model puts this small frame's threshold higher, so it is the workgroup-per-frame kernels in a second round.  256: the
    threshold held at its least, so the same batch is beyond it and takes the packed kernel."""
    from openpystruct_amd import _cabi
    _cabi.set_option("frame_latency_batch", latency_batch)
    r = _reference("4x2", 300)
    assert (int(_cabi.load().ops_frame_plan_signature(300, r["topo"].n_eq, r["topo"].kd)) != 0) == (latency_batch == 256)
    _check_against_dense(oa, r)


@pytest.mark.parametrize("shared", [False, True])
def test_load_gradient_has_the_shape_of_the_loads(oa, dispatch, shared):
    """Loads [B,Nn,3]: lambda per frame; loads [Nn,3] shared by the batch: its sum over the frames."""
    r = _reference("2x3", 5, shared)
    assert r["gL"].shape == ((r["topo"].Nn, 3) if shared else (5, r["topo"].Nn, 3))
    _check_against_dense(oa, r)


def test_vjp_matches_central_differences_of_the_forward(oa):
    """Independent of the dense model: directional derivatives in I and in the loads (relative directions) from the VJP against
    central differences of the GPU forward, 2 x 3 frame, B = 8.  Step 1e-4 and bound 2e-5 as in the beam test: the frames'
    cond(K_ff) is ~1e3, so the forward's rounding error over the step is ~1e-9 and the truncation error ~1e-8 (the same
    quotient of the CPU oracle deviates from dense autograd by at most 4e-7 in I and 4e-10 in the loads)."""
    from openpystruct_amd import frames
    r = _reference("2x3", 8)
    topo, I, loads = r["topo"], r["I"], r["loads"]
    cot = [_gpu(c) for c in r["cot"]]

    def loss(I_, l_):
        s = frames.frame_solve(topo, _gpu(I_), _gpu(l_))
        return float(sum((o * c).sum() for o, c in zip(s[:4], cot)))

    _, gI, gL = _op_grads(oa, r)
    gI, gL = gI.cpu().numpy(), gL.cpu().numpy()
    rng = np.random.default_rng(5)
    h = 1e-4
    for _ in range(3):
        dI = rng.standard_normal(I.shape) * I
        dl = rng.standard_normal(loads.shape) * loads
        fd_I = (loss(I + h * dI, loads) - loss(I - h * dI, loads)) / (2 * h)
        fd_l = (loss(I, loads + h * dl) - loss(I, loads - h * dl)) / (2 * h)
        print(f"I {abs(fd_I - (gI * dI).sum()) / abs(fd_I):.3e} loads {abs(fd_l - (gL * dl).sum()) / abs(fd_l):.3e}")
        assert abs(fd_I - (gI * dI).sum()) <= 2e-5 * abs(fd_I), (fd_I, (gI * dI).sum())
        assert abs(fd_l - (gL * dl).sum()) <= 2e-5 * abs(fd_l), (fd_l, (gL * dl).sum())


def test_null_cotangents_equal_zeros(oa):
    """Every NULL cotangent is a zero one, bit for bit, in all 16 combinations."""
    from openpystruct_amd import frames
    r = _reference("4x2", 5)
    topo, I = r["topo"], _gpu(r["I"])
    s = frames.frame_solve(topo, I, _gpu(r["loads"]))
    cot = [_gpu(c) for c in r["cot"]]
    for mask in range(16):
        c_null = [c if not (mask >> k) & 1 else None for k, c in enumerate(cot)]
        c_zero = [c if not (mask >> k) & 1 else torch.zeros_like(c) for k, c in enumerate(cot)]
        p = oa.frame_solve_vjp(topo, I, s.disp, *c_null)
        q = oa.frame_solve_vjp(topo, I, s.disp, *c_zero)
        for u, w in zip(p, q):
            assert torch.equal(u, w), mask
    gI, lam, st = oa.frame_solve_vjp(topo, I, s.disp)          # no cotangent at all: no gradient
    assert int(st.abs().sum()) == 0 and not gI.any() and not lam.any()


def test_c_entries_validate_arguments(oa):
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    d = torch.zeros(4096, dtype=torch.float64, device="cuda")
    i4 = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p, q = d.data_ptr(), i4.data_ptr()

    def rhs(B=1, Nn=4, Ne=3, geo=p, EA=p, E=p, conn=q, ptr=q, idx=q, I=p, out=p):
        return lib.ops_frame_adjoint_rhs_f64(B, Nn, Ne, geo, EA, E, conn, ptr, idx, I, None, None, None, None, out, None)

    def contract(B=1, Nn=4, Ne=3, geo=p, E=p, conn=q, disp=p, lam=p, gI=p):
        return lib.ops_frame_grad_contract_f64(B, Nn, Ne, geo, E, conn, disp, lam, None, None, None, None, None, gI, None)

    for call, required in ((rhs, ("geo", "EA", "E", "conn", "ptr", "idx", "I", "out")),
                           (contract, ("geo", "E", "conn", "disp", "lam", "gI"))):
        assert call(B=0) == _cabi.OK
        assert call(B=0, **{required[0]: None}) == _cabi.OK              # nothing is read for an empty batch
        assert call(B=-1) == _cabi.ERR_INVALID_ARG
        assert call(Nn=-4) == _cabi.ERR_INVALID_ARG and call(Nn=1) == _cabi.ERR_INVALID_ARG
        assert call(Ne=-3) == _cabi.ERR_INVALID_ARG and call(Ne=0) == _cabi.ERR_INVALID_ARG
        for name in required:
            assert call(**{name: None}) == _cabi.ERR_INVALID_ARG, name
    torch.cuda.synchronize()


def test_singular_frames_get_nan_and_leave_the_others_alone(oa):
    r = _reference("4x2", 12)
    topo = r["topo"]
    I = r["I"].copy()
    bad = [2, 7, 8]
    I[2, 3] = -0.1
    I[7, :] = 0.0
    I[8, -1] = -1.0

    def grads(rows):
        It, Lt = _gpu(I[rows]).requires_grad_(True), _gpu(r["loads"][rows]).requires_grad_(True)
        s = oa.differentiable_frame_solve(topo, It, Lt)
        cot = [_gpu(c[rows]) for c in r["cot"]]
        L = sum((torch.nan_to_num(o, nan=0.0) * c).sum() for o, c in zip(s[:4], cot))
        g = torch.autograd.grad(L, [It, Lt])
        st = oa.frame_solve_vjp(topo, It.detach(), s.disp.detach(), *cot, status=s.status)[2]
        return [t.cpu() for t in g], s.status.cpu(), st.cpu()

    (gI, gL), st_fwd, st = grads(np.arange(12))
    for b in range(12):
        if b in bad:
            assert int(st[b]) != 0 and int(st_fwd[b]) != 0
            assert torch.isnan(gI[b]).all() and torch.isnan(gL[b]).all()
        else:
            assert int(st[b]) == 0 and int(st_fwd[b]) == 0
            (gI1, gL1), _, _ = grads(np.array([b]))
            assert torch.equal(gI[b], gI1[0]) and torch.equal(gL[b], gL1[0]), b


def test_opcheck_both_operators(oa):
    r = _reference("2x3", 5)
    topo = r["topo"]
    from openpystruct_amd import frames, torch_op
    tid = torch_op._topology_id(topo)
    I, loads = _gpu(r["I"]), _gpu(r["loads"])
    fwd, vjp = torch.ops.openpystruct_amd.frame_solve.default, torch.ops.openpystruct_amd.frame_solve_vjp.default
    torch.library.opcheck(fwd, (I, loads, topo.Nn, tid))
    torch.library.opcheck(fwd, (I, topo.d_loads, topo.Nn, tid))
    torch.library.opcheck(fwd, (I.clone().requires_grad_(True), loads.clone().requires_grad_(True), topo.Nn, tid))
    s = frames.frame_solve(topo, I, loads)
    g = [_gpu(c) for c in r["cot"]]
    torch.library.opcheck(vjp, (I, s.disp, s.status) + tuple(g) + (tid,))
    torch.library.opcheck(vjp, (I, s.disp, None, g[0], None, None, g[3], tid))


def test_operator_keeps_its_topology_alive_and_refuses_a_topology_it_does_not_know(oa):
    """The operators name the FrameTopology by an integer: the autograd graph holds the object until backward has run; a node
    count that is not the topology's, or an integer nothing is registered under, is an error."""
    import gc
    from openpystruct_amd import frames, torch_op
    r = _reference("2x3", 5)
    I = _gpu(r["I"]).requires_grad_(True)
    s = oa.differentiable_frame_solve(frames.grid_frame(2, 3), I, _gpu(r["loads"]))       # nothing else refers to this topology
    gc.collect()
    gI, = torch.autograd.grad(sum((o * _gpu(c)).sum() for o, c in zip(s[:4], r["cot"])), [I])
    assert _nrel(gI.cpu().numpy(), r["gI"], r["sI"]) < max(1e-8, 4e-16 * r["kappa"])
    with pytest.raises(ValueError, match="n_nodes = 13"):
        torch.ops.openpystruct_amd.frame_solve(I.detach(), _gpu(r["loads"]), 13, torch_op._topology_id(r["topo"]))
    with pytest.raises(RuntimeError, match="no live FrameTopology"):
        torch.ops.openpystruct_amd.frame_solve(I.detach(), _gpu(r["loads"]), r["topo"].Nn, 1 << 40)


def test_forward_status_alone_marks_a_frame(oa):
    """The contraction's status_fwd: a frame flagged by the forward's status gets a NaN gI row even where its displacements and
    the adjoint solve are healthy; the other rows are bit-equal to the call without it."""
    from openpystruct_amd import frames
    r = _reference("4x2", 5)
    topo, I = r["topo"], _gpu(r["I"])
    s = frames.frame_solve(topo, I, _gpu(r["loads"]))
    cot = [_gpu(c) for c in r["cot"]]
    st = torch.zeros(5, dtype=torch.int32, device="cuda"); st[3] = 7
    gI0, lam0, adj0 = oa.frame_solve_vjp(topo, I, s.disp, *cot)
    gI1, lam1, adj1 = oa.frame_solve_vjp(topo, I, s.disp, *cot, status=st)
    assert torch.isnan(gI1[3]).all() and torch.equal(lam1, lam0) and int(adj1.abs().sum()) == 0
    keep = [0, 1, 2, 4]
    assert torch.equal(gI1[keep], gI0[keep]) and not torch.isnan(gI0).any()
    assert torch.equal(oa.frame_solve_vjp(topo, I, s.disp, *cot, status=torch.zeros_like(st))[0], gI0)


def test_forward_and_backward_capture_in_a_graph(oa):
    """Forward + backward captured after an eager warm-up on the capture stream (the warm-up builds that stream's workspaces and
    plans eagerly: a plan kernel that is only recorded is the hazard tests/test_gpu_frames.py documents)."""
    r = _reference("4x2", 5)
    I, loads = _gpu(r["I"]).requires_grad_(True), _gpu(r["loads"]).requires_grad_(True)
    cot = [_gpu(c) for c in r["cot"]]

    def step():
        s = oa.differentiable_frame_solve(r["topo"], I, loads)
        L = sum((o * c).sum() for o, c in zip(s[:4], cot))
        return torch.autograd.grad(L, [I, loads])

    eager = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            captured = step()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    for p, q in zip(captured, eager):
        assert torch.equal(p, q)


def _fr_loss(cfg, I, V, M):
    """compute_combined_loss of the reference's frame script (FR:141-160) in float64."""
    return (I.sum() + cfg.alpha_moment * (M ** 2 / (2 * cfg.E * I + 1e-8)).sum()
            + cfg.alpha_shear * (V ** 2 / (cfg.G * (cfg.k * I ** 0.5))).sum())


def test_exact_frame_loss_gradient_matches_differences_and_differs_from_explicit_terms(oa):
    """The exact gradient of the reference's frame loss on a 3 x 3 frame against central differences of the GPU forward (step and
    bound of the test above: the same quotient of the CPU oracle deviates from dense autograd by at most 1e-7), and against the
    explicit-terms gradient (V and M detached: what the sizing kernels and the reference's own loop use), from which it differs
    by ~10 % in norm (profiles/frame_vjp_notes.md)."""
    from openpystruct_amd import frames
    cfg = frames.FrameConfig()
    topo = frames.grid_frame(3, 3, cfg)
    rng = np.random.default_rng(2)
    I0 = fd.random_inertias(rng, 4, topo.Ne)
    I = _gpu(I0).requires_grad_(True)
    s = oa.differentiable_frame_solve(topo, I)
    exact, = torch.autograd.grad(_fr_loss(cfg, I, s.V, s.M), [I])
    explicit, = torch.autograd.grad(_fr_loss(cfg, I, s.V.detach(), s.M.detach()), [I])

    def L(Iv):
        t = frames.frame_solve(topo, Iv)
        return float(_fr_loss(cfg, Iv, t.V, t.M))

    h = 1e-4
    for _ in range(3):
        d = _gpu(rng.standard_normal(I0.shape) * I0)
        fd_ = (L(I.detach() + h * d) - L(I.detach() - h * d)) / (2 * h)
        print(f"exact vs differences {abs(fd_ - float((exact * d).sum())) / abs(fd_):.3e}")
        assert abs(fd_ - float((exact * d).sum())) <= 2e-5 * abs(fd_)
    ratio = float((exact - explicit).norm() / exact.norm())
    print(f"|exact - explicit| / |exact| = {ratio:.6f}")
    assert ratio > 0


def test_plain_frame_solve_keeps_no_graph_and_streams_do_not_disturb_each_other(oa):
    from openpystruct_amd import frames
    r = _reference("4x2", 300)
    topo = r["topo"]
    Ia, la = _gpu(r["I"]).requires_grad_(True), _gpu(r["loads"])
    s = frames.frame_solve(topo, Ia, la)
    assert not any(t.requires_grad for t in s)
    d = oa.differentiable_frame_solve(topo, Ia, la)
    assert all(t.requires_grad for t in d[:4]) and not d.status.requires_grad
    # a forward on one stream while another stream runs forward + backward on the same topology
    rb = _reference("4x2", 300, True)
    cot = [_gpu(c) for c in r["cot"]]

    def fwd_bwd():
        Ib = _gpu(rb["I"]).requires_grad_(True)
        t = oa.differentiable_frame_solve(topo, Ib, _gpu(rb["loads"]))
        return torch.autograd.grad(sum((o * c).sum() for o, c in zip(t[:4], cot)), [Ib])[0]

    ra, gb = frames.frame_solve(topo, Ia.detach(), la), fwd_bwd()
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(sa):
            qa = frames.frame_solve(topo, Ia.detach(), la)
        with torch.cuda.stream(sb):
            qg = fwd_bwd()
    torch.cuda.synchronize()
    assert relerr(qa.disp.cpu().numpy().reshape(300, -1), ra.disp.cpu().numpy().reshape(300, -1)) < 1e-10
    assert relerr(qa.forces.cpu().numpy().reshape(300, -1), ra.forces.cpu().numpy().reshape(300, -1)) < 1e-9
    assert _nrel(qg.cpu().numpy(), gb.cpu().numpy()) < 1e-9
    assert len(topo._ws) >= 3 and len(topo._ws_adjoint) >= 2
