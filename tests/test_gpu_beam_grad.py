"""Gradients through the batched beam solve on the GPU: `ops_beam_solve_vjp_f64` (csrc/beam_vjp.hip), the operator
`openpystruct_amd::beam_solve_vjp` and the autograd formula of `openpystruct_amd::beam_solve` (torch_op.py), checked
against autograd of a dense float64 model (tests/beam_dense.py), against central differences of the GPU forward, and
for the exact gradient of the reference's SingleCore sizing loss."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.beam_dense import cond_free, dense_solve, gI_term_scale, random_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SC, UDL_SC = 200e9, -1000.0        # SingleCore.py:20, uniform_udl


@pytest.fixture(scope="module")
def oa():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    import openpystruct_amd
    from openpystruct_amd import torch_op  # noqa: F401
    return openpystruct_amd


def _gpu(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


def _nrel(a, b, scale=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), scale, 1e-300))


def _op_args(x, E, I, fix, Fy, wy, grad=()):
    """GPU tensors for the operator; the names in `grad` require grad."""
    t = dict(x=_gpu(x), E=_gpu(E), I=_gpu(I), fix=_gpu(fix, torch.uint8), Fy=_gpu(Fy), wy=_gpu(wy))
    for k in grad:
        t[k].requires_grad_(True)
    return t


# (Ne, B, per-beam x / fix, per-element E / wy): every VJP tiling regime (16x7, 32x4, 64x4, 64x8, 64x16), the largest Ne
CASES = [(1, 1, False, False), (2, 7, True, True), (5, 1000, False, True), (13, 7, True, False), (100, 1000, True, True),
         (100, 7, False, False), (120, 7, False, True), (255, 7, True, False), (500, 1, False, True), (1023, 1, False, False),
         (1023, 7, True, True)]


@pytest.mark.parametrize("Ne,B,per_beam,per_elem", CASES)
def test_vjp_matches_dense_autograd(oa, Ne, B, per_beam, per_elem):
    rng = np.random.default_rng(31 * Ne + B + per_beam + 2 * per_elem)
    N = Ne + 1
    x, fix, I, Fy = random_case(rng, B, Ne, per_beam=per_beam)
    E = rng.uniform(1.5e11, 2.5e11, size=(B, Ne)) if per_elem else np.float64(2e11)
    wy = rng.uniform(-2e3, 0, size=(B, Ne)) if per_elem else np.float64(-750.0)
    cot = [rng.standard_normal((B, N)) * 1e3, rng.standard_normal((B, N)) * 1e3, rng.standard_normal((B, Ne)),
           rng.standard_normal((B, Ne))]

    # the dense model (CPU, float64) and its autograd
    td = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in (("E", E), ("I", I), ("Fy", Fy), ("wy", wy))}
    outs_d = dense_solve(torch.tensor(x), td["E"], td["I"], fix, td["Fy"], td["wy"])
    L_d = sum((o * torch.tensor(c)).sum() for o, c in zip(outs_d, cot))
    ref = dict(zip(("E", "I", "Fy", "wy"), (g.numpy() for g in torch.autograd.grad(L_d, [td["E"], td["I"], td["Fy"], td["wy"]]))))
    outs_d = [o.detach().numpy() for o in outs_d]

    # the operator on the GPU
    a = _op_args(x, E, I, fix, Fy, wy, grad=("E", "I", "Fy", "wy"))
    outs = torch.ops.openpystruct_amd.beam_solve(a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"])
    assert int(outs[4].abs().sum()) == 0
    L = sum((o * _gpu(c)).sum() for o, c in zip(outs[:4], cot))
    got = dict(zip(("E", "I", "Fy", "wy"), (g.cpu().numpy() for g in torch.autograd.grad(L, [a["E"], a["I"], a["Fy"], a["wy"]]))))

    beams = range(min(B, 3))
    kappa = max(cond_free(x if x.ndim == 1 else x[b], E if np.ndim(E) == 0 else E[b], I[b], fix if fix.ndim == 1 else fix[b])
                for b in beams)
    tol = max(1e-8, 4e-16 * kappa)
    # the test's model is the forward: pinned first
    for o, r in zip(outs[:4], outs_d):
        assert _nrel(o.detach().cpu().numpy(), r) < max(1e-10, 4e-16 * kappa)
    sI = gI_term_scale(x, I, wy, outs_d, cot)   # gI (and a shared gE) can be a difference of much larger terms
    assert _nrel(got["I"], ref["I"], sI) < tol
    assert _nrel(got["Fy"], ref["Fy"]) < tol
    assert _nrel(got["wy"], ref["wy"]) < tol
    sE = sI * float(np.abs(I).sum()) / float(np.min(E))
    assert _nrel(got["E"], ref["E"], 0.0 if per_elem else sE) < tol
    assert got["E"].shape == np.shape(E) and got["wy"].shape == np.shape(wy)


def test_vjp_matches_central_differences_of_the_forward(oa):
    """Independent of the dense model: directional derivatives in I and wy from the VJP against central differences of
    the GPU forward.  A difference quotient carries the forward's rounding error (~eps cond(K)) divided by the step, so the
    case is a well-conditioned one (Ne = 12, cond ~1e5) and the relative step 1e-4 (truncation error ~1e-8)."""
    rng = np.random.default_rng(5)
    B, Ne = 16, 12
    x, fix, I, Fy = random_case(rng, B, Ne, per_beam=True)
    wy = rng.uniform(-2e3, -100, size=(B, Ne))
    cot = [_gpu(rng.standard_normal(s)) for s in ((B, Ne + 1), (B, Ne + 1), (B, Ne), (B, Ne))]
    cot[0] *= 1e4
    cot[1] *= 1e3

    def loss(I_, w_):
        s = oa.beam_solve(_gpu(x), 2e11, _gpu(I_), _gpu(fix, torch.uint8), _gpu(Fy), _gpu(w_))
        return float(sum((o * c).sum() for o, c in zip(s[:4], cot)))

    a = _op_args(x, 2e11, I, fix, Fy, wy, grad=("I", "wy"))
    outs = torch.ops.openpystruct_amd.beam_solve(a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"])
    gI, gw = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs[:4], cot)), [a["I"], a["wy"]])
    gI, gw = gI.cpu().numpy(), gw.cpu().numpy()
    h = 1e-4
    for _ in range(3):
        dI = rng.standard_normal((B, Ne)) * I            # relative direction
        dw = rng.standard_normal((B, Ne)) * wy
        fd_I = (loss(I + h * dI, wy) - loss(I - h * dI, wy)) / (2 * h)
        fd_w = (loss(I, wy + h * dw) - loss(I, wy - h * dw)) / (2 * h)
        assert abs(fd_I - (gI * dI).sum()) <= 2e-5 * abs(fd_I), (fd_I, (gI * dI).sum())
        assert abs(fd_w - (gw * dw).sum()) <= 2e-5 * abs(fd_w), (fd_w, (gw * dw).sum())


def test_opcheck_both_operators(oa):
    rng = np.random.default_rng(11)
    B, Ne = 5, 30
    x, fix, I, Fy = random_case(rng, B, Ne)
    a = _op_args(x, 2e11, I, fix, Fy, -500.0)
    args = (a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"])
    torch.library.opcheck(torch.ops.openpystruct_amd.beam_solve.default, args)
    a["I"].requires_grad_(True)
    a["Fy"].requires_grad_(True)
    torch.library.opcheck(torch.ops.openpystruct_amd.beam_solve.default, (a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"]))
    s = oa.beam_solve(*args)
    g = [_gpu(rng.standard_normal(t.shape)) for t in (s.v, s.theta, s.V, s.M)]
    vargs = (a["x"], a["E"], a["I"].detach(), a["fix"], a["wy"], s.v, s.theta)
    torch.library.opcheck(torch.ops.openpystruct_amd.beam_solve_vjp.default, vargs + tuple(g))
    torch.library.opcheck(torch.ops.openpystruct_amd.beam_solve_vjp.default, vargs + (g[0], None, None, g[3]))


def test_null_cotangents_and_outputs_equal_zeros(oa):
    """Every NULL cotangent of the C entry is a zero one, and NULL gFy / gwy leave gI unchanged, bit for bit."""
    from openpystruct_amd import _cabi
    rng = np.random.default_rng(3)
    B, Ne = 9, 40
    x, fix, I, Fy = random_case(rng, B, Ne, per_beam=True)
    xs, Es, Is, fs, Fs, ws = _gpu(x), _gpu(2e11), _gpu(I), _gpu(fix, torch.uint8), _gpu(Fy), _gpu(-800.0)
    s = oa.beam_solve(xs, Es, Is, fs, Fs, ws)
    cot = [_gpu(rng.standard_normal(t.shape)) for t in (s.v, s.theta, s.V, s.M)]
    for mask in range(16):
        c_null = [c if not (mask >> k) & 1 else None for k, c in enumerate(cot)]
        c_zero = [c if not (mask >> k) & 1 else torch.zeros_like(c) for k, c in enumerate(cot)]
        p = oa.beam_solve_vjp(xs, Es, Is, fs, ws, s.v, s.theta, *c_null)
        q = oa.beam_solve_vjp(xs, Es, Is, fs, ws, s.v, s.theta, *c_zero)
        for u, w in zip(p, q):
            assert torch.equal(u, w), mask
    full = oa.beam_solve_vjp(xs, Es, Is, fs, ws, s.v, s.theta, *cot)
    lib = _cabi.load()
    N = Ne + 1
    for drop_F, drop_w in ((True, False), (False, True), (True, True)):
        gI = torch.empty_like(Is)
        gF = None if drop_F else torch.empty_like(Fs)
        gw = None if drop_w else torch.empty_like(Is)
        st = torch.empty(B, dtype=torch.int32, device="cuda")
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = lib.ops_beam_solve_vjp_f64(B, Ne, xs.data_ptr(), N, Es.data_ptr(), 0, Is.data_ptr(), Ne, fs.data_ptr(), N,
                                        ws.data_ptr(), 0, s.v.data_ptr(), s.theta.data_ptr(), *[c.data_ptr() for c in cot],
                                        gI.data_ptr(), ptr(gF), ptr(gw), st.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == _cabi.OK
        torch.cuda.synchronize()
        assert torch.equal(gI, full[0]) and torch.equal(st, full[3])
        if gF is not None:
            assert torch.equal(gF, full[1])
        if gw is not None:
            assert torch.equal(gw, full[2])


def test_c_entry_validates_arguments(oa):
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    d = torch.zeros(4096, dtype=torch.float64, device="cuda")
    f8 = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, pf = d.data_ptr(), f8.data_ptr()

    def call(B, Ne, I_bs=None, x=p, v=p, gI=p, x_bs=0):
        return lib.ops_beam_solve_vjp_f64(B, Ne, x, x_bs, p, 0, p, Ne if I_bs is None else I_bs, pf, 0, p, 0, v, p,
                                          None, None, None, None, gI, None, None, None, None)
    assert call(0, 10) == _cabi.OK
    assert call(-1, 10) == 1 and call(1, 0) == 1
    assert call(1, 10, x=None) == 1 and call(1, 10, v=None) == 1 and call(1, 10, gI=None) == 1
    assert call(1, 10, I_bs=9) == 1 and call(1, 10, x_bs=5) == 1
    assert call(1, 1024) == 2


def test_singular_beams_get_nan_and_leave_the_others_alone(oa):
    rng = np.random.default_rng(17)
    B, Ne = 12, 50
    x, fix, I, Fy = random_case(rng, B, Ne, per_beam=True)
    bad = [2, 7, 8]
    I[2, 10] = -0.1
    I[7, :] = 0.0
    I[8, 49] = -1.0
    cot = [rng.standard_normal((B, Ne + 1)), rng.standard_normal((B, Ne + 1)), rng.standard_normal((B, Ne)),
           rng.standard_normal((B, Ne))]

    def grads(rows):
        a = _op_args(x[rows], 2e11, I[rows], fix[rows], Fy[rows], -600.0, grad=("I", "Fy", "wy"))
        outs = torch.ops.openpystruct_amd.beam_solve(a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"])
        L = sum((torch.nan_to_num(o, nan=0.0) * _gpu(c[rows])).sum() for o, c in zip(outs[:4], cot))
        g = torch.autograd.grad(L, [a["I"], a["Fy"]])
        st = oa.beam_solve_vjp(a["x"], a["E"], a["I"].detach(), a["fix"], a["wy"], outs[0], outs[1], *[_gpu(c[rows]) for c in cot])[3]
        return [t.cpu() for t in g], outs[4].cpu(), st.cpu()

    (gI, gF), st_fwd, st = grads(np.arange(B))
    for b in range(B):
        if b in bad:
            assert int(st[b]) != 0 and int(st_fwd[b]) != 0
            assert torch.isnan(gI[b]).all() and torch.isnan(gF[b]).all()
        else:
            assert int(st[b]) == 0
            (gI1, gF1), _, _ = grads(np.array([b]))
            assert torch.equal(gI[b], gI1[0]) and torch.equal(gF[b], gF1[0])


def test_forward_and_backward_capture_in_a_graph(oa):
    rng = np.random.default_rng(23)
    B, Ne = 64, 100
    x, fix, I, Fy = random_case(rng, B, Ne)
    a = _op_args(x, 2e11, I, fix, Fy, -1000.0, grad=("I", "Fy", "wy"))
    cot = [_gpu(rng.standard_normal(s)) for s in ((B, Ne + 1), (B, Ne + 1), (B, Ne), (B, Ne))]

    def step():
        outs = torch.ops.openpystruct_amd.beam_solve(a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"])
        L = sum((o * c).sum() for o, c in zip(outs[:4], cot))
        return torch.autograd.grad(L, [a["I"], a["Fy"], a["wy"]])

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


def _sc_case(i=0):
    from openpystruct_amd import sizing
    z = np.load(os.path.join(ROOT, "tests", "golden", "sizing_reference_sc.npz"))
    nr, nf = int(z["n_rollers"][i]), int(z["n_forces"][i])
    cases = sizing.cases_from_lists(z["node_positions"][i], [z["roller_nodes"][i, :nr].tolist()],
                                    [z["force_nodes"][i, :nf].tolist()], [z["force_values"][i, :nf].tolist()], device="cuda")
    return cases.node_positions[0].contiguous(), cases.fix[0].contiguous(), cases.Fy, z["I_values"][i:i + 1].astype(np.float64)


def _sc_loss(I, V, M, E=E_SC):
    """SingleCore.py:193-197 in float64: sum I + 1e-2 sum M^2 / (2 E I + 1e-6) + 1e-2 sum V^2 / (G 0.03 sqrt I)."""
    G = E / (2 * (1 + 0.3))
    return I.sum() + 1e-2 * (M ** 2 / (2 * E * I + 1e-6)).sum() + 1e-2 * (V ** 2 / (G * (0.03 * I ** 0.5))).sum()


def test_exact_sizing_gradient_matches_differences_and_differs_from_explicit_terms(oa):
    x, fix, Fy, I0 = _sc_case(0)
    wy = torch.tensor(UDL_SC, dtype=torch.float64, device="cuda")
    E = torch.tensor(E_SC, dtype=torch.float64, device="cuda")
    I = _gpu(I0).requires_grad_(True)
    s = oa.differentiable_beam_solve(x, E, I, fix, Fy, wy)
    exact, = torch.autograd.grad(_sc_loss(I, s.V, s.M), [I])
    explicit, = torch.autograd.grad(_sc_loss(I, s.V.detach(), s.M.detach()), [I])   # what the sizing kernels use

    def L(Iv):
        t = oa.beam_solve(x, E, Iv, fix, Fy, wy)
        return float(_sc_loss(Iv, t.V, t.M))

    # relative step 1e-4: at 1e-6 the loss's own rounding noise (the end moments are zero up to rounding, and enter squared)
    # is ~1e-3 of a difference quotient; a dense float64 LU solve shows the same
    rng = np.random.default_rng(2)
    h = 1e-4
    for _ in range(3):
        d = _gpu(rng.standard_normal(I0.shape) * I0)
        fd = (L(I.detach() + h * d) - L(I.detach() - h * d)) / (2 * h)
        assert abs(fd - float((exact * d).sum())) <= 1e-4 * abs(fd)
    for e in (37, 99):                         # and element by element
        d = torch.zeros_like(I.detach()); d[0, e] = float(I0[0, e])
        fd = (L(I.detach() + h * d) - L(I.detach() - h * d)) / (2 * h)
        assert abs(fd - float(exact[0, e]) * float(I0[0, e])) <= 1e-4 * abs(fd)
    # not the same quantity: the explicit-terms gradient misses dV/dI and dM/dI (here they differ by ~60 % in norm)
    assert float((exact - explicit).norm()) > 0.1 * float(exact.norm())


def test_plain_beam_solve_keeps_no_graph_and_x_is_not_differentiable(oa):
    rng = np.random.default_rng(1)
    x, fix, I, Fy = random_case(rng, 3, 20)
    a = _op_args(x, 2e11, I, fix, Fy, -500.0, grad=("I",))
    s = oa.beam_solve(a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"])
    assert not any(t.requires_grad for t in s)
    outs = torch.ops.openpystruct_amd.beam_solve(a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"])
    assert all(o.requires_grad for o in outs[:4]) and not outs[4].requires_grad
    for o, t in zip(outs, s):
        assert torch.equal(o.detach(), t)
    a["x"].requires_grad_(True)
    with pytest.raises(ValueError, match="node coordinates are not differentiable"):
        torch.ops.openpystruct_amd.beam_solve(a["x"], a["E"], a["I"], a["fix"], a["Fy"], a["wy"])
