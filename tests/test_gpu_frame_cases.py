"""Several load cases per frame on one kept factorisation, on the GPU: the keeping solve
(`ops_frame_factor_solve_f64`, the wave-per-frame kernel with KEEP) and the substitution-only kernel of csrc/frame_resolve.hpp
(`ops_frame_resolve_f64`) behind `frame_factor` / `frame_resolve` / `frame_solve_cases` / `frame_solve_cases_vjp` -- against the
3-DOF oracle per (frame, case), against `frame_solve` and `frame_solve_vjp` on the rows, against autograd of the dense float64
model summed over the cases, and bit for bit where the arithmetic is the same.

Bit-for-bit comparisons between two FACTORISATIONS use frames of at most 64 elements (one wavefront fills the plan: the order
of the assembly's LDS atomics is then fixed, tests/test_gpu_frame_grad.py); comparisons on ONE kept factor use every shape."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import beam_oracle as bo  # noqa: E402
from tests import frame_dense as fd  # noqa: E402
from tests import frame_dense_w as fw  # noqa: E402
from tests.helpers import relerr  # noqa: E402
from tests.test_gpu_frame_grad import _cotangents, _gpu, _nrel, _tuned_kernels_for_every_batch, oa  # noqa: E402,F401

SENT = -98765.4321

# name -> (constructor arguments, n_eq, kd); None: not a grid
SHAPES = {"1x1": ((1, 1), 6, 5), "4x2": ((4, 2), 30, 8), "3x6": ((3, 6), 72, 14), "10x2n": ((10, 2, "node"), 66, 35),
          "10x4n": ((10, 4, "node"), 132, 35), "12x2n": ((12, 2, "node"), 78, 41), "16x2n": ((16, 2, "node"), 102, 53),
          "2x3": ((2, 3), None, None), "general": None, "hub": None}
FORWARD = ["1x1", "4x2", "3x6", "10x2n", "10x4n", "12x2n", "16x2n", "general", "hub"]
BATCHES = [(5, 3), (1, 1), (3, 9)]


@functools.lru_cache(maxsize=None)
def _topology(name):
    from openpystruct_amd import frames
    if name == "general":
        return fd.custom_frame(2, 2, True, True, "cuda")
    if name == "hub":
        return fd.hub_frame("cuda")
    args, n_eq, kd = SHAPES[name]
    topo = frames.grid_frame(args[0], args[1], numbering=args[2] if len(args) > 2 else "auto")
    if n_eq is not None:
        assert (topo.n_eq, topo.kd) == (n_eq, kd), (name, topo.n_eq, topo.kd)
    return topo


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    """Bit equality of two device tensors (NaN payloads included)."""
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _same_solution(p, q):
    return all(_same(a, b) for a, b in zip(p, q))


@functools.lru_cache(maxsize=None)
def _inputs(name, B, C):
    """B designs, C load cases each: distinct nodal loads and element loads per (frame, case); case 1 (where there is one) has no
    element load at all."""
    topo = _topology(name)
    rng = np.random.default_rng(sum(map(ord, name)) + 17 * B + C)
    I = fd.random_inertias(rng, B, topo.Ne)
    loads = (np.broadcast_to(topo.nodal_loads, (B, C, topo.Nn, 3)) * rng.uniform(0.5, 2.0, size=(B, C, 1, 1))
             + rng.standard_normal((B, C, topo.Nn, 3)) * 1e3)
    w = fw.random_element_loads(rng, B * C, topo.Ne).reshape(B, C, topo.Ne, 2)
    if C > 1:
        w[:, 1] = 0.0
    for a in (I, loads, w):
        a.setflags(write=False)
    return topo, I, loads, w


@functools.lru_cache(maxsize=None)
def _oracle(name, B, C):
    topo, I, loads, w = _inputs(name, B, C)
    ref = [bo.solve_model_3dof(topo.coords, topo.conn, topo.A, topo.E, I[b], topo.fix3, loads[b, c], wy=w[b, c, :, 0], wx=w[b, c, :, 1])
           for b in range(B) for c in range(C)]
    assert all(r[2] == 0 for r in ref)
    disp, forces = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    disp.setflags(write=False); forces.setflags(write=False)
    return disp, forces


def _assert_rows(sol, disp, forces):
    """The bounds of tests/test_gpu_frame_loads.py::_assert_solution on the B * C rows."""
    R = disp.shape[0]
    assert int(sol.status.abs().sum()) == 0
    e_d = relerr(sol.disp.cpu().numpy().reshape(R, -1), disp.reshape(R, -1))
    e_f = relerr(sol.forces.cpu().numpy().reshape(R, -1), forces.reshape(R, -1))
    print(f"disp {e_d:.3e} forces {e_f:.3e}")
    assert e_d < 1e-8 and e_f < 1e-7
    assert _same(sol.V, sol.forces[..., 1]) and _same(sol.M, sol.forces[..., 2])


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C", BATCHES)
@pytest.mark.parametrize("name", FORWARD)
def test_cases_vs_oracle_per_frame_and_case(oa, name, B, C):
    topo, I, loads, w = _inputs(name, B, C)
    sol = oa.frame_solve_cases(topo, _gpu(I), _gpu(loads), _gpu(w))
    assert sol.disp.shape == (B, C, topo.Nn, 3) and sol.forces.shape == (B, C, topo.Ne, 6) and sol.status.shape == (B, C)
    assert sol.V.shape == sol.M.shape == (B, C, topo.Ne) and sol.status.dtype == torch.int32
    _assert_rows(sol, *_oracle(name, B, C))


@pytest.mark.parametrize("name", FORWARD)
def test_cases_vs_frame_solve_case_by_case(oa, name):
    """`frame_solve_cases(...)[:, c]` against `frame_solve` with that case's loads (another kernel family, another order)."""
    from openpystruct_amd import frames
    topo, I, loads, w = _inputs(name, 5, 3)
    fac = oa.frame_factor(topo, _gpu(I))
    sol = oa.frame_resolve(fac, _gpu(loads), _gpu(w))
    disp, forces = [], []
    for c in range(3):
        s = frames.frame_solve(topo, _gpu(I), _gpu(loads[:, c]), element_loads=_gpu(w[:, c]))
        assert int(s.status.abs().sum()) == 0
        disp.append(s.disp.cpu().numpy()); forces.append(s.forces.cpu().numpy())
    _assert_rows(sol, np.stack(disp, 1).reshape(15, topo.Nn, 3), np.stack(forces, 1).reshape(15, topo.Ne, 6))
    # the keeping solve itself: the topology's own loads, frame_solve's answer to its tolerances
    own = frames.frame_solve(topo, _gpu(I))
    assert fac.status is fac.solution.status and int(fac.status.abs().sum()) == 0
    assert relerr(fac.solution.disp.cpu().numpy().reshape(5, -1), own.disp.cpu().numpy().reshape(5, -1)) < 1e-8
    assert relerr(fac.solution.forces.cpu().numpy().reshape(5, -1), own.forces.cpu().numpy().reshape(5, -1)) < 1e-7
    # None: the topology's element loads in every case
    s0 = oa.frame_resolve(fac, topo.d_loads.expand(5, 1, -1, -1).contiguous())
    assert relerr(s0.disp[:, 0].cpu().numpy().reshape(5, -1), own.disp.cpu().numpy().reshape(5, -1)) < 1e-8
    assert relerr(s0.forces[:, 0].cpu().numpy().reshape(5, -1), own.forces.cpu().numpy().reshape(5, -1)) < 1e-7


def _c_factor(lib, topo, I, loads, w, override=None):
    """ops_frame_factor_solve_f64 into sentinel-filled outputs."""
    B = I.shape[0]
    f64 = dict(dtype=torch.float64, device="cuda")
    out = [torch.full((B, topo.Nn, 3), SENT, **f64), torch.full((B, topo.Ne, 6), SENT, **f64), torch.full((B, topo.Ne), SENT, **f64),
           torch.full((B, topo.Ne), SENT, **f64), torch.full((B,), -7, dtype=torch.int32, device="cuda")]
    nbytes = int(lib.ops_frame_factor_workspace_bytes(max(B, 1), topo.n_eq, topo.kd)) or 4096
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    a = dict(B=B, Nn=topo.Nn, Ne=topo.Ne, n_eq=topo.n_eq, kd=topo.kd, geo=topo.d_geo.data_ptr(), EA=topo.d_EA.data_ptr(), E=topo.d_E.data_ptr(),
             w=w.data_ptr(), elem_eq=topo.d_elem_eq.data_ptr(), node_eq=topo.d_node_eq.data_ptr(), I=I.data_ptr(), loads=loads.data_ptr(),
             lbs=3 * topo.Nn if loads.dim() == 3 else 0, disp=out[0].data_ptr(), forces=out[1].data_ptr(), V=out[2].data_ptr(),
             M=out[3].data_ptr(), status=out[4].data_ptr(), factor=ws.data_ptr(), factor_bytes=nbytes,
             stream=torch.cuda.current_stream().cuda_stream)
    a.update(override or {})
    rc = lib.ops_frame_factor_solve_f64(*a.values())
    torch.cuda.synchronize()
    return rc, out, ws


def _c_resolve(lib, topo, I, rhs, C, fstat, ws, override=None):
    """ops_frame_resolve_f64 into sentinel-filled outputs."""
    B = I.shape[0]
    f64 = dict(dtype=torch.float64, device="cuda")
    out = [torch.full((B, C, topo.Nn, 3), SENT, **f64), torch.full((B, C, topo.Ne, 6), SENT, **f64), torch.full((B, C, topo.Ne), SENT, **f64),
           torch.full((B, C, topo.Ne), SENT, **f64), torch.full((B, C), -7, dtype=torch.int32, device="cuda")]
    a = dict(B=B, C=C, Nn=topo.Nn, Ne=topo.Ne, n_eq=topo.n_eq, kd=topo.kd, geo=topo.d_geo.data_ptr(), EA=topo.d_EA.data_ptr(),
             E=topo.d_E.data_ptr(), elem_eq=topo.d_elem_eq.data_ptr(), node_eq=topo.d_node_eq.data_ptr(), I=I.data_ptr(), rhs=rhs.data_ptr(),
             rbs=C * 3 * topo.Nn if rhs.dim() == 4 else 0, fstat=fstat.data_ptr(), disp=out[0].data_ptr(), forces=out[1].data_ptr(),
             V=out[2].data_ptr(), M=out[3].data_ptr(), status=out[4].data_ptr(), factor=ws.data_ptr(), factor_bytes=ws.numel(),
             stream=torch.cuda.current_stream().cuda_stream)
    a.update(override or {})
    rc = lib.ops_frame_resolve_f64(*a.values())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", FORWARD)
def test_resolve_of_the_keeping_solves_own_loads_returns_its_bits(oa, name):
    """The same arithmetic in the same order: with no element loads, the re-solve of the loads the keeping solve was given (C = 1)
    is that solve's disp, forces, V and M bit for bit."""
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    topo, I, loads, _ = _inputs(name, 5, 3)
    I, l0 = _gpu(I), _gpu(loads[:, 0])
    zero_w = torch.zeros((topo.Ne, 2), dtype=torch.float64, device="cuda")
    rc, kept, ws = _c_factor(lib, topo, I, l0, zero_w)
    assert rc == _cabi.OK and int(kept[4].abs().sum()) == 0 and not any(bool((t == SENT).any()) for t in kept[:4])
    rc, again = _c_resolve(lib, topo, I, l0.unsqueeze(1).contiguous(), 1, kept[4], ws)
    assert rc == _cabi.OK and int(again[4].abs().sum()) == 0
    for p, q in zip(again[:4], kept[:4]):
        assert _same(p[:, 0], q)


@pytest.mark.parametrize("name", FORWARD)
def test_a_case_depends_on_its_own_right_hand_side_alone(oa, name):
    """On one kept factor: case c of a (5, 3) call is bit-equal to the same case solved alone (C = 1: another NR), at another case
    index of a C = 9 call (three passes, the last one partial) and with shared [C,Nn,3] loads against their replication."""
    topo, I, loads, w = _inputs(name, 5, 3)
    fac = oa.frame_factor(topo, _gpu(I))
    L, Wl = _gpu(loads), _gpu(w)
    sol = oa.frame_resolve(fac, L, Wl)
    assert int(sol.status.abs().sum()) == 0
    for c in range(3):
        alone = oa.frame_resolve(fac, L[:, c:c + 1].contiguous(), Wl[:, c:c + 1].contiguous())
        assert _same_solution([t[:, 0] for t in alone], [t[:, c] for t in sol]), c
    two = oa.frame_resolve(fac, L[:, 1:].contiguous(), Wl[:, 1:].contiguous())                    # C = 2
    assert _same_solution(two, [t[:, 1:] for t in sol])
    order = [2, 0, 1, 1, 2, 0, 0, 2, 1]
    nine = oa.frame_resolve(fac, L[:, order].contiguous(), Wl[:, order].contiguous())
    for k, c in enumerate(order):
        assert _same_solution([t[:, k] for t in nine], [t[:, c] for t in sol]), (k, c)
    shared = oa.frame_resolve(fac, L[0].contiguous(), Wl[0].contiguous())
    repl = oa.frame_resolve(fac, L[:1].expand(5, -1, -1, -1).contiguous(), Wl[:1].expand(5, -1, -1, -1).contiguous())
    assert _same_solution(shared, repl) and int(shared.status.abs().sum()) == 0
    mixed = oa.frame_resolve(fac, L[0].contiguous(), Wl[:1].expand(5, -1, -1, -1).contiguous())
    assert _same_solution(mixed, repl)


@pytest.mark.parametrize("name", ["1x1", "4x2", "3x6", "10x2n", "12x2n", "general"])
def test_a_case_does_not_depend_on_the_batch_or_its_position(oa, name):
    """Another factorisation (frames of at most 64 elements, see the module's docstring): frames 4, 0, 2 of the batch of five as a
    batch of three, in that order."""
    topo, I, loads, w = _inputs(name, 5, 3)
    assert topo.Ne <= 64
    sol = oa.frame_solve_cases(topo, _gpu(I), _gpu(loads), _gpu(w))
    pick = [4, 0, 2]
    sub = oa.frame_solve_cases(topo, _gpu(I[pick]), _gpu(loads[pick]), _gpu(w[pick]))
    assert _same_solution(sub, [t[pick] for t in sol]) and int(sub.status.abs().sum()) == 0


def test_failed_frames_are_nan_in_every_case_and_leave_the_others_alone(oa):
    """The construction of tests/test_gpu_frame_grad.py (test_singular_frames_get_nan_and_leave_the_others_alone): a status path,
    nothing is provoked on the device."""
    topo, I, loads, w = _inputs("4x2", 12, 3)
    healthy = oa.frame_solve_cases(topo, _gpu(I), _gpu(loads), _gpu(w))
    assert int(healthy.status.abs().sum()) == 0
    Ib = I.copy()
    Ib[2, 3] = -0.1
    Ib[7, :] = 0.0
    bad, good = [2, 7], [b for b in range(12) if b not in (2, 7)]
    fac = oa.frame_factor(topo, _gpu(Ib))
    sol = oa.frame_resolve(fac, _gpu(loads), _gpu(w))
    assert bool((fac.status[bad] != 0).all()) and bool((fac.status[good] == 0).all())
    assert bool((sol.status[bad] == 1).all()) and bool((sol.status[good] == 0).all())
    for t in sol[:4]:
        assert bool(torch.isnan(t[bad]).all())
    assert _same_solution([t[good] for t in sol], [t[good] for t in healthy])
    # the gradient: NaN rows for the failed frames
    cot = [_gpu(c).reshape((12, 3) + c.shape[1:]) for c in _cotangents(np.random.default_rng(3), 36, topo.Nn, topo.Ne)]
    gI, gL, gW = oa.frame_solve_cases_vjp(fac, sol, *cot)
    for t in (gI, gL, gW):
        assert bool(torch.isnan(t[bad]).all()) and bool(torch.isfinite(t[good]).all())


# ---------------------------------------------------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gradient_reference(name):
    """B = 5, C = 3: autograd of the dense float64 model on the 15 rows with I repeated per case -- the sum over the cases is
    autograd's own."""
    B, C = 5, 3
    topo, I, loads, w = _inputs(name, B, C)
    case = fd.case_of(topo)
    R = B * C
    cot = _cotangents(np.random.default_rng(sum(map(ord, name)) + 1), R, topo.Nn, topo.Ne)
    It, Lt, Wt = (torch.tensor(a, requires_grad=True) for a in (I, loads.reshape(R, topo.Nn, 3), w.reshape(R, topo.Ne, 2)))
    outs = fw.dense_frame_solve_w(case, It.repeat_interleave(C, 0), Lt, Wt)
    loss = sum((o * torch.tensor(c)).sum() for o, c in zip(outs, cot))
    gI, lam, gW = (g.numpy() for g in torch.autograd.grad(loss, [It, Lt, Wt]))
    outs = [o.detach().numpy() for o in outs]
    kappa = max(fd.cond_free(case, I[b]) for b in range(3))
    sI = fd.gI_term_scale(case, outs[0], lam, fd.fold(R, topo.Ne, *cot[1:]))
    for a in (gI, lam, gW, *cot):
        a.setflags(write=False)
    return dict(cot=cot, gI=gI, gL=lam.reshape(B, C, topo.Nn, 3), gW=gW.reshape(B, C, topo.Ne, 2), kappa=kappa, sI=sI)


@pytest.mark.parametrize("name", ["2x3", "10x2n", "general"])
def test_vjp_matches_dense_autograd_and_the_row_by_row_vjp(oa, name):
    from openpystruct_amd import frames
    B, C = 5, 3
    topo, I, loads, w = _inputs(name, B, C)
    r = _gradient_reference(name)
    Ig, Lg, Wg = _gpu(I), _gpu(loads), _gpu(w)
    fac = oa.frame_factor(topo, Ig)
    sol = oa.frame_resolve(fac, Lg, Wg)
    cot = [_gpu(c).reshape((B, C) + c.shape[1:]) for c in r["cot"]]
    gI, gL, gW = oa.frame_solve_cases_vjp(fac, sol, *cot)
    assert gI.shape == (B, topo.Ne) and gL.shape == (B, C, topo.Nn, 3) and gW.shape == (B, C, topo.Ne, 2)
    tol = max(1e-8, 4e-16 * r["kappa"])
    eI, eL, eW = _nrel(gI.cpu().numpy(), r["gI"], r["sI"]), _nrel(gL.cpu().numpy(), r["gL"]), _nrel(gW.cpu().numpy(), r["gW"])
    print(f"dense: gI {eI:.3e} g_loads {eL:.3e} g_w {eW:.3e} tol {tol:.3e} kappa {r['kappa']:.3e}")
    assert eI < tol and eL < tol and eW < tol
    # the existing VJP case by case (a factorisation each), summed over the cases
    sI, sL, sW = torch.zeros_like(gI), [], []
    for c in range(C):
        s = frames.frame_solve(topo, Ig, Lg[:, c].contiguous(), element_loads=Wg[:, c].contiguous())
        cc = [t[:, c].contiguous() for t in cot]
        gIc, lam, st = oa.frame_solve_vjp(topo, Ig, s.disp, *cc, status=s.status)
        sW.append(oa.frame_element_load_vjp(topo, lam, *cc[1:], status=s.status, status_adj=st))
        sI += gIc
        sL.append(lam)
    eI = _nrel(gI.cpu().numpy(), sI.cpu().numpy(), r["sI"])
    eL, eW = _nrel(gL.cpu().numpy(), torch.stack(sL, 1).cpu().numpy()), _nrel(gW.cpu().numpy(), torch.stack(sW, 1).cpu().numpy())
    print(f"rows:  gI {eI:.3e} g_loads {eL:.3e} g_w {eW:.3e}")
    assert eI < tol and eL < tol and eW < tol


def test_null_cotangents_equal_zeros(oa):
    topo, I, loads, w = _inputs("4x2", 5, 3)
    fac = oa.frame_factor(topo, _gpu(I))
    sol = oa.frame_resolve(fac, _gpu(loads), _gpu(w))
    cot = [_gpu(c).reshape((5, 3) + c.shape[1:]) for c in _cotangents(np.random.default_rng(9), 15, topo.Nn, topo.Ne)]
    for mask in range(16):
        c_null = [c if not (mask >> k) & 1 else None for k, c in enumerate(cot)]
        c_zero = [c if not (mask >> k) & 1 else torch.zeros_like(c) for k, c in enumerate(cot)]
        for u, v in zip(oa.frame_solve_cases_vjp(fac, sol, *c_null), oa.frame_solve_cases_vjp(fac, sol, *c_zero)):
            assert _same(u, v), mask
    gI, gL, gW = oa.frame_solve_cases_vjp(fac, sol)
    assert not gI.any() and not gL.any() and not gW.any()


# ---------------------------------------------------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------------------------------------------------
def test_half_bandwidth_56_is_refused(oa):
    from openpystruct_amd import _cabi, frames
    lib = _cabi.load()
    topo = frames.grid_frame(17, 2, numbering="node")
    assert topo.kd == 56
    assert lib.ops_frame_factor_workspace_bytes(5, topo.n_eq, topo.kd) == 0
    assert lib.ops_frame_factor_workspace_bytes(5, topo.n_eq, 55) > 0
    I = _gpu(fd.random_inertias(np.random.default_rng(0), 5, topo.Ne))
    loads = topo.d_loads.expand(5, -1, -1).contiguous()
    rc, out, ws = _c_factor(lib, topo, I, loads, topo.d_w)
    assert rc == _cabi.ERR_UNSUPPORTED and all(bool((t == SENT).all()) for t in out[:4]) and bool((out[4] == -7).all())
    rc, out = _c_resolve(lib, topo, I, loads.unsqueeze(1).contiguous(), 1, torch.zeros(5, dtype=torch.int32, device="cuda"), ws)
    assert rc == _cabi.ERR_UNSUPPORTED and all(bool((t == SENT).all()) for t in out[:4]) and bool((out[4] == -7).all())
    with pytest.raises(ValueError, match="frame_solve"):
        oa.frame_factor(topo, I)
    assert int(frames.frame_solve(topo, I).status.abs().sum()) == 0            # ... which serves it


def test_c_entries_refuse_bad_arguments_and_write_nothing(oa):
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    topo, I, loads, _ = _inputs("4x2", 5, 3)
    I, L = _gpu(I), _gpu(loads)
    untouched = lambda out: all(bool((t == SENT).all()) for t in out[:4]) and bool((out[4] == -7).all())      # noqa: E731
    Nn, full = topo.Nn, int(lib.ops_frame_factor_workspace_bytes(5, topo.n_eq, topo.kd))
    assert full > 0 and lib.ops_frame_factor_workspace_bytes(0, topo.n_eq, topo.kd) == 0
    assert lib.ops_frame_factor_workspace_bytes(5, 0, topo.kd) == 0 and lib.ops_frame_factor_workspace_bytes(5, topo.n_eq, -1) == 0

    rc, kept, ws = _c_factor(lib, topo, I, L[:, 0].contiguous(), topo.d_w)
    assert rc == _cabi.OK and not untouched(kept) and int(kept[4].abs().sum()) == 0
    bad = [{k: None} for k in ("geo", "EA", "E", "w", "elem_eq", "node_eq", "I", "loads", "disp", "forces", "V", "M", "factor")]
    bad += [{"B": -1}, {"Nn": 1}, {"Nn": -4}, {"Ne": 0}, {"n_eq": 0}, {"kd": -1}, {"lbs": 3}, {"lbs": -3 * Nn}, {"factor_bytes": full - 8},
            {"factor_bytes": 0}]
    for override in bad:
        rc, out, _ = _c_factor(lib, topo, I, L[:, 0].contiguous(), topo.d_w, override=override)
        assert rc == _cabi.ERR_INVALID_ARG and untouched(out), override
    rc, out, _ = _c_factor(lib, topo, I, L[:, 0].contiguous(), topo.d_w, override={"B": 0, "geo": None})
    assert rc == _cabi.OK and untouched(out)

    rc, out = _c_resolve(lib, topo, I, L, 3, kept[4], ws)
    assert rc == _cabi.OK and not untouched(out) and int(out[4].abs().sum()) == 0
    bad = [{k: None} for k in ("geo", "EA", "E", "elem_eq", "node_eq", "I", "rhs", "fstat", "disp", "forces", "V", "M", "status", "factor")]
    bad += [{"B": -1}, {"C": -1}, {"Nn": 1}, {"Ne": 0}, {"n_eq": 0}, {"kd": -1}, {"rbs": 3 * Nn}, {"rbs": 3}, {"rbs": -9 * Nn}, {"rbs": 9 * Nn + 1},
            {"factor_bytes": full - 8}, {"factor_bytes": 0}]
    for override in bad:
        rc, out = _c_resolve(lib, topo, I, L, 3, kept[4], ws, override=override)
        assert rc == _cabi.ERR_INVALID_ARG and untouched(out), override
    for override in ({"B": 0, "geo": None}, {"C": 0, "rbs": 0, "geo": None}):
        rc, out = _c_resolve(lib, topo, I, L, 3, kept[4], ws, override=override)
        assert rc == _cabi.OK and untouched(out), override
    # values on constrained DOFs are ignored
    junk = L.clone()
    junk[:, :, torch.as_tensor(topo.fix3, device="cuda")] = float("nan")
    rc, clean = _c_resolve(lib, topo, I, L, 3, kept[4], ws)
    rc2, dirty = _c_resolve(lib, topo, I, junk, 3, kept[4], ws)
    assert rc == _cabi.OK and rc2 == _cabi.OK and bool(torch.isfinite(clean[0]).all())
    assert all(_same(p, q) for p, q in zip(clean, dirty))


def test_python_entries_check_their_arguments_and_out_allocates_nothing(oa):
    topo, I, loads, w = _inputs("4x2", 5, 3)
    Ig, L, Wl = _gpu(I), _gpu(loads), _gpu(w)
    fac = oa.frame_factor(topo, Ig)
    assert fac.I is Ig and fac.topo is topo and fac.workspace.dtype == torch.uint8
    sol = oa.frame_resolve(fac, L, Wl)
    first = [t.clone() for t in sol]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = oa.frame_resolve(fac, L, Wl, out=sol)
    torch.cuda.synchronize()
    assert again is sol and torch.cuda.memory_allocated() == before
    assert _same_solution(sol, first)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_resolve(fac, L.cpu(), Wl)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_factor(topo, Ig.cpu())
    for bad_loads in (L[:4].contiguous(), L[..., :2].contiguous(), L.float(), L[0, 0].contiguous()):
        with pytest.raises(ValueError):
            oa.frame_resolve(fac, bad_loads, Wl)
    for bad_w in (Wl[:, :2].contiguous(), Wl[:3].contiguous(), Wl.float()):
        with pytest.raises(ValueError):
            oa.frame_resolve(fac, L, bad_w)
    with pytest.raises(ValueError):
        oa.frame_resolve(fac, L, Wl, out=sol._replace(status=sol.status.long()))
    with pytest.raises(ValueError):
        oa.frame_factor(topo, Ig[:, :-1].contiguous())
    with pytest.raises(ValueError):
        oa.frame_solve_cases_vjp(fac, sol, g_disp=sol.disp[:, :2].contiguous())
