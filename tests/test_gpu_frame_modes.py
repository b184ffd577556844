"""Natural frequencies and mode shapes on the kept factorisation, on the GPU: the three kernels behind
`ops_frame_mass_apply_f64`, `ops_frame_modes_ritz_f64` and `ops_frame_modes_grad_f64` (csrc/frame_loads.hip, arithmetic
csrc/frame_modes.hpp) and `FrameMass` / `frame_modes` / `frame_solve_modes` / `frame_modes_vjp` / `differentiable_frame_frequencies`
and the command shim's `eigen` -- against the dense float64 reference of tests/frame_modes_ref.py, whose cases (topology, batch, mass
kind, nodal mass, vectors) and elementwise constants this file shares with tests/test_frame_modes_host.py.

Bit-for-bit comparisons between two FACTORISATIONS use frames of at most 64 elements (tests/test_gpu_frame_cases.py)."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import frame_dense as fd  # noqa: E402
from tests import frame_modes_ref as fr  # noqa: E402
from tests.test_gpu_frame_cases import _same  # noqa: E402
from tests.test_gpu_frame_grad import _gpu, _tuned_kernels_for_every_batch, oa  # noqa: E402,F401

SENT = -98765.4321
KEYS = list(fr.CASES)


@functools.lru_cache(maxsize=None)
def _setup(key):
    """(topology, FrameMass, I on the device) of a shared case."""
    import openpystruct_amd as pkg
    case, I, mbar, nodal, kind, p = fr.inputs(key)
    topo = fr.topology(fr.CASES[key][0], "cuda")
    return topo, pkg.FrameMass(topo, mbar, nodal, kind=kind), _gpu(I)


def _guarded(shape, dtype=torch.float64):
    """A sentinel-filled output between two guard regions of 64 elements: (whole buffer, the output view)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 128,), SENT if dtype == torch.float64 else -7, dtype=dtype, device="cuda")
    return whole, whole[64:64 + n].view(shape)


def _guards_intact(whole, out):
    fill = SENT if whole.dtype == torch.float64 else -7
    return bool((whole[:64] == fill).all()) and bool((whole[-64:] == fill).all()) and not bool((out == fill).any())


def _dense_M(key, b):
    case, _, mbar, nodal, kind, _ = fr.inputs(key)
    return fr.dense_M(case, mbar, kind, fr.nodal_of(nodal, b))


# ---------------------------------------------------------------------------------------------------------------------
# the streaming entries alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_mass_apply_alone_matches_the_dense_mass_matrix(oa, key):
    """Elementwise |got - ref| <= c 2^-52 (|M| |x|) with c = tests/frame_modes_ref.py::C_MASS = 4 x 2.69 = 10.76: four times the
    largest ratio that the g++ build of csrc/frame_modes.hpp shows on these inputs (tests/test_frame_modes_host.py pins it); never
    taken from the device.  Measured on the device: ratio at most 2.69 (10x4n-c), the host's figure in every case."""
    from openpystruct_amd import _cabi, frames
    lib = _cabi.load()
    topo, mass, I = _setup(key)
    B = I.shape[0]
    x = fr.mass_apply_x(key)
    xg = _gpu(x)
    whole, y = _guarded((B * 3, topo.Nn, 3))
    adj = frames._adjoint_tables(topo)
    rc = lib.ops_frame_mass_apply_f64(B * 3, 3, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), adj.conn.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(),
                                      mass.d_mass.data_ptr(), mass.consistent, None if mass.d_nodal is None else mass.d_nodal.data_ptr(),
                                      mass.nodal_bstride, xg.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _cabi.OK and _guards_intact(whole, y)
    got = y.cpu().numpy().reshape(B, 3, -1)
    worst = 0.0
    for b in range(B):
        M = _dense_M(key, b)
        ref, scale = x[b] @ M.T, np.abs(x[b]) @ np.abs(M).T
        assert np.all(got[b][scale == 0] == 0.0)
        worst = max(worst, float((np.abs(got[b] - ref)[scale > 0] / (fr.EPS * scale[scale > 0])).max()))
    print(f"mass apply {key}: largest ratio {worst:.3f} (bound {fr.C_MASS})")
    assert worst <= fr.C_MASS


@pytest.mark.parametrize("key", KEYS)
def test_gradient_entry_alone_matches_the_reference(oa, key):
    """Fed the reference's phi: |got - ref| <= c 2^-52 sum_j |g_j| |phi_j|^T |K_b| |phi_j| with c = C_GRAD = 4 x 2.56 = 10.24, four
    times the host's largest ratio; a frame with a non-zero status gets a NaN row.  Measured on the device: ratio at most 2.56
    (10x4n-c)."""
    from openpystruct_amd import _cabi, frames
    lib = _cabi.load()
    topo, _, I = _setup(key)
    case = fr.inputs(key)[0]
    ref = fr.reference(key)
    B = I.shape[0]
    phi = np.stack([r["phi"] for r in ref])
    g = fr.grad_cotangent(key)
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    if B > 1:
        status[B - 1] = 3
    whole, gI = _guarded((B, topo.Ne))
    adj = frames._adjoint_tables(topo)
    phi_g, g_g = _gpu(phi), _gpu(g)
    rc = lib.ops_frame_modes_grad_f64(B, 2, 2, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(),
                                      phi_g.data_ptr(), g_g.data_ptr(), status.data_ptr(), gI.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _cabi.OK and _guards_intact(whole, gI)
    got = gI.cpu().numpy()
    worst = 0.0
    for b in range(B - (B > 1)):
        worst = max(worst, float((np.abs(got[b] - g[b] @ ref[b]["dl"]) / (fr.EPS * fr.grad_scale(case, phi[b], g[b]))).max()))
    print(f"gradient {key}: largest ratio {worst:.3f} (bound {fr.C_GRAD})")
    assert worst <= fr.C_GRAD and (B == 1 or np.isnan(got[B - 1]).all())


# ---------------------------------------------------------------------------------------------------------------------
# the iteration
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_iteration(key, p):
    case, I, _, _, _, _ = fr.inputs(key)
    out = [fr.iterate(case, I[b], _dense_M(key, b), fr.default_start(case, p), 3) for b in range(I.shape[0])]
    return np.stack([[it[0] for it in its] for its in out])                      # [B,3,p]


@pytest.mark.parametrize("p", [1, 2, 8])
@pytest.mark.parametrize("key", KEYS)
def test_ritz_values_after_one_two_and_three_iterations(oa, key, p):
    """From the default start, all p Ritz values against the NumPy restatement of the iteration, relative <= 1e-8: the bound
    tests/test_gpu_frame_cases.py::_assert_rows holds the re-solve's displacements to, whose Rayleigh quotients they are.  On the
    1 x 1 frame (six equations) 8 stands for 4, and for 3 under the lumped matrix: four DOFs carry mass there, four start vectors
    span all of them, and the first pencil X^T M X then has a condition of 4e11 (1e6 with three vectors), at which the reference's own
    Ritz values are good to 1e-4 and not to the bound.
    Measured: after one iteration at most 9.3e-10 (1x1-c, four vectors: condition 5e7) and 3.5e-10 elsewhere (3x6-l, eight vectors);
    after two and three iterations at most 2.2e-13."""
    topo, mass, I = _setup(key)
    p = min(p, 3 if key == "1x1-l" else 4) if key.startswith("1x1") else p
    ref = _reference_iteration(key, p)
    fac = oa.frame_factor(topo, I)
    worst = []
    for t in (1, 2, 3):
        r = oa.frame_modes(fac, mass, n_modes=p, n_vectors=p, iters=t)
        assert r.iterations == t and int(r.status.abs().sum()) == 0 and r.eigenvalues.shape == (I.shape[0], p)
        lam = r.eigenvalues.cpu().numpy()
        worst.append(float(np.abs(lam / ref[:, t - 1] - 1.0).max()))
        assert bool(torch.isinf(r.change).all()) == (t == 1)
    print(f"{key} p {p}: Ritz values after 1, 2, 3 iterations {worst[0]:.2e} {worst[1]:.2e} {worst[2]:.2e}")
    assert max(worst) <= 1e-8


@pytest.mark.parametrize("key,p,start", [("1x1-c", 6, "unit"), ("1x1-l", 4, "unit"), ("general-c", 5, "default"), ("general-c", 7, "default"),
                                         ("10x4n-c", 6, "default")])
def test_ritz_values_at_the_other_vector_counts(oa, key, p, start):
    """The vector counts the test above does not reach: five, six and seven vectors, and the 1 x 1 frame at its largest sizes -- six
    vectors under the consistent matrix (as many as equations), four under the lumped one (as many as DOFs with mass).  There the
    start is `X0` = the unit vectors of the free DOFs (tests/frame_modes_ref.py::unit_start: the first pencil has a condition of 6e6
    and 2e3, where the default start gives 1e17 and 4e11), so `X0` as an argument is checked too.  Ritz values after 1, 2 and 3
    iterations against the reference iteration from the same start, relative <= 1e-8; after 16 iterations the two lowest against dense
    eigh, relative <= 1e-8.  Measured: after one iteration at most 2.7e-11 (10x4n-c, six vectors), after two and three 9.5e-14, after 16
    against eigh 1.2e-10 (general-c, five vectors: its second mode converges slowest)."""
    topo, mass, I = _setup(key)
    case, In = fr.inputs(key)[:2]
    B = I.shape[0]
    x0 = fr.default_start(case, p) if start == "default" else fr.unit_start(case, p, translations_only=key == "1x1-l")
    X0 = None if start == "default" else _gpu(x0.reshape(p, topo.Nn, 3))
    ref = np.stack([[it[0] for it in fr.iterate(case, In[b], _dense_M(key, b), x0, 3)] for b in range(B)])          # [B,3,p]
    fac = oa.frame_factor(topo, I)
    worst = []
    for t in (1, 2, 3):
        r = oa.frame_modes(fac, mass, n_modes=p, n_vectors=p, iters=t, X0=X0)
        assert int(r.status.abs().sum()) == 0
        worst.append(float(np.abs(r.eigenvalues.cpu().numpy() / ref[:, t - 1] - 1.0).max()))
    r = oa.frame_modes(fac, mass, n_modes=2, n_vectors=p, iters=fr.ITERS, X0=X0 if X0 is None else X0.expand(B, -1, -1, -1).contiguous())
    dense = np.stack([d["lam"][:2] for d in fr.reference(key)])
    e16 = float(np.abs(r.eigenvalues.cpu().numpy() / dense - 1.0).max())
    print(f"{key} p {p} {start}: Ritz values after 1, 2, 3 iterations {worst[0]:.2e} {worst[1]:.2e} {worst[2]:.2e}; after 16 against eigh {e16:.2e}")
    assert max(worst) <= 1e-8 and e16 <= 1e-8 and int(r.status.abs().sum()) == 0


@pytest.mark.parametrize("key,p", [("1x1-c", 4), ("general-l", 8), ("hub-c", 3)])
def test_ritz_entry_alone_between_guard_regions(oa, key, p):
    """`ops_frame_modes_ritz_f64` by itself, every output between sentinel-filled guard regions, fed X, MX and R of the reference's second
    iteration: 1x1 (12 entries per vector: fewer than a wave), hub (57 entries) and general (27 entries) with B = 5, 67 and 5 frames -- none
    a multiple of the four frames of a block.  Ritz values relative <= 1e-8 against the reference's, Q^T M Q = I to 1e-10, the next
    R = M Q, change against the values `lambda` held, status zero, nothing outside the outputs written.
    Measured: Ritz values 4.2e-15, orthonormality 3.6e-15, the next R 2.3e-16."""
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    topo, _, I = _setup(key)
    case, In = fr.inputs(key)[:2]
    B, n = I.shape[0], 3 * topo.Nn
    assert B % 4 != 0
    its = [fr.iterate(case, In[b], _dense_M(key, b), fr.default_start(case, p), 2) for b in range(B)]
    X, MX, R = (_gpu(np.stack([it[1][k] for it in its])) for k in (3, 4, 5))
    prev = np.stack([it[0][0] for it in its])
    bufs = {name: _guarded(shape, dt) for name, shape, dt in (("R", (B, p, n), torch.float64), ("Q", (B, p, n), torch.float64),
                                                                ("lam", (B, p), torch.float64), ("change", (B, p), torch.float64),
                                                                ("status", (B,), torch.int32))}
    bufs["R"][1].copy_(R)
    bufs["lam"][1].copy_(_gpu(prev))
    row_status = torch.zeros((B, p), dtype=torch.int32, device="cuda")
    rc = lib.ops_frame_modes_ritz_f64(B, p, topo.Nn, X.data_ptr(), MX.data_ptr(), bufs["R"][1].data_ptr(), bufs["Q"][1].data_ptr(),
                                      bufs["lam"][1].data_ptr(), bufs["change"][1].data_ptr(), row_status.data_ptr(),
                                      bufs["status"][1].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _cabi.OK and all(_guards_intact(*v) for v in bufs.values())
    q, r, lam, change = (bufs[k][1].cpu().numpy() for k in ("Q", "R", "lam", "change"))
    assert not bufs["status"][1].any()
    e_lam = e_orth = e_r = 0.0
    for b in range(B):
        M = _dense_M(key, b)
        e_lam = max(e_lam, float(np.abs(lam[b] / its[b][1][0] - 1.0).max()))
        e_orth = max(e_orth, float(np.abs(q[b] @ M @ q[b].T - np.eye(p)).max()))
        e_r = max(e_r, float(np.linalg.norm(r[b] - q[b] @ M.T) / np.linalg.norm(r[b])))
    print(f"{key} p {p}: Ritz values {e_lam:.2e} orthonormality {e_orth:.2e} next R {e_r:.2e}")
    assert e_lam <= 1e-8 and e_orth <= 1e-10 and e_r <= 1e-12
    assert np.array_equal(change, np.abs(lam - prev) / lam)


@functools.lru_cache(maxsize=None)
def _converged(key):
    import openpystruct_amd as pkg
    topo, mass, I = _setup(key)
    fac = pkg.frame_factor(topo, I)
    return fac, pkg.frame_modes(fac, mass, n_modes=2, n_vectors=fr.CASES[key][4], iters=fr.ITERS)


def _m_norm(M, v):
    return float(np.sqrt(v @ M @ v))


@pytest.mark.parametrize("key", KEYS)
def test_converged_run_matches_the_dense_eigenpairs(oa, key):
    """n_modes = 2, n_vectors = min(8, allowed), iters = 16: eigenvalues against dense eigh relative <= 1e-8, shapes (up to sign) in the
    M-norm <= 1e-8 / min(1, gap) where the mode's gap to both neighbours is at least 0.25 (mode 1: always), shapes^T M shapes = I to
    1e-10, status zero, frequencies == sqrt(eigenvalues) / 2 pi.
    Measured: eigenvalues at most 1.9e-13 (3x6-l), shapes 2.7e-12 (general-c), orthonormality 5.6e-16."""
    topo, mass, I = _setup(key)
    ref = fr.reference(key)
    _, r = _converged(key)
    B = I.shape[0]
    assert r.iterations == fr.ITERS and int(r.status.abs().sum()) == 0 and r.status.dtype == torch.int32
    assert r.eigenvalues.shape == r.frequencies.shape == r.change.shape == (B, 2) and r.shapes.shape == (B, 2, topo.Nn, 3)
    assert _same(r.frequencies, torch.sqrt(r.eigenvalues) / (2.0 * math.pi))
    lam, phi = r.eigenvalues.cpu().numpy(), r.shapes.cpu().numpy().reshape(B, 2, -1)
    assert not phi[:, :, np.asarray(topo.fix3).reshape(-1)].any()
    e_lam = e_phi = e_orth = 0.0
    for b in range(B):
        M = ref[b]["M"]
        e_lam = max(e_lam, float(np.abs(lam[b] / ref[b]["lam"][:2] - 1.0).max()))
        e_orth = max(e_orth, float(np.abs(phi[b] @ M @ phi[b].T - np.eye(2)).max()))
        for j in (0, 1):
            gap = fr.gap(ref[b]["lam"], j)
            if j == 0 or gap >= fr.GAP:
                err = min(_m_norm(M, phi[b, j] - ref[b]["phi"][j]), _m_norm(M, phi[b, j] + ref[b]["phi"][j]))
                e_phi = max(e_phi, err * min(1.0, gap))
                lead = phi[b, j][np.abs(phi[b, j]).argmax()]
                assert lead > 0.0
    print(f"{key}: eigenvalues {e_lam:.2e} shapes x min(1, gap) {e_phi:.2e} orthonormality {e_orth:.2e}")
    assert e_lam <= 1e-8 and e_phi <= 1e-8 and e_orth <= 1e-10


@pytest.mark.parametrize("key", ["1x1-c", "3x6-l", "10x4n-c", "general-c", "hub-c"])
def test_vjp_and_autograd_match_the_reference_gradient(oa, key):
    """`frame_modes_vjp` on the converged run and autograd of `differentiable_frame_frequencies` against g . dlambda/dI of the dense
    eigenvectors, norm-wise relative <= max(1e-8, 4e-16 kappa) / min(1, gap), kappa = frame_dense.cond_free; the cotangent of mode 2 is
    zero in a frame where its gap to a neighbour is below 0.25.
    Measured: at most 1.6e-4 of the bound (general-c), through the eigenvalues and through the frequencies."""
    topo, mass, I = _setup(key)
    case, In = fr.inputs(key)[:2]
    ref = fr.reference(key)
    fac, r = _converged(key)
    B = I.shape[0]
    g = fr.grad_cotangent(key).copy()
    gaps = np.ones(B)
    for b in range(B):
        if fr.gap(ref[b]["lam"], 1) < fr.GAP:
            g[b, 1] = 0.0
            gaps[b] = min(1.0, fr.gap(ref[b]["lam"], 0))
        else:
            gaps[b] = min(1.0, fr.gap(ref[b]["lam"], 0), fr.gap(ref[b]["lam"], 1))
    gI = oa.frame_modes_vjp(fac, r, _gpu(g))
    assert gI.shape == (B, topo.Ne)
    Ig = I.clone().requires_grad_(True)
    eig, freq = oa.differentiable_frame_frequencies(topo, Ig, mass, n_modes=2, n_vectors=fr.CASES[key][4], iters=fr.ITERS)
    assert _same(freq.detach(), torch.sqrt(eig.detach()) / (2.0 * math.pi))
    (eig * _gpu(g)).sum().backward()
    if topo.Ne <= 64:                                  # another factorisation: the same bits up to 64 elements (the module's docstring)
        assert _same(eig.detach(), r.eigenvalues) and _same(Ig.grad, gI)
    # through the frequencies: d f / d lambda = 1 / (4 pi sqrt(lambda))
    Ig2 = I.clone().requires_grad_(True)
    _, f2 = oa.differentiable_frame_frequencies(topo, Ig2, mass, n_modes=2, n_vectors=fr.CASES[key][4], iters=fr.ITERS)
    (f2 * _gpu(g)).sum().backward()
    got, got_a, got_f = gI.cpu().numpy(), Ig.grad.cpu().numpy(), Ig2.grad.cpu().numpy()
    worst = worst_f = 0.0
    for b in range(B):                                     # every frame: the last wave's tail included
        tol = max(1e-8, 4e-16 * fd.cond_free(case, In[b])) / gaps[b]
        want = g[b] @ ref[b]["dl"]
        want_f = (g[b] / (4.0 * math.pi * np.sqrt(ref[b]["lam"][:2]))) @ ref[b]["dl"]
        e, e_f = np.linalg.norm(got[b] - want) / np.linalg.norm(want), np.linalg.norm(got_f[b] - want_f) / np.linalg.norm(want_f)
        e = max(e, np.linalg.norm(got_a[b] - want) / np.linalg.norm(want))
        worst, worst_f = max(worst, e / tol), max(worst_f, e_f / tol)
    print(f"{key}: gradient error / bound: eigenvalues {worst:.3e} frequencies {worst_f:.3e}")
    assert worst <= 1.0 and worst_f <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# bits, independence, failures
# ---------------------------------------------------------------------------------------------------------------------
def _same_modes(a, b):
    return all(_same(p, q) for p, q in zip((a.eigenvalues, a.frequencies, a.shapes, a.change, a.status), (b.eigenvalues, b.frequencies, b.shapes, b.change, b.status)))


def test_a_frame_alone_equals_the_frame_in_a_batch_of_67_and_two_runs_are_equal(oa):
    """general-l (12 elements, B = 67): frames 0, 33 and 66 solved alone (another factorisation, another grid) bit for bit; the same
    call twice on one factor bit for bit, with nothing allocated by the second call beyond its results."""
    topo, mass, I = _setup("general-l")
    fac, r = _converged("general-l")
    for b in (0, 33, 66):
        alone = oa.frame_solve_modes(topo, I[b:b + 1].contiguous(), mass, n_modes=2, n_vectors=8, iters=fr.ITERS)
        assert _same_modes(alone, oa.FrameModes(*(t[b:b + 1] if torch.is_tensor(t) else t for t in r))), b
    again = oa.frame_modes(fac, mass, n_modes=2, n_vectors=8, iters=fr.ITERS)
    assert _same_modes(again, r)
    del again
    torch.cuda.synchronize()
    before, kept = torch.cuda.memory_allocated(), len(fac._scratch)
    third = oa.frame_modes(fac, mass, n_modes=2, n_vectors=8, iters=fr.ITERS)
    del third
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and len(fac._scratch) == kept


def test_per_frame_nodal_mass_follows_its_frame(oa):
    """general-c (per-frame nodal masses, B = 5): frames 3 and 1 as a batch of two with their own masses, bit for bit."""
    topo, mass, I = _setup("general-c")
    _, r = _converged("general-c")
    pick = [3, 1]
    _, _, mbar, nodal, kind, p = fr.inputs("general-c")
    sub = oa.frame_solve_modes(topo, I[pick].contiguous(), oa.FrameMass(topo, mbar, nodal[pick], kind=kind), n_modes=2, n_vectors=p, iters=fr.ITERS)
    assert _same_modes(sub, oa.FrameModes(*(t[pick] if torch.is_tensor(t) else t for t in r)))


def test_a_failed_factorisation_is_nan_with_status_1_for_that_frame_alone(oa):
    """The failing inertias of tests/test_gpu_frame_cases.py (a status path: nothing is provoked on the device)."""
    from openpystruct_amd import frames
    topo = frames.grid_frame(4, 2)
    rng = np.random.default_rng(12)
    I = fd.random_inertias(rng, 12, topo.Ne)
    mass = oa.FrameMass(topo, fr.MBAR, np.full((topo.Nn, 3), fr.NODAL))
    healthy = oa.frame_solve_modes(topo, _gpu(I), mass, n_modes=2, iters=6)
    assert int(healthy.status.abs().sum()) == 0
    Ib = I.copy()
    Ib[2, 3] = -0.1
    Ib[7, :] = 0.0
    bad, good = [2, 7], [b for b in range(12) if b not in (2, 7)]
    fac = oa.frame_factor(topo, _gpu(Ib))
    r = oa.frame_modes(fac, mass, n_modes=2, iters=6)
    assert bool((r.status[bad] == 1).all()) and bool((r.status[good] == 0).all())
    for name in ("eigenvalues", "frequencies", "shapes", "change"):
        t = getattr(r, name)
        assert bool(torch.isnan(t[bad]).all()) and _same(t[good], getattr(healthy, name)[good]), name
    gI = oa.frame_modes_vjp(fac, r, torch.ones((12, 2), dtype=torch.float64, device="cuda"))
    assert bool(torch.isnan(gI[bad]).all()) and bool(torch.isfinite(gI[good]).all())


def test_more_vectors_than_dofs_with_mass_is_nan_with_status_2_for_that_frame_alone(oa):
    """Lumped mass on the 1 x 1 frame, six vectors: frame 3 has no nodal mass, so four of its DOFs carry mass and X^T M X is singular;
    the others have a rotational nodal mass.  The start is the six unit vectors of the free DOFs (as many default start vectors as
    equations are numerically dependent after one solve)."""
    from openpystruct_amd import frames
    topo = frames.grid_frame(1, 1)
    I = _gpu(fd.random_inertias(np.random.default_rng(4), 5, topo.Ne))
    nodal = np.tile(np.array([fr.NODAL, fr.NODAL, 50.0]), (5, topo.Nn, 1))
    nodal[3] = 0.0
    X0 = np.zeros((6, topo.Nn * 3))
    X0[np.arange(6), np.nonzero(~topo.fix3.reshape(-1))[0]] = 1.0
    X0 = _gpu(X0.reshape(6, topo.Nn, 3))
    r = oa.frame_solve_modes(topo, I, oa.FrameMass(topo, fr.MBAR, nodal, kind="lumped"), n_modes=2, n_vectors=6, iters=4, X0=X0)
    assert r.status.cpu().tolist() == [0, 0, 0, 2, 0]
    good = [0, 1, 2, 4]
    for t in (r.eigenvalues, r.frequencies, r.shapes, r.change):
        assert bool(torch.isnan(t[3]).all()) and bool(torch.isfinite(t[good]).all())
    sub = oa.frame_solve_modes(topo, I[good].contiguous(), oa.FrameMass(topo, fr.MBAR, nodal[good], kind="lumped"), n_modes=2, n_vectors=6,
                               iters=4, X0=X0)
    assert _same_modes(sub, oa.FrameModes(*(t[good] if torch.is_tensor(t) else t for t in r)))
    four = oa.frame_solve_modes(topo, I, oa.FrameMass(topo, fr.MBAR, nodal, kind="lumped"), n_modes=2, n_vectors=4, iters=4)
    assert int(four.status.abs().sum()) == 0                                          # four vectors are served


def test_tol_mode_stops_within_max_iters(oa):
    """3x6-c, two modes, the default six vectors: the loop ends at a multiple of poll_every with change <= tol on both modes.
    Measured: 8 iterations."""
    topo, mass, I = _setup("3x6-c")
    ref = fr.reference("3x6-c")
    r = oa.frame_solve_modes(topo, I, mass, n_modes=2, tol=1e-10, max_iters=64, poll_every=4)
    print(f"iterations {r.iterations} change {r.change.cpu().numpy()}")
    assert 4 <= r.iterations <= 64 and r.iterations % 4 == 0 and int(r.status.abs().sum()) == 0
    assert bool((r.change <= 1e-10).all())
    assert float(np.abs(r.eigenvalues.cpu().numpy()[0] / ref[0]["lam"][:2] - 1.0).max()) <= 1e-8
    capped = oa.frame_solve_modes(topo, I, mass, n_modes=2, tol=1e-300, max_iters=5, poll_every=2)
    assert capped.iterations == 5


def test_shim_eigen_equals_frame_solve_modes(oa):
    """`ops.eigen(2)` on the recorded 2 x 3 frame against `frame_solve_modes` on `grid_frame(2, 3)`, bit for bit."""
    from openpystruct_amd import frames, ops
    cfg = frames.FrameConfig()
    topo = frames.grid_frame(2, 3, cfg)
    rng = np.random.default_rng(23)
    I = fd.random_inertias(rng, 1, topo.Ne)
    mbar = fr.MBAR * rng.uniform(0.5, 2.0, size=topo.Ne)
    nodal = np.zeros((topo.Nn, 3))
    nodal[3:] = (fr.NODAL, fr.NODAL, 50.0)
    want = oa.frame_solve_modes(topo, _gpu(I), oa.FrameMass(topo, mbar, nodal, kind="consistent"), n_modes=2)
    ops.wipe()
    ops.model("basic", "-ndm", 2, "-ndf", 3)
    for n, (x, y) in enumerate(topo.coords, start=1):
        ops.node(n, x, y)
        if y == 0.0:
            ops.fix(n, 1, 1, 1)
        else:
            ops.mass(n, fr.NODAL, fr.NODAL, 50.0)
    ops.geomTransf("Linear", 1)
    for e, (a, b) in enumerate(topo.conn, start=1):
        ops.element("elasticBeamColumn", e, int(a) + 1, int(b) + 1, cfg.A, cfg.E, float(I[0, e - 1]), 1, "-mass", float(mbar[e - 1]), "-cMass")
    lam = ops.eigen("-genBandArpack", 2)
    assert lam == [float(v) for v in want.eigenvalues[0].cpu().numpy()]
    shapes = want.shapes[0].cpu().numpy()
    for n in (4, topo.Nn):
        assert ops.nodeEigenvector(n, 2) == [float(v) for v in shapes[1, n - 1]]
        assert ops.nodeEigenvector(n, 1, 1) == float(shapes[0, n - 1, 0])
    ops.wipe()
