"""Linear buckling load factors on the kept factorisation, on the GPU: the three kernels behind
`ops_frame_geom_apply_f64`, `ops_frame_buckling_ritz_f64` and `ops_frame_buckling_grad_f64` (csrc/frame_loads.hip, arithmetic
csrc/frame_buckling.hpp) and `frame_buckling` / `frame_solve_buckling` / `frame_buckling_vjp` / `differentiable_frame_buckling` --
against the dense float64 reference of tests/frame_buckling_ref.py, whose cases (topology, batch, kind, load state, vectors) and
constants this file shares with tests/test_frame_buckling_host.py.

Bit-for-bit comparisons between two FACTORISATIONS use frames of at most 64 elements (tests/test_gpu_frame_cases.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import frame_buckling_ref as br  # noqa: E402
from tests import frame_dense as fd  # noqa: E402
from tests.test_gpu_frame_cases import _same  # noqa: E402
from tests.test_gpu_frame_grad import _gpu, _tuned_kernels_for_every_batch, oa  # noqa: E402,F401
from tests.test_gpu_frame_modes import _guarded, _guards_intact  # noqa: E402

KEYS = list(br.CASES)


@functools.lru_cache(maxsize=None)
def _setup(key):
    """(topology, I on the device, factor, reference FrameSolution | None) of a shared case: None is the factor's own keeping solution,
    otherwise case 0 of a `frame_resolve` under the case's per-frame nodal loads and the topology's element loads."""
    import openpystruct_amd as pkg
    from openpystruct_amd import frames
    case, I, loads, kind, p = br.inputs(key)
    topo = br.topology(br.CASES[key][0], "cuda")
    Ig = _gpu(I)
    fac = pkg.frame_factor(topo, Ig)
    reference = None
    if loads is not None:
        s = pkg.frame_resolve(fac, _gpu(loads[:, None]))
        reference = frames.FrameSolution(s.disp[:, 0].contiguous(), s.forces[:, 0].contiguous(), s.V[:, 0].contiguous(),
                                         s.M[:, 0].contiguous(), s.status[:, 0].contiguous())
    return topo, Ig, fac, reference


def _run(pkg, key, **kw):
    topo, I, fac, reference = _setup(key)
    return pkg.frame_buckling(fac, reference=reference, kind=br.CASES[key][2], **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the streaming entries alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_geometric_apply_alone_matches_the_dense_matrix(oa, key):
    """Fed the dense reference's end forces: elementwise |got - ref| <= c 2^-52 (|S| |x|), |S| the sum of the absolute terms of S (the
    four terms of every axial force included), c = tests/frame_buckling_ref.py::C_GEOM = 4 x 2.02 = 8.08: four times the largest
    ratio the g++ build of csrc/frame_buckling.hpp shows on these inputs (tests/test_frame_buckling_host.py pins it); never taken
    from the device.  Three rows per frame, B = 1, 5 and 67; the output between guard regions.
    Measured on the device: ratio at most 2.13 (10x4n-c)."""
    from openpystruct_amd import _cabi, frames
    lib = _cabi.load()
    topo, I, _, _ = _setup(key)
    ref = br.reference(key)
    B = I.shape[0]
    x = br.geom_apply_x(key)
    xg, fg = _gpu(x), _gpu(np.stack([r["forces"] for r in ref]))
    whole, y = _guarded((B * 3, topo.Nn, 3))
    adj = frames._adjoint_tables(topo)
    rc = lib.ops_frame_geom_apply_f64(B * 3, 3, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), adj.conn.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(),
                                      fg.data_ptr(), int(br.CASES[key][2] == "consistent"), xg.data_ptr(), y.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _cabi.OK and _guards_intact(whole, y)
    got = y.cpu().numpy().reshape(B, 3, -1)
    worst = 0.0
    for b in range(B):
        want, scale = x[b] @ ref[b]["S"].T, np.abs(x[b]) @ ref[b]["Sabs"].T
        assert np.all(got[b][scale == 0] == 0.0)
        worst = max(worst, float((np.abs(got[b] - want)[scale > 0] / (br.EPS * scale[scale > 0])).max()))
    print(f"geometric apply {key}: largest ratio {worst:.3f} (bound {br.C_GEOM})")
    assert worst <= br.C_GEOM


@pytest.mark.parametrize("key", KEYS)
def test_gradient_entry_alone_matches_the_reference(oa, key):
    """Fed the reference's phi and lambda: the direct term and the six cotangents of the end forces, |got - ref| <= c 2^-52 times the
    sum of the absolute terms, c = C_BGRAD = 4 x 3.68 = 14.72, four times the host's largest ratio; a frame with a non-zero status
    gets NaN rows; both outputs between guard regions.  Measured on the device: ratio at most 3.29 (10x4n-c)."""
    from openpystruct_amd import _cabi, frames
    lib = _cabi.load()
    topo, I, _, _ = _setup(key)
    case, kind = br.inputs(key)[0], br.CASES[key][2]
    ref = br.reference(key)
    B = I.shape[0]
    phi, lam, g = np.stack([r["phi"] for r in ref]), np.stack([r["lam"][:2] for r in ref]), br.grad_cotangent(key)
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    if B > 1:
        status[B - 1] = 3
    (w_d, gI), (w_f, gf) = _guarded((B, topo.Ne)), _guarded((B, topo.Ne, 6))
    adj = frames._adjoint_tables(topo)
    phi_g, lam_g, g_g = _gpu(phi), _gpu(lam), _gpu(g)
    rc = lib.ops_frame_buckling_grad_f64(B, 2, 2, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(),
                                         int(kind == "consistent"), phi_g.data_ptr(), lam_g.data_ptr(), g_g.data_ptr(), status.data_ptr(),
                                         gI.data_ptr(), gf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _cabi.OK and _guards_intact(w_d, gI) and _guards_intact(w_f, gf)
    got = np.concatenate([gI.cpu().numpy()[..., None], gf.cpu().numpy()], axis=2)
    worst = 0.0
    for b in range(B - (B > 1)):
        d, f, sd, sf = br.grad_rows(case, kind, phi[b], lam[b], g[b])
        want, scale = np.concatenate([d[:, None], f], 1), np.concatenate([sd[:, None], sf], 1)
        assert np.all(got[b][scale == 0] == 0.0)
        worst = max(worst, float((np.abs(got[b] - want)[scale > 0] / (br.EPS * scale[scale > 0])).max()))
    print(f"gradient rows {key}: largest ratio {worst:.3f} (bound {br.C_BGRAD})")
    assert worst <= br.C_BGRAD and (B == 1 or np.isnan(got[B - 1]).all())


@pytest.mark.parametrize("key", ["1x1-c", "10x4n-c", "hub-p"])
def test_ritz_entry_alone_between_guard_regions(oa, key):
    """`ops_frame_buckling_ritz_f64` by itself, every output between sentinel-filled guard regions, fed X, SX and R of the reference's
    second iteration on the case's vectors: 1x1 (12 entries per vector: fewer than a wave, three vectors), hub (57 entries, eight) and
    10x4n (165 entries, eight) with B = 5, 5 and 67 frames -- none a multiple of the four frames of a block.  Ritz values <= 1e-8 of
    the step's largest |mu| against the reference's (the host measures 7.2e-14 for this arithmetic: below 1e-10, so the project's
    1e-8), descending; lambda = 1 / mu where mu > 0, else +inf, bit for bit; Q^T K Q = I to 1e-10; the next R = S Q; change against the
    values `mu` held, bit for bit; status zero; nothing outside the outputs written.
    Measured: Ritz values 3.7e-15, orthonormality 6.0e-14, the next R 3.6e-16."""
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    topo, I, _, _ = _setup(key)
    case, In = br.inputs(key)[:2]
    ref = br.reference(key)
    p = br.CASES[key][4]
    B, n = I.shape[0], 3 * topo.Nn
    assert B % 4 != 0
    X, SX, R = (_gpu(np.stack([r["its"][1][k] for r in ref])) for k in (3, 4, 5))
    prev = np.stack([r["its"][0][0] for r in ref])
    bufs = {name: _guarded(shape, dt) for name, shape, dt in (("R", (B, p, n), torch.float64), ("Q", (B, p, n), torch.float64),
                                                                ("mu", (B, p), torch.float64), ("lam", (B, p), torch.float64),
                                                                ("change", (B, p), torch.float64), ("status", (B,), torch.int32))}
    bufs["R"][1].copy_(R)
    bufs["mu"][1].copy_(_gpu(prev))
    row_status = torch.zeros((B, p), dtype=torch.int32, device="cuda")
    rc = lib.ops_frame_buckling_ritz_f64(B, p, topo.Nn, X.data_ptr(), SX.data_ptr(), bufs["R"][1].data_ptr(), bufs["Q"][1].data_ptr(),
                                         bufs["mu"][1].data_ptr(), bufs["lam"][1].data_ptr(), bufs["change"][1].data_ptr(),
                                         row_status.data_ptr(), bufs["status"][1].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _cabi.OK and all(_guards_intact(*v) for v in bufs.values())
    q, r, mu, lam, change = (bufs[k][1].cpu().numpy() for k in ("Q", "R", "mu", "lam", "change"))
    assert not bufs["status"][1].any()
    e_mu = e_orth = e_r = 0.0
    for b in range(B):
        want = ref[b]["its"][1][0]
        e_mu = max(e_mu, float(np.abs(mu[b] - want).max() / np.abs(want).max()))
        e_orth = max(e_orth, float(np.abs(q[b] @ br.dense_K(case, In[b]) @ q[b].T - np.eye(p)).max()))
        e_r = max(e_r, float(np.linalg.norm(r[b] - q[b] @ ref[b]["S"].T) / np.linalg.norm(r[b])))
    print(f"{key} p {p}: Ritz values {e_mu:.2e} orthonormality {e_orth:.2e} next R {e_r:.2e}")
    assert e_mu <= 1e-8 and e_orth <= 1e-10 and e_r <= 1e-12 and np.all(np.diff(mu, axis=1) <= 0.0)
    assert np.array_equal(lam, br.load_factors(mu)) and np.array_equal(change, np.abs(mu - prev) / np.abs(mu))


# ---------------------------------------------------------------------------------------------------------------------
# the iteration
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("key", KEYS)
def test_ritz_values_after_one_two_and_three_iterations(oa, key, p):
    """From the default start, all p Ritz values against the NumPy restatement of the iteration, <= 1e-8 of the step's largest |mu|
    (the host measures the g++ build against the restatement at 7.2e-14: below 1e-10, so the project's bound for this arithmetic,
    the one tests/test_gpu_frame_cases.py::_assert_rows holds the re-solve's displacements to).  On the 1 x 1 frame more than three
    vectors stand for three (tests/frame_buckling_ref.py: cond(X^T K X) is 1.7e9 with five).  On 10x4n-c the first eight of the 67 frames
    are compared (the restatement costs a dense factorisation per frame and vector count; every frame runs).
    Measured: at most 1.1e-12 (hub-p, one vector, second iteration), 2.9e-13 elsewhere."""
    topo, I, fac, reference = _setup(key)
    case, In = br.inputs(key)[:2]
    ref = br.reference(key)
    p = min(p, 3) if key.startswith("1x1") else p
    frames_ = range(min(I.shape[0], 8))
    want = np.stack([[it[0] for it in br.iterate(case, In[b], ref[b]["S"], br.default_start(case, p), 3)] for b in frames_])     # [F,3,p]
    worst = []
    for t in (1, 2, 3):
        r = _run(oa, key, n_modes=p, n_vectors=p, iters=t)
        assert r.iterations == t and int(r.status.abs().sum()) == 0 and r.mu.shape == r.load_factors.shape == (I.shape[0], p)
        mu = r.mu.cpu().numpy()
        worst.append(float((np.abs(mu[:len(frames_)] - want[:, t - 1]).max(axis=1) / np.abs(want[:, t - 1]).max(axis=1)).max()))
        assert np.array_equal(r.load_factors.cpu().numpy(), br.load_factors(mu))
        assert bool(torch.isinf(r.change).all()) == (t == 1)
    print(f"{key} p {p}: Ritz values after 1, 2, 3 iterations {worst[0]:.2e} {worst[1]:.2e} {worst[2]:.2e}")
    assert max(worst) <= 1e-8


@functools.lru_cache(maxsize=None)
def _converged(key):
    import openpystruct_amd as pkg
    return _run(pkg, key, n_modes=2, n_vectors=br.CASES[key][4], iters=br.ITERS)


@pytest.mark.parametrize("key", KEYS)
def test_converged_run_matches_the_dense_eigenpairs(oa, key):
    """n_modes = 2, the case's vectors, iters = 16: mu and lambda against dense eigh relative <= 1e-8 (the NumPy restatement is within
    2.0e-15 of dense after 16 iterations: below 1e-10); shapes (up to sign) in the K-norm <= bound / min(1, gap), mode 2 where its gap
    to both neighbours is at least 0.25, bound = tests/frame_buckling_ref.py::shape_bound: 1e-8 where the restatement's own shapes are
    within 1e-10 of dense after 16 iterations, else 100 x what it shows (3x6-c: 1.2e-7, 10x4n-c: 1.2e-6; the ten-bay frame's second
    shape converges at |mu_9| / mu_2 = 0.31 per iteration whatever the inertias); shapes^T K shapes = I and shapes^T S shapes =
    diag(mu) to 1e-10; status zero; the component of largest magnitude positive.
    Measured: mu and lambda at most 1.0e-13 (hub-p); shapes 5.4e-14 where the bound is 1e-8, 1.13e-9 on 3x6-c and 1.09e-8 on 10x4n-c (the
    restatement's figures to three digits); K-orthonormality 8.8e-14, S 3.1e-14."""
    topo, I, fac, reference = _setup(key)
    case, In = br.inputs(key)[:2]
    ref = br.reference(key)
    r = _converged(key)
    B = I.shape[0]
    assert r.iterations == br.ITERS and int(r.status.abs().sum()) == 0 and r.status.dtype == torch.int32 and r.kind == br.CASES[key][2]
    assert r.load_factors.shape == r.mu.shape == r.change.shape == (B, 2) and r.shapes.shape == (B, 2, topo.Nn, 3)
    assert r.reference is (fac.solution if reference is None else r.reference)
    mu, lam, phi = r.mu.cpu().numpy(), r.load_factors.cpu().numpy(), r.shapes.cpu().numpy().reshape(B, 2, -1)
    assert not phi[:, :, np.asarray(topo.fix3).reshape(-1)].any()
    e_mu = e_lam = e_phi = e_orth = e_s = 0.0
    for b in range(B):
        K = br.dense_K(case, In[b])
        e_mu = max(e_mu, float(np.abs(mu[b] / ref[b]["mu"][:2] - 1.0).max()))
        e_lam = max(e_lam, float(np.abs(lam[b] / ref[b]["lam"][:2] - 1.0).max()))
        e_orth = max(e_orth, float(np.abs(phi[b] @ K @ phi[b].T - np.eye(2)).max()))
        e_s = max(e_s, float((np.abs(phi[b] @ ref[b]["S"] @ phi[b].T - np.diag(mu[b])) / np.abs(mu[b]).max()).max()))
        for j in (0, 1):
            gap = br.gap(ref[b]["mu"], j)
            if j == 0 or gap >= br.GAP:
                e_phi = max(e_phi, br.shape_error(K, phi[b, j], ref[b]["phi"][j]) * min(1.0, gap))
                assert phi[b, j][np.abs(phi[b, j]).argmax()] > 0.0
    print(f"{key}: mu {e_mu:.2e} lambda {e_lam:.2e} shapes x min(1, gap) {e_phi:.2e} (bound {br.shape_bound(key):.1e}) K-orthonormality {e_orth:.2e} S {e_s:.2e}")
    assert e_mu <= 1e-8 and e_lam <= 1e-8 and e_phi <= br.shape_bound(key) and e_orth <= 1e-10 and e_s <= 1e-10


def _gradient_errors(key, got):
    """Largest norm-wise error / bound over tests/frame_buckling_ref.py::gradient_frames, bound = max(1e-8, 4e-16 kappa) / min(1, gap)."""
    case, In = br.inputs(key)[:2]
    want, _, gaps = br.reference_gradient(key)
    worst = 0.0
    for k, b in enumerate(br.gradient_frames(key)):
        tol = max(1e-8, 4e-16 * fd.cond_free(case, In[b])) / gaps[k]
        worst = max(worst, float(np.linalg.norm(got[b] - want[k]) / np.linalg.norm(want[k])) / tol)
    return worst


@pytest.mark.parametrize("key", KEYS)
def test_vjp_matches_the_reference_gradient_and_the_homogeneity_identity(oa, key):
    """`frame_buckling_vjp` on the converged run against autograd of the dense model through eigvalsh (tests/frame_buckling_ref.py, which
    knows nothing of the adjoint formula), norm-wise relative <= max(1e-8, 4e-16 kappa) / min(1, gap), kappa = frame_dense.cond_free; the
    cotangent of mode 2 is zero in a frame where its gap to a neighbour is below 0.25.  Compared on gradient_frames(key): every frame
    up to eight, six of the 67 (first, middle, last: autograd of the dense model costs a dense solve and an eigh each).
    Then the homogeneity identity with the cotangent e_1: lambda_1 is homogeneous of degree -1 in the reference's loads, so
    sum loads . g_loads + sum w . g_element_loads = -lambda_1, held to the same bound relative to the sum of the absolute terms.
    Measured, error / bound: gradient 0.67 on 10x4n-c and 0.049 on 3x6-c (the truncation of 16 iterations on the second shape: the
    restatement shows the same on the CPU), at most 5.9e-6 elsewhere; homogeneity at most 1.2e-6."""
    topo, I, fac, reference = _setup(key)
    case, In, loads = br.inputs(key)[:3]
    r = _converged(key)
    B = I.shape[0]
    _, g, gaps = br.reference_gradient(key)
    gI, g_loads, g_w = oa.frame_buckling_vjp(fac, r, _gpu(g))
    assert gI.shape == (B, topo.Ne) and g_loads.shape == (B, topo.Nn, 3) and g_w.shape == (B, topo.Ne, 2)
    worst = _gradient_errors(key, gI.cpu().numpy())
    e1 = np.zeros((B, 2)); e1[:, 0] = 1.0
    _, h_loads, h_w = oa.frame_buckling_vjp(fac, r, _gpu(e1))
    h_loads, h_w, lam = h_loads.cpu().numpy(), h_w.cpu().numpy(), r.load_factors.cpu().numpy()[:, 0]
    f = np.broadcast_to(case.nodal_loads if loads is None else loads, (B, topo.Nn, 3))
    w = np.stack([case.wy, case.wx], axis=1)[None]
    worst_h = 0.0
    for k, b in enumerate(br.gradient_frames(key)):
        terms = np.concatenate([(f[b] * h_loads[b]).ravel(), (w[0] * h_w[b]).ravel()])
        tol = max(1e-8, 4e-16 * fd.cond_free(case, In[b])) / min(1.0, br.gap(br.reference(key)[b]["mu"], 0))
        worst_h = max(worst_h, abs(terms.sum() + lam[b]) / np.abs(terms).sum() / tol)
    print(f"{key}: gradient error / bound {worst:.3e}, homogeneity defect / bound {worst_h:.3e}")
    assert worst <= 1.0 and worst_h <= 1.0


@pytest.mark.parametrize("key", ["1x1-c", "3x6-p", "3x6-c", "10x4n-c", "hub-p"])
def test_autograd_of_the_operator_matches_the_reference_gradient(oa, key):
    """`differentiable_frame_buckling` (the topology's own loads: every shared case but general-c, whose reference is a `frame_resolve`
    case) against the same reference gradient and bound; up to 64 elements the load factors and the gradient equal those of
    `frame_buckling` / `frame_buckling_vjp` on another factorisation bit for bit.  Measured: the figures of the test above."""
    topo, I, fac, _ = _setup(key)
    r = _converged(key)
    _, g, _ = br.reference_gradient(key)
    Ig = I.clone().requires_grad_(True)
    lam = oa.differentiable_frame_buckling(topo, Ig, n_modes=2, kind=br.CASES[key][2], n_vectors=br.CASES[key][4], iters=br.ITERS)
    (lam * _gpu(g)).sum().backward()
    if topo.Ne <= 64:
        assert _same(lam.detach(), r.load_factors) and _same(Ig.grad, oa.frame_buckling_vjp(fac, r, _gpu(g))[0])
    worst = _gradient_errors(key, Ig.grad.cpu().numpy())
    print(f"{key}: autograd error / bound {worst:.3e}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# bits, independence, failures
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ("load_factors", "mu", "shapes", "change", "status")


def _same_result(a, b, rows=None):
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    return all(_same(getattr(a, k), pick(getattr(b, k))) for k in FIELDS)


def test_a_frame_alone_equals_the_frame_in_a_batch_of_67_and_two_runs_are_equal(oa):
    """The general topology (12 elements), B = 67, its own loads, eight vectors, six iterations: frames 0, 33 and 66 solved alone
    (another factorisation, another grid) bit for bit; the same call twice on one factor bit for bit, with nothing allocated by the
    later calls beyond their results."""
    topo = br.topology("general", "cuda")
    I = _gpu(fd.random_inertias(np.random.default_rng(67), 67, topo.Ne))
    fac = oa.frame_factor(topo, I)
    r = oa.frame_buckling(fac, n_modes=2, n_vectors=8, iters=6)
    assert int(r.status.abs().sum()) == 0
    for b in (0, 33, 66):
        alone = oa.frame_solve_buckling(topo, I[b:b + 1].contiguous(), n_modes=2, n_vectors=8, iters=6)
        assert _same_result(alone, r, slice(b, b + 1)), b
    again = oa.frame_buckling(fac, n_modes=2, n_vectors=8, iters=6)
    assert _same_result(again, r)
    del again
    torch.cuda.synchronize()
    before, kept = torch.cuda.memory_allocated(), len(fac._scratch)
    third = oa.frame_buckling(fac, n_modes=2, n_vectors=8, iters=6)
    del third
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and len(fac._scratch) == kept


def test_a_failed_factorisation_is_nan_with_status_1_for_that_frame_alone(oa):
    """The failing inertias of tests/test_gpu_frame_cases.py (a status path: nothing is provoked on the device)."""
    from openpystruct_amd import frames
    topo = frames.grid_frame(4, 2)
    I = fd.random_inertias(np.random.default_rng(12), 12, topo.Ne)
    healthy = oa.frame_solve_buckling(topo, _gpu(I), n_modes=2, iters=6)
    assert int(healthy.status.abs().sum()) == 0
    Ib = I.copy()
    Ib[2, 3] = -0.1
    Ib[7, :] = 0.0
    bad, good = [2, 7], [b for b in range(12) if b not in (2, 7)]
    fac = oa.frame_factor(topo, _gpu(Ib))
    r = oa.frame_buckling(fac, n_modes=2, iters=6)
    assert bool((r.status[bad] == 1).all()) and bool((r.status[good] == 0).all())
    for name in FIELDS[:-1]:
        t = getattr(r, name)
        assert bool(torch.isnan(t[bad]).all()) and _same(t[good], getattr(healthy, name)[good]), name
    gI, g_loads, g_w = oa.frame_buckling_vjp(fac, r, torch.ones((12, 2), dtype=torch.float64, device="cuda"))
    for t in (gI, g_loads, g_w):
        assert bool(torch.isnan(t[bad]).all()) and bool(torch.isfinite(t[good]).all())


def test_more_vectors_than_the_rank_of_s_is_nan_with_status_2(oa):
    """pdelta on the 1 x 1 frame: every element carries one transverse difference, so S has rank three and five vectors (and four)
    make X^T K X singular: status 2 and NaN for every frame of that call, while three vectors on the same factor are served.  Then status 2 for ONE
    frame alone: three vectors, frame 3 with a zero start vector (its row and column of X^T K X are exactly zero), the others
    bit for bit what they are without it."""
    from openpystruct_amd import frames
    import importlib
    topo = frames.grid_frame(1, 1)
    I = _gpu(fd.random_inertias(np.random.default_rng(4), 5, topo.Ne))
    fac = oa.frame_factor(topo, I)
    five = oa.frame_buckling(fac, n_modes=2, kind="pdelta", n_vectors=5, iters=4)
    assert five.status.cpu().tolist() == [2] * 5
    for name in FIELDS[:-1]:
        assert bool(torch.isnan(getattr(five, name)).all()), name
    assert oa.frame_buckling(fac, n_modes=2, kind="pdelta", n_vectors=4, iters=4).status.cpu().tolist() == [2] * 5
    three = oa.frame_buckling(fac, n_modes=2, kind="pdelta", n_vectors=3, iters=4)
    assert int(three.status.abs().sum()) == 0 and all(bool(torch.isfinite(getattr(three, k)).all()) for k in ("mu", "shapes"))
    fm = importlib.import_module("openpystruct_amd.frame_modes")
    X0 = _gpu(np.broadcast_to(fm.default_start(topo, 3), (5, 3, topo.Nn, 3)).copy())
    X0[3, 2] = 0.0
    r = oa.frame_buckling(fac, n_modes=2, kind="pdelta", n_vectors=3, iters=4, X0=X0)
    assert r.status.cpu().tolist() == [0, 0, 0, 2, 0]
    good = [0, 1, 2, 4]
    for name in FIELDS[:-1]:
        assert bool(torch.isnan(getattr(r, name)[3]).all()) and _same(getattr(r, name)[good], getattr(three, name)[good]), name


def test_a_column_in_tension_does_not_buckle(oa):
    """The 4-element column under tip tension: every mu is negative, the load factors are +inf with status 0 and the gradient is zero
    (a mode with lambda = +inf contributes nothing); under tip compression the first load factor is Euler's load to the
    discretisation error the host test measures (+3.3e-5, consistent)."""
    topo = br.column(4, load=+1.0, device="cuda")
    I = torch.full((3, 4), 1e-4, dtype=torch.float64, device="cuda")
    fac = oa.frame_factor(topo, I)
    r = oa.frame_buckling(fac, n_modes=2, iters=8)
    assert int(r.status.abs().sum()) == 0 and bool((r.mu < 0.0).all()) and bool(torch.isinf(r.load_factors).all()) and bool((r.load_factors > 0).all())
    assert bool(torch.isfinite(r.shapes).all())
    for t in oa.frame_buckling_vjp(fac, r, torch.ones((3, 2), dtype=torch.float64, device="cuda")):
        assert bool((t == 0.0).all())
    Ig = I.clone().requires_grad_(True)
    oa.differentiable_frame_buckling(topo, Ig, n_modes=1, iters=8).sum().backward()
    assert bool((Ig.grad == 0.0).all())
    pushed = oa.frame_solve_buckling(br.column(4, load=-1.0, device="cuda"), I, n_modes=1, iters=br.ITERS)
    euler = np.pi ** 2 * 200e9 * 1e-4 / (4 * 4.0 ** 2)
    err = pushed.load_factors.cpu().numpy()[:, 0] / euler - 1.0
    print(f"column: load factor / Euler - 1 = {err}")
    assert np.all((err > 3.0e-5) & (err < 3.6e-5))


def test_tol_mode_stops_at_a_multiple_of_poll_every(oa):
    """3x6-p, two modes, the default six vectors: the loop ends at a multiple of poll_every with change <= tol on both modes.
    Measured: 8 iterations."""
    topo, I, fac, _ = _setup("3x6-p")
    ref = br.reference("3x6-p")
    r = oa.frame_buckling(fac, n_modes=2, kind="pdelta", tol=1e-10, max_iters=64, poll_every=4)
    print(f"iterations {r.iterations} change {r.change.cpu().numpy()}")
    assert 4 <= r.iterations <= 64 and r.iterations % 4 == 0 and int(r.status.abs().sum()) == 0
    assert bool((r.change <= 1e-10).all())
    assert float(np.abs(r.mu.cpu().numpy()[0] / ref[0]["mu"][:2] - 1.0).max()) <= 1e-8
    capped = oa.frame_buckling(fac, n_modes=2, kind="pdelta", tol=1e-300, max_iters=5, poll_every=2)
    assert capped.iterations == 5
