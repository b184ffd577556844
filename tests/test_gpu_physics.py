"""FE-residual operator (HIP), its vector-Jacobian product and the surrogates' fused residual term: against the dense oracle
stiffness matrix on the reference bridge, and against the float64 references of tests/beam_dense.py over the shapes, input
forms and edges the kernels index by."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import beam_oracle as bo  # noqa: E402
from tests.beam_dense import dense_solve, random_case, residual_ref, residual_term_ref, residual_vjp_scales  # noqa: E402
from tests.helpers import FAT_P, TILINGS  # noqa: E402


def _case(B=5, seed=0):
    rng = np.random.default_rng(seed)
    x = np.linspace(0, 200, 101)
    fix = bo.reference_fix_mask()
    I, Fy = bo.random_cases(rng, B, inertia="trajectory")
    return x, fix, I, Fy


def test_residual_vanishes_at_the_fe_solution_and_matches_dense_K():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    import openpystruct_amd as oa
    from openpystruct_amd import physics
    x, fix, I, Fy = _case()
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device="cuda")  # noqa: E731
    sol = oa.beam_solve(t(x), t(bo.E_REF), t(I), t(fix, torch.uint8), t(Fy), t(bo.UDL_REF))
    rv, rt = physics.fe_residual(t(I), sol.v, sol.theta, t(x), t(bo.E_REF), t(fix, torch.uint8), t(Fy), t(bo.UDL_REF))
    fmax = float(np.abs(Fy).max())
    assert float(rv.abs().max()) < 1e-6 * fmax and float(rt.abs().max()) < 1e-6 * fmax      # equilibrium
    # arbitrary displacement field: compare with the dense oracle K u - f on the free DOFs
    rng = np.random.default_rng(1)
    v = rng.normal(size=Fy.shape) * 1e-2; th = rng.normal(size=Fy.shape) * 1e-3
    rv, rt = physics.fe_residual(t(I), t(v), t(th), t(x), t(bo.E_REF), t(fix, torch.uint8), t(Fy), t(bo.UDL_REF))
    for b in range(I.shape[0]):
        K, f = bo.assemble_beam(x, bo.E_REF, I[b], Fy[b], bo.UDL_REF)
        u = np.empty(202); u[0::2] = v[b]; u[1::2] = th[b]
        r = K @ u - f
        r[0::2][fix != 0] = 0.0
        np.testing.assert_allclose(rv[b].cpu().numpy(), r[0::2], rtol=1e-10, atol=1e-6 * np.abs(r).max())
        np.testing.assert_allclose(rt[b].cpu().numpy(), r[1::2], rtol=1e-10, atol=1e-6 * np.abs(r).max())


def test_vjp_matches_autograd_of_a_dense_reference():
    from openpystruct_amd import physics
    x, fix, I, Fy = _case(B=3, seed=2)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device="cuda")  # noqa: E731
    rng = np.random.default_rng(3)
    v0 = rng.normal(size=Fy.shape) * 1e-2; th0 = rng.normal(size=Fy.shape) * 1e-3
    gv = rng.normal(size=Fy.shape); gt = rng.normal(size=Fy.shape)
    Iq, vq, tq = t(I).requires_grad_(), t(v0).requires_grad_(), t(th0).requires_grad_()
    rv, rt = physics.fe_residual(Iq, vq, tq, t(x), t(bo.E_REF), t(fix, torch.uint8), t(Fy), t(bo.UDL_REF))
    ((rv * t(gv)).sum() + (rt * t(gt)).sum()).backward()
    # dense torch reference on the CPU: K(I) assembled from the oracle's element matrix, autograd through it
    for b in range(3):
        Ic = torch.tensor(I[b], dtype=torch.float64, requires_grad=True)
        uc = torch.zeros(202, dtype=torch.float64); uc[0::2] = torch.tensor(v0[b]); uc[1::2] = torch.tensor(th0[b])
        uc.requires_grad_()
        K = torch.zeros(202, 202, dtype=torch.float64)
        for e in range(100):
            ke = torch.tensor(bo.element_stiffness(bo.E_REF, 2.0)) * Ic[e]      # EI = E * I, L = 2
            K[2 * e:2 * e + 4, 2 * e:2 * e + 4] = K[2 * e:2 * e + 4, 2 * e:2 * e + 4] + ke
        _, f = bo.assemble_beam(x, bo.E_REF, I[b], Fy[b], bo.UDL_REF)
        r = K @ uc - torch.tensor(f)
        mask = torch.ones(202, dtype=torch.float64); mask[0::2][torch.tensor(fix != 0)] = 0.0
        g = torch.zeros(202, dtype=torch.float64); g[0::2] = torch.tensor(gv[b]); g[1::2] = torch.tensor(gt[b])
        ((r * mask) * g).sum().backward()
        np.testing.assert_allclose(Iq.grad[b].cpu().numpy(), Ic.grad.numpy(), rtol=1e-9, atol=1e-9 * float(Ic.grad.abs().max()))
        np.testing.assert_allclose(vq.grad[b].cpu().numpy(), uc.grad[0::2].numpy(), rtol=1e-9, atol=1e-9 * float(uc.grad.abs().max()))
        np.testing.assert_allclose(tq.grad[b].cpu().numpy(), uc.grad[1::2].numpy(), rtol=1e-9, atol=1e-9 * float(uc.grad.abs().max()))


def test_residual_loss_is_zero_at_solution_and_decreases_under_gradient_descent():
    import openpystruct_amd as oa
    from openpystruct_amd import physics
    x, fix, I, Fy = _case(B=4, seed=5)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device="cuda")  # noqa: E731
    sol = oa.beam_solve(t(x), t(bo.E_REF), t(I), t(fix, torch.uint8), t(Fy), t(bo.UDL_REF))
    args = (t(x), t(bo.E_REF), t(fix, torch.uint8), t(Fy), t(bo.UDL_REF))
    assert float(physics.fe_residual_loss(t(I), sol.v, sol.theta, *args)) < 1e-16
    v = (sol.v * 1.05).clone().requires_grad_(); th = (sol.theta * 0.97).clone().requires_grad_()
    l0 = physics.fe_residual_loss(t(I), v, th, *args)
    l0.backward()
    assert float(l0) > 1e-6 and torch.isfinite(v.grad).all() and float(v.grad.abs().max()) > 0


def test_pinn_training_with_the_fe_residual_term():
    """Per-case PINN (n_cases = 1) with the HIP FE-residual physics term switched on: loss finite, gradients flow."""
    from openpystruct_amd import dataprep, sizing, train
    cfg_s = sizing.SizingConfig(max_e=20)
    rec = sizing.generate_dataset(256, cfg_s, "cuda", seed=3)
    d = dataprep.prepare(rec, kind="pinn", n_cases=1, seed=0, device="cuda")
    assert d.Fy_train is not None and d.Fy_train.shape == (204, 101)
    cfg = train.PinnConfig(n_cases=1, batch_size=64)
    phys = train.PhysicsTerm(weight=1e-3, x=torch.linspace(0, 200, 101, dtype=torch.float64), E=cfg_s.E,
                             fix=torch.as_tensor(bo.reference_fix_mask()), wy=cfg_s.uniform_udl)
    out = train.train_surrogate("pinn", d, cfg, device="cuda", max_epochs=2, physics=phys)
    assert out["epochs"] == 2 and np.isfinite(out["history"]["train"]).all()
    base = train.train_surrogate("pinn", d, cfg, device="cuda", max_epochs=2)
    assert out["history"]["train"][0] != base["history"]["train"][0]       # the term is really in the loss


@pytest.mark.parametrize("kind", ["tfd", "fnn"])
def test_i_only_models_train_with_the_fe_residual_of_the_recorded_field(kind):
    """BASELINE config 4: the I-only surrogates take their physics loss from K(I_pred) u_recorded - f (HIP residual kernels)."""
    from openpystruct_amd import dataprep, physics, sizing, train
    cfg_s = sizing.SizingConfig(max_e=20)
    rec = sizing.generate_dataset(256, cfg_s, "cuda", seed=5)
    d = dataprep.prepare(rec, kind=kind, n_cases=1, seed=0, device="cuda")
    assert d.v_train is not None and d.v_train.shape == (204, 101) and d.v_train.dtype == torch.float64
    x = torch.linspace(0, 200, 101, dtype=torch.float64)
    fix = torch.as_tensor(bo.reference_fix_mask())
    # the recorded field belongs to the inertias one Adam step BEFORE the recorded ones (the reference's lag): zero
    # residual for those, and already a visible one for the recorded `I_values`
    I_rec = rec["I_solved"]
    args = (rec["deflections"], rec["rotations"], x.cuda(), cfg_s.E, fix.cuda(), None, cfg_s.uniform_udl)
    Fy = torch.zeros((256, 102), dtype=torch.float64, device="cuda").scatter_add_(1, rec["force_nodes"].long(), rec["force_values"].double())[:, 1:]
    l_true = float(physics.fe_residual_loss(I_rec, args[0], args[1], args[2], args[3], args[4], Fy, args[6]))
    l_wrong = float(physics.fe_residual_loss(rec["I_values"].double(), args[0], args[1], args[2], args[3], args[4], Fy, args[6]))
    assert l_true < 1e-6 * l_wrong
    cfg = (train.TfdConfig if kind == "tfd" else train.FnnConfig)(n_cases=1, batch_size=64)
    phys = train.PhysicsTerm(weight=1e-3, x=x, E=cfg_s.E, fix=fix, wy=cfg_s.uniform_udl)
    out = train.train_surrogate(kind, d, cfg, device="cuda", max_epochs=2, physics=phys)
    base = train.train_surrogate(kind, d, cfg, device="cuda", max_epochs=2)
    assert out["epochs"] == 2 and np.isfinite(out["history"]["train"]).all()
    assert out["history"]["train"][0] != base["history"]["train"][0]


@pytest.mark.parametrize("mode,dtype", [("recorded", torch.float32), ("predicted", torch.float32), ("recorded", torch.bfloat16), ("predicted", torch.bfloat16)])
def test_fused_residual_term_equals_the_framework_composition(mode, dtype):
    """r04: csrc/beam_residual.hip ops_physics_loss_fwd / _bwd (three launches) against what train.py built from physics.fe_residual_loss and
    ~60 framework ops: inverse scaler -> clamp -> float64 -> [row gathers] -> residual -> Jacobi scaling -> four means -> weight, and
    autograd's backward of all that.  Standardised predictions (some clamped at 1e-8), recorded displacement fields gathered by row
    (the I-only models) or predicted ones (the PINN's columns); value to 1e-6, the gradient w.r.t. the predictions to 1e-5 relative L2
    in float32 (bfloat16 predictions: the gradient's own bf16 rounding, 4e-3)."""
    from openpystruct_amd import physics
    from openpystruct_amd.dataprep import StandardScalerT
    dev = "cuda"
    x, fix, I, Fy = _case(B=40, seed=3)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=dev)  # noqa: E731
    G, nel, N = 40, 100, 101
    g = torch.Generator().manual_seed(5)
    sol_v = (torch.randn(G, N, generator=g) * 1e-2).double().to(dev)
    sol_t = (torch.randn(G, N, generator=g) * 1e-3).double().to(dev)
    sI, sD, sR = StandardScalerT(), StandardScalerT(), StandardScalerT()
    sI.fit(t(I).float()); sD.fit(sol_v.float()); sR.fit(sol_t.float())
    B = 24
    rows = torch.randperm(G, generator=g)[:B].to(dev)
    C = nel if mode == "recorded" else nel + 2 * N
    p32 = torch.randn(B, C, generator=g).to(dev)
    p32[:, :nel] = sI.transform(t(I).float()[rows]) * (1.0 + 0.05 * torch.randn(B, nel, generator=g).to(dev))
    p32[0, :7] = -50.0                                        # far below the clamp: inertia 1e-8, no gradient
    preds = p32.to(dtype).requires_grad_(True)
    ref = preds.detach().clone().requires_grad_(True)
    weight, E, wy = 1e-3, bo.E_REF, bo.UDL_REF
    # the framework composition (train.py before r04)
    pf = ref.float()
    I_p = sI.inverse_transform(pf[:, :nel]).clamp_min(1e-8)
    if mode == "recorded":
        v_p, t_p = sol_v[rows], sol_t[rows]
    else:
        v_p, t_p = sD.inverse_transform(pf[:, nel:nel + N]), sR.inverse_transform(pf[:, nel + N:])
    want = weight * physics.fe_residual_loss(I_p, v_p, t_p, t(x), t(E), t(fix, torch.uint8), t(Fy)[rows], t(wy)).float()
    want.backward()
    acc = torch.full((), 3.0, device=dev)
    disp = (sol_v, sol_t) if mode == "recorded" else (sD, sR)
    got = physics.fused_residual_term(preds, nel, sI, disp, rows, t(Fy), t(x), E, t(fix, torch.uint8), wy, weight, acc)
    got.backward(torch.ones((), device=dev))
    torch.cuda.synchronize()
    assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want)) and abs(float(acc) - 3.0 - float(got)) <= 1e-6 * abs(float(got))
    gw, gg = ref.grad.double(), preds.grad.double()
    tol = 1e-5 if dtype == torch.float32 else 4e-3
    assert float((gg - gw).norm() / gw.norm()) < tol and float(gw.norm()) > 0
    assert float(gg[0, :7].abs().max()) == 0.0                 # clamped inertias
    if mode == "recorded":
        assert preds.grad.shape == (B, nel)


# ================================================================================================================================
# The FE-residual family against the float64 references of tests/beam_dense.py, over the shapes, input forms and edges the
# kernels index by: non-uniform per-beam meshes, per-beam constraint masks with clamped rotations, per-element E and wy, one
# workgroup exactly and one node more, training-size batches.  Errors are bounded relative to the size of the terms each
# entry is a sum of (residual_ref's term scale, residual_vjp_scales), not to the entry itself: the float64 operators to
# 4e-15 of it (~18 eps; measured <= 1e-15), the solver's solution to 1e-13 (measured <= 1.7e-14 over every tiling).
# ================================================================================================================================
P_OF_100 = sorted({p for p, m in TILINGS if p * m >= 101})


@pytest.fixture(scope="module")
def ph():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi, physics
    _cabi.load()
    return physics


def _gpu(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _cpu(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


def _ratio(got, want, scale, bound):
    """max over the entries of |got - want| / (bound * scale): the comparison passes at <= 1."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu() if torch.is_tensor(want) else want, dtype=np.float64)
    scale = np.asarray(scale.detach().cpu() if torch.is_tensor(scale) else scale, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(bound * scale, 1e-300)).max())


def _inputs(rng, B, Ne, per_beam, per_elem):
    x, fix, I, Fy = random_case(rng, B, Ne, per_beam=per_beam, rz=True)
    E = rng.uniform(1.5e11, 2.5e11, size=(B, Ne)) if per_elem else np.float64(2e11)
    wy = rng.uniform(-2e3, 0, size=(B, Ne)) if per_elem else np.float64(-750.0)
    return x, fix, I, Fy, E, wy


# (Ne, B, per-beam x / fix, per-element E / wy, displacement field): B (Ne + 1) = 256 (one workgroup) and 257, Ne up to
# 1023, training-size batches; "solution": dense_solve's equilibrium field (the residual is a cancellation), else random
RES_CASES = [(1, 1, False, False, "random"), (1, 7, True, True, "solution"), (1, 128, True, True, "random"),
             (1, 1000, True, True, "random"), (2, 7, True, True, "solution"), (13, 7, True, False, "solution"),
             (13, 1000, False, True, "random"), (100, 1, True, True, "solution"), (100, 7, True, True, "random"),
             (100, 1000, True, True, "random"), (255, 1, False, True, "random"), (256, 1, True, True, "solution"),
             (255, 7, True, True, "solution"), (256, 1000, True, False, "random"), (1023, 1, True, True, "solution"),
             (1023, 7, False, True, "random"), (1023, 1000, True, True, "random")]


@pytest.mark.parametrize("Ne,B,per_beam,per_elem,field", RES_CASES)
def test_residual_and_its_vjp_match_the_float64_reference(ph, Ne, B, per_beam, per_elem, field):
    rng = np.random.default_rng(7 * Ne + B + 2 * per_beam + 4 * per_elem)
    N = Ne + 1
    x, fix, I, Fy, E, wy = _inputs(rng, B, Ne, per_beam, per_elem)
    if field == "solution":
        v, th = (o.numpy() for o in dense_solve(_cpu(x), _cpu(E), _cpu(I), fix, _cpu(Fy), _cpu(wy))[:2])
    else:
        v, th = rng.standard_normal((B, N)) * 1e-2, rng.standard_normal((B, N)) * 1e-3
    gv, gt = rng.standard_normal((B, N)), rng.standard_normal((B, N))

    Ic, vc, tc = (_cpu(a).requires_grad_(True) for a in (I, v, th))
    rv_r, rt_r, s_v, s_t = residual_ref(x, _cpu(E), Ic, fix, _cpu(Fy), _cpu(wy), vc, tc)
    dI_r, dv_r, dt_r = torch.autograd.grad((rv_r * _cpu(gv)).sum() + (rt_r * _cpu(gt)).sum(), [Ic, vc, tc])
    s_dv, s_dt, s_dI = residual_vjp_scales(x, _cpu(E), Ic.detach(), fix, vc.detach(), tc.detach(), _cpu(gv), _cpu(gt))

    Ig, vg, tg = (_gpu(a).requires_grad_(True) for a in (I, v, th))
    rv, rt = ph.fe_residual(Ig, vg, tg, _gpu(x), _gpu(E), _gpu(fix, torch.uint8), _gpu(Fy), _gpu(wy))
    dI, dv, dt = torch.autograd.grad((rv * _gpu(gv)).sum() + (rt * _gpu(gt)).sum(), [Ig, vg, tg])

    fixb = np.broadcast_to(fix, (B, N)).astype(np.int64)
    assert (fixb & 2).any()                                                        # clamped rotations are in the case
    assert float(rv.detach().cpu()[torch.from_numpy((fixb & 1) != 0)].abs().max()) == 0.0
    assert float(rt.detach().cpu()[torch.from_numpy((fixb & 2) != 0)].abs().max()) == 0.0
    assert _ratio(rv, rv_r, s_v, 4e-15) <= 1 and _ratio(rt, rt_r, s_t, 4e-15) <= 1
    assert _ratio(dv, dv_r, s_dv, 4e-15) <= 1 and _ratio(dt, dt_r, s_dt, 4e-15) <= 1
    assert _ratio(dI, dI_r, s_dI, 4e-15) <= 1


@pytest.mark.parametrize("tiling", [0] + P_OF_100)
def test_residual_vanishes_at_the_solver_solution(ph, tiling):
    """Ties the solver's load and constraint semantics to the operator's: at beam_solve's solution (every tiling of 100 elements)
    the HIP residual is rounding-level relative to its term sizes.  The fat-wave tiling takes shared geometry and scalars only."""
    import openpystruct_amd as oa
    rng = np.random.default_rng(40 + tiling)
    shared = tiling in FAT_P
    B, Ne = 200, 100
    x, fix, I, Fy, E, wy = _inputs(rng, B, Ne, per_beam=not shared, per_elem=not shared)
    args = (_gpu(x), _gpu(E), _gpu(I), _gpu(fix, torch.uint8), _gpu(Fy), _gpu(wy))
    sol = oa.beam_solve(*args, tiling=tiling)
    assert int(sol.status.abs().sum()) == 0
    rv, rt = ph.fe_residual(args[2], sol.v, sol.theta, args[0], args[1], args[3], args[4], args[5])
    rv_r, rt_r, s_v, s_t = residual_ref(x, _cpu(E), _cpu(I), fix, _cpu(Fy), _cpu(wy), sol.v.cpu(), sol.theta.cpu())
    assert _ratio(rv, 0.0, s_v, 1e-13) <= 1 and _ratio(rt, 0.0, s_t, 1e-13) <= 1
    assert _ratio(rv_r, 0.0, s_v, 1e-13) <= 1 and _ratio(rt_r, 0.0, s_t, 1e-13) <= 1


def _scaler(t):
    from openpystruct_amd.dataprep import StandardScalerT
    return StandardScalerT().fit(t.float())


def _bf16_ulp(r):
    """One bfloat16 ulp at |r| (8 significant bits)."""
    _, e = torch.frexp(r.abs())
    return torch.ldexp(torch.ones_like(r), e - 8)


def _term_case(rng, B, Ne, mesh, rows_kind, mode, dtype):
    """Inputs of the fused term: shared mesh (the reference bridge or a non-uniform one), G recorded cases, rows into them
    (with repeats and G > B, or None), standardised predictions near the scaled truth with some inertias clamped."""
    N = Ne + 1
    G = B + 3
    if mesh == "bridge":
        x, fix = np.linspace(0, 200, N), bo.reference_fix_mask()
        I, Fy = bo.random_cases(rng, G, inertia="trajectory")
    else:
        x, fix, I, Fy = random_case(rng, G, Ne, rz=True)
    v_rec, t_rec = _gpu(rng.standard_normal((G, N)) * 1e-2), _gpu(rng.standard_normal((G, N)) * 1e-3)
    sI, sD, sR = _scaler(_gpu(I)), _scaler(v_rec), _scaler(t_rec)
    if rows_kind == "repeat":
        r = rng.integers(0, G, size=B)
        r[-1] = r[0]
        rows = torch.as_tensor(r, dtype=torch.int64, device="cuda")
    else:
        rows = None
    ri = torch.arange(B, device="cuda") if rows is None else rows
    C = Ne if mode == "recorded" else Ne + 2 * N
    p = _gpu(rng.standard_normal((B, C)), torch.float32)
    p[:, :Ne] = sI.transform(_gpu(I).float()[ri]) * (1.0 + 0.05 * _gpu(rng.standard_normal((B, Ne)), torch.float32))
    clamped = []
    if B > 1 or Ne > 2:
        b, e = B - 1, Ne // 2
        p[b, e] = -50.0                                          # far below the clamp: inertia 1e-8, no gradient
        clamped.append((b, e))
    disp = (v_rec, t_rec) if mode == "recorded" else (sD, sR)
    return dict(x=_gpu(x), fix=_gpu(fix, torch.uint8), Fy=_gpu(Fy), sI=sI, disp=disp, rows=rows, p=p.to(dtype), C=C,
                clamped=clamped)


# (B, Ne, mesh, rows): the smallest term, one workgroup exactly / one node more at B = 1, training batches on the reference
# bridge, and a non-uniform shared mesh at a training shape
TERM_CASES = [(1, 1, "random", "none"), (1, 255, "random", "repeat"), (1, 256, "random", "none"), (24, 100, "bridge", "repeat"),
              (24, 100, "random", "repeat"), (512, 100, "bridge", "none"), (4096, 100, "bridge", "repeat")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["recorded", "predicted"])
@pytest.mark.parametrize("B,Ne,mesh,rows_kind", TERM_CASES)
def test_fused_term_matches_the_float64_reference(ph, B, Ne, mesh, rows_kind, mode, dtype):
    rng = np.random.default_rng(B + 3 * Ne + (mode == "predicted") + 2 * (dtype == torch.bfloat16) + 4 * (mesh == "random"))
    c = _term_case(rng, B, Ne, mesh, rows_kind, mode, dtype)
    E, wy, weight = 2e11, -750.0, 1e-3
    spec = (Ne, c["sI"], c["disp"], c["rows"], c["Fy"], c["x"], E, c["fix"], wy, weight)
    want, g_ref, _ = residual_term_ref(c["p"], *spec)

    # contiguous predictions
    p1 = c["p"].clone().requires_grad_(True)
    got = ph.fused_residual_term(p1, *spec)
    got.backward()
    # the same predictions as a column view of a wider matrix (row stride > C), with the running sum
    wide = torch.zeros(B, c["C"] + 7, dtype=dtype, device="cuda")
    wide[:, 3:3 + c["C"]] = c["p"]
    wide.requires_grad_(True)
    acc = torch.full((), 3.0, device="cuda")
    got2 = ph.fused_residual_term(wide[:, 3:3 + c["C"]], *spec, acc=acc)
    got2.backward()
    torch.cuda.synchronize()

    assert float(want) > 0 and _ratio(float(got), float(want), abs(float(want)), 2e-7) <= 1       # the float32 value's rounding
    assert torch.equal(got, got2) and torch.equal(acc, torch.full((), 3.0, device="cuda") + got)
    assert torch.equal(wide.grad[:, 3:3 + c["C"]], p1.grad)
    assert float(wide.grad[:, :3].abs().max()) == 0.0 and float(wide.grad[:, 3 + c["C"]:].abs().max()) == 0.0
    g = p1.grad.double().cpu()
    for b, e in c["clamped"]:
        assert float(g[b, e]) == 0.0 and float(g_ref[b, e]) == 0.0
    if dtype == torch.float32:
        assert _ratio(g, g_ref, float(g_ref.abs().max()), 1.2e-7) <= 1                                # float32 rounding: <= 2^-24 |g|
    else:
        assert _ratio(g, g_ref, _bf16_ulp(g_ref), 1.0) <= 1                                           # within one bfloat16 ulp


@pytest.mark.parametrize("mode", ["recorded", "predicted"])
def test_a_nan_inertia_prediction_shows_in_the_term_on_both_paths(ph, mode):
    """A diverged prediction is not clamped away: the term is NaN whether it is fused or composed from framework ops
    (clamp_min), and the other samples' gradient rows are those of the same call with that prediction finite, bit for bit."""
    rng = np.random.default_rng(61 + (mode == "predicted"))
    B, Ne = 24, 100
    N = Ne + 1
    c = _term_case(rng, B, Ne, "bridge", "repeat", mode, torch.float32)
    E, wy, weight = 2e11, -750.0, 1e-3
    spec = (Ne, c["sI"], c["disp"], c["rows"], c["Fy"], c["x"], E, c["fix"], wy, weight)
    k = 5
    grads = []
    for bad in (False, True):
        p = c["p"].clone()
        if bad:
            p[k, 17] = float("nan")
        p.requires_grad_(True)
        val = ph.fused_residual_term(p, *spec)
        val.backward()
        grads.append(p.grad.clone())
        assert torch.isnan(val).item() == bad
        # the framework composition of the same term (the `fused_physics` switch off)
        I_p = c["sI"].inverse_transform(p.detach()[:, :Ne]).clamp_min(1e-8)
        if mode == "recorded":
            v_p, t_p = (d[c["rows"]] for d in c["disp"])
        else:
            v_p, t_p = c["disp"][0].inverse_transform(p.detach()[:, Ne:Ne + N]), c["disp"][1].inverse_transform(p.detach()[:, Ne + N:])
        ref = weight * ph.fe_residual_loss(I_p, v_p, t_p, c["x"], E, c["fix"], c["Fy"][c["rows"]], wy)
        assert torch.isnan(ref).item() == bad
    others = [b for b in range(B) if b != k]
    assert torch.equal(grads[0][others], grads[1][others])
    assert torch.isfinite(grads[1][others]).all()


class _NoLaunch:
    """The library with its residual entries replaced by a failure: a wrapper that reached them did not refuse first."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in ("ops_beam_residual_f64", "ops_beam_residual_vjp_f64", "ops_physics_loss_fwd", "ops_physics_loss_bwd"):
            raise AssertionError(f"{name} reached with arguments the wrapper should refuse")
        return getattr(self._lib, name)


def test_wrappers_refuse_shapes_the_kernels_would_read_out_of_range(ph, monkeypatch):
    from openpystruct_amd import _cabi
    monkeypatch.setattr(_cabi, "load", lambda lib=_NoLaunch(_cabi.load()): lib)
    rng = np.random.default_rng(3)
    B, Ne = 5, 8
    N = Ne + 1
    x, fix, I, Fy, E, wy = _inputs(rng, B, Ne, per_beam=True, per_elem=True)
    v, th = _gpu(rng.standard_normal((B, N))), _gpu(rng.standard_normal((B, N)))
    ok = dict(x=_gpu(x), E=_gpu(E), fix=_gpu(fix, torch.uint8), wy=_gpu(wy))
    bad = [("E", _gpu(E[0])), ("E", _gpu(E[:, 0])), ("wy", _gpu(wy[0])), ("wy", _gpu(wy[:, 0])),
           ("x", _gpu(x[:B - 1])), ("fix", _gpu(fix[:B - 1], torch.uint8))]
    for name, t in bad:
        a = dict(ok, **{name: t})
        with pytest.raises(ValueError, match=rf"^{name} must"):
            ph.fe_residual(_gpu(I), v, th, a["x"], a["E"], a["fix"], _gpu(Fy), a["wy"])
    c = _term_case(rng, 4, Ne, "random", "repeat", "recorded", torch.float32)
    for name, xs, fs in (("x", c["x"].expand(4, N).contiguous(), c["fix"]), ("x", c["x"][:Ne], c["fix"]),
                         ("fix", c["x"], c["fix"].expand(4, N).contiguous()), ("fix", c["x"], c["fix"][:Ne])):
        with pytest.raises(ValueError, match=rf"^{name} must"):
            ph.fused_residual_term(c["p"], Ne, c["sI"], c["disp"], c["rows"], c["Fy"], xs, 2e11, fs, -750.0, 1e-3)
