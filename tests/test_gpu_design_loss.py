"""The design-objective term on the GPU: ops_design_loss_finish on synthetic rows and ops_design_loss_prep against
the float64 / framework references of tests/design_loss_ref.py, the four launches end to end against autograd of the design
objective through the dense model (one leaf per design), the term's failure semantics and independence of its launch, and two
epochs of training with `train.DesignTerm`."""
import ctypes
import functools
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import design_loss_ref as dr  # noqa: E402
from tests import sizing_multicase_ref as mr  # noqa: E402
from tests import sizing_step_cases as sc  # noqa: E402
from tests import sizing_total_ref as tr  # noqa: E402
from tests.beam_dense import cond_free, gI_term_scale, random_case  # noqa: E402
from tests.test_design_loss_emulation import SHAPES, Scaler, check_against_reference, predictions, variants  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from openpystruct_amd import _cabi
    return _cabi.load()


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def call_finish(lib, s, C, agg, w, extra, t, sI, weight, ref=None, rows=None, status_solve=None, status_grad=None, G=None):
    """ops_design_loss_finish on the synthetic rows `s` (tests.design_loss_ref.synthetic_rows), V, M, grad and extra passed straight
    through the C entry.  Returns the host copies of every output."""
    from openpystruct_amd import _cabi
    B, Ne = s.I.shape
    bf16 = t.dtype == torch.bfloat16
    f64 = dict(dtype=torch.float64, device=DEV)
    keep = dict(I=_dev(np.repeat(s.I, C, axis=0)), V=_dev(s.V.reshape(B * C, Ne)), M=_dev(s.M.reshape(B * C, Ne)),
                g=_dev(s.grad.reshape(B * C, Ne)), ex=_dev(None if extra is None else extra.reshape(-1)), w=_dev(w), p=t.to(DEV),
                sc=sI.scale_.to(DEV), mn=sI.mean_.to(DEV), ref=_dev(ref), rows=_dev(rows, torch.int64),
                ss=_dev(status_solve, torch.int32), sg=_dev(status_grad, torch.int32))
    out = dict(sample_loss=torch.empty((B,), **f64), gI=torch.empty((B, Ne), **f64), case_penalty=torch.empty((B, C), **f64),
               governing=torch.empty((B,), dtype=torch.int32, device=DEV), dpreds=torch.zeros_like(keep["p"]),
               value=torch.empty((), dtype=torch.float32, device=DEV), acc=torch.full((), 2.0, dtype=torch.float32, device=DEV))
    part = torch.empty((int(lib.ops_design_loss_part_doubles(B)),), **f64)
    a = _cabi.DesignLossArgs(B=B, C=C, Ne=Ne, G=G if G is not None else B, aggregate=agg, preds_bf16=int(bf16), ldp=t.stride(0),
                             preds=keep["p"].data_ptr(), I_scale=keep["sc"].data_ptr(), I_mean=keep["mn"].data_ptr(), I_min=1e-8,
                             weight=weight, rows=_ptr(keep["rows"]), ref=_ptr(keep["ref"]), weights=_ptr(keep["w"]),
                             I_rows=keep["I"].data_ptr(), V=keep["V"].data_ptr(), M=keep["M"].data_ptr(), grad=keep["g"].data_ptr(),
                             loss_extra=_ptr(keep["ex"]), status_solve=_ptr(keep["ss"]), status_grad=_ptr(keep["sg"]),
                             sample_loss=out["sample_loss"].data_ptr(), gI=out["gI"].data_ptr(),
                             case_penalty=out["case_penalty"].data_ptr(), governing=out["governing"].data_ptr(),
                             dpreds=out["dpreds"].data_ptr(), part=part.data_ptr(), value=out["value"].data_ptr(),
                             value_sum=out["acc"].data_ptr())
    assert lib.ops_design_loss_finish(ctypes.byref(a), ctypes.byref(s.hp), _stream()) == 0
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in out.items()}
    got["dpreds"] = got["dpreds"].float().numpy().astype(np.float64)
    got["value"], got["acc"] = float(got["value"]), float(got["acc"])
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the finish kernel on synthetic rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("B,C,Ne", SHAPES)
def test_finish_kernel_vs_the_float64_reference(lib, B, C, Ne, with_extra):
    """Every elements-per-lane instantiation (Ne 1..64, 65..128, 512), one and several blocks of four samples, a ragged last block,
    C = 1 and the C = 64 limit; the three aggregates; float32 predictions with ref and rows NULL, bfloat16 ones with both given
    (rows with repeats, into a longer ref)."""
    rng = np.random.default_rng([B, C, Ne, with_extra])
    s = dr.synthetic_rows(B, C, Ne, seed=1)
    extra = s.extra if with_extra else None
    weight = float(np.float32(0.7))
    G = B + 2
    for bf16 in (False, True):
        rows = rng.integers(0, G, size=B) if bf16 else None
        if bf16 and B > 1:
            rows[-1] = rows[0]
        ref = rng.uniform(0.5, 50.0, size=G) if bf16 else None
        t, sI = predictions(rng, B, Ne, Ne + 2, bf16)
        live = (dr.raw_reference(t[:, :Ne], sI) > 1e-8).numpy()
        for name, agg, w in variants(C):
            r = dr.finish_reference(s.I, s.V, s.M, s.grad, extra, w, agg, s.hp, live=live, scale=sI.scale_.numpy(), weight=weight,
                                    ref=None if ref is None else ref[rows])
            # at least 5 % between the two largest (weighted) penalties of every reference input: the governing case is not a matter of rounding
            assert dr.well_separated(r.case_penalty if agg == mr.MAX else (np.ones(C) if w is None else w) * r.case_penalty), name
            got = call_finish(lib, s, C, agg, w, extra, t, sI, weight, ref=ref, rows=rows, G=G)
            check_against_reference(got, r, Ne, bf16, weight, B)
            assert (got["dpreds"][:, :Ne][~live] == 0).all() and not live.all()
            assert got["acc"] == float(np.float32(2.0) + np.float32(got["value"]))
            if agg == mr.MAX:
                assert np.array_equal(got["governing"], s.big) and np.array_equal(got["gI"], s.grad[np.arange(B), s.big])


def test_two_identical_case_rows_the_lower_index_governs(lib):
    rng = np.random.default_rng(5)
    B, C, Ne = 5, 4, 65
    s = dr.synthetic_rows(B, C, Ne, seed=2)
    t, sI = predictions(rng, B, Ne, Ne, False)
    for a in (s.V, s.M, s.grad):
        a[:, 1] = a[np.arange(B), s.big]
        a[:, 3] = a[:, 1]
    for agg in (mr.MAX, mr.SUM):
        got = call_finish(lib, s, C, agg, None, None, t, sI, 1.0)
        assert (got["governing"] == np.where(s.big == 0, 0, 1)).all()


def test_a_failed_row_of_either_launch_is_nan_for_its_sample_only(lib):
    rng = np.random.default_rng(6)
    B, C, Ne = 9, 3, 100
    s = dr.synthetic_rows(B, C, Ne, seed=3)
    t, sI = predictions(rng, B, Ne, Ne, False)
    clean = call_finish(lib, s, C, mr.SUM, None, None, t, sI, 1.0)
    ss, sg = np.zeros(B * C, dtype=np.int32), np.zeros(B * C, dtype=np.int32)
    ss[1 * C + 2], sg[6 * C + 0] = 3, 1
    hit = call_finish(lib, s, C, mr.SUM, None, None, t, sI, 1.0, status_solve=ss, status_grad=sg)
    ok = np.ones(B, dtype=bool)
    ok[[1, 6]] = False
    for k in ("sample_loss", "gI", "dpreds"):
        assert np.isnan(hit[k][~ok]).all() and np.array_equal(hit[k][ok], clean[k][ok]), k
    assert np.isnan(hit["value"]) and np.isfinite(clean["value"])


# ---------------------------------------------------------------------------------------------------------------------
# the prep kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("B,C,Ne", [(1, 1, 1), (7, 3, 13), (5, 6, 100), (3, 2, 512)])
def test_prep_kernel_is_the_frameworks_expression_and_the_gather(lib, B, C, Ne, bf16):
    from openpystruct_amd import _cabi
    rng = np.random.default_rng([B, C, Ne, bf16])
    N, G, ld = Ne + 1, B + 3, Ne + 5
    t, sI = predictions(rng, B, ld, ld, bf16)          # a wider matrix: the term reads its columns 2 .. 2 + Ne
    sI = Scaler(sI.scale_[:Ne], sI.mean_[:Ne])
    big = t.to(DEV)
    view = big[:, 2:2 + Ne]
    Fy = torch.as_tensor(rng.uniform(-1e5, 1e4, size=(G, C, N))).to(DEV)
    rows_h = rng.integers(0, G, size=B)
    rows_h[0] = G + 1                                   # out of range on both sides: wrapped modulo G, never read
    if B > 1:
        rows_h[1] = -2
    for rows in (None, torch.as_tensor(rows_h).to(DEV)):
        I_rows = torch.full((B * C, Ne), -1.0, dtype=torch.float64, device=DEV)
        Fy_rows = torch.full((B * C, N), -1.0, dtype=torch.float64, device=DEV)
        sc_d, mn_d = sI.scale_.to(DEV), sI.mean_.to(DEV)
        a = _cabi.DesignLossArgs(B=B, C=C, Ne=Ne, G=G, preds_bf16=int(bf16), ldp=view.stride(0), preds=view.data_ptr(),
                                 I_scale=sc_d.data_ptr(), I_mean=mn_d.data_ptr(), I_min=1e-8, rows=_ptr(rows), Fy_src=Fy.data_ptr(),
                                 I_rows=I_rows.data_ptr(), Fy_rows=Fy_rows.data_ptr())
        assert lib.ops_design_loss_prep(ctypes.byref(a), _stream()) == 0
        torch.cuda.synchronize()
        want = sI.inverse_transform(view.float()).clamp_min(1e-8).double()
        assert torch.equal(I_rows.reshape(B, C, Ne), want[:, None].expand(B, C, Ne))
        src = torch.arange(B, device=DEV) if rows is None else torch.remainder(rows, G)
        assert torch.equal(Fy_rows.reshape(B, C, N), Fy[src])
    assert Ne == 1 or bool((want == float(np.float32(1e-8))).any())


# ---------------------------------------------------------------------------------------------------------------------
# the four launches
# ---------------------------------------------------------------------------------------------------------------------
def _unstandardise(I, rng):
    """A scaler and float32 standardised predictions whose inverse transform lands near I (the term then works on the float32
    value it computes, which the references take over)."""
    Ne = I.shape[1]
    sI = Scaler(rng.uniform(0.05, 0.3, size=Ne).astype(np.float32), rng.uniform(0.2, 0.6, size=Ne).astype(np.float32))
    p = ((torch.as_tensor(I).float() - sI.mean_) / sI.scale_).contiguous()
    return p, sI


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """The reference bridge (Ne = 100: SizingConfig's 101 nodes and five rollers) or a non-uniform mesh (Ne = 13): B = 3 designs under
    C = 3 load cases, one case's loads scaled by 4; the dense model's rows computed once."""
    from openpystruct_amd import sizing
    B, C = 3, 3
    hp = sc.beam_hp()
    if name == "bridge":
        cfg = sizing.SizingConfig()
        cases = sizing.make_cases(B * C, cfg, seed=5, device="cpu")
        x, fix, Fy = cases.node_positions[0].numpy(), cases.fix[0].numpy(), cases.Fy.numpy().reshape(B, C, -1).copy()
        rng = np.random.default_rng(17)
        I = np.exp(rng.uniform(np.log(0.05), np.log(0.5), size=(B, cfg.num_elements)))
        E, wy = cfg.E, cfg.uniform_udl
    else:
        rng = np.random.default_rng(18)
        x, fix, I, Fy = random_case(rng, B * C, 13)
        I, Fy = I[:B], Fy.reshape(B, C, -1).copy()
        E, wy = 2.0e11, -750.0
    Fy[np.arange(B), [2, 0, 1]] *= 4.0
    p, sI = _unstandardise(I, rng)
    I = dr.prep_reference(p, sI).numpy()          # what the term sizes: the float32 inverse transform, widened
    rows = [[tr.total_gradient_ref(x, E, I[b:b + 1], fix, Fy[b, c:c + 1], wy, hp, tr.objective()) for c in range(C)] for b in range(B)]
    scale = np.array([[max(np.linalg.norm(r.grad), gI_term_scale(x, I[b:b + 1], wy, r.outs, r.cot)) for r in rows[b]] for b in range(B)])
    kappa = max(cond_free(x, E, I[b], fix) for b in range(B))
    return types.SimpleNamespace(x=x, fix=fix, I=I, Fy=Fy, E=E, wy=wy, hp=hp, p=p, sI=sI, rows=rows, scale=scale, kappa=kappa, B=B, C=C)


def run_term(m, p, *, aggregate="sum", weights=None, weight=1.0, ref=None, rows=None, acc=None, Fy=None, **kw):
    from openpystruct_amd import design_loss
    Fy = torch.as_tensor(m.Fy if Fy is None else Fy).to(DEV)
    spec = design_loss._term_spec(torch.device(DEV), m.I.shape[1], m.sI, rows, Fy, _dev(m.x), m.E, _dev(m.fix, torch.uint8), m.wy, m.hp,
                                  weight, aggregate, weights, kw.get("alpha_deflection", 0.0), kw.get("deflection_limit"), ref, acc)
    o = design_loss._term_launches(p.to(DEV), spec)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("mode", ["sum", "sum+w", "max"])
@pytest.mark.parametrize("name", ["bridge", "mesh13"])
def test_term_end_to_end_vs_autograd_of_the_design_objective(lib, name, mode):
    """gI to the bound tests/test_gpu_sizing_total.py holds the gradient kernel to on the mesh -- tol = max(1e-8, 4e-16 cond) in the
    scale of `grad_error` -- summed over the cases with |w_c| (only a C-term float64 sum lies between that kernel and gI).  The
    value: V and M carry the forward's error, at most fwd = max(1e-10, 4e-16 cond) of their norms (tests/test_gpu_beam_grad.py), which
    moves a case's penalty by at most 2 fwd (a_M |M| |M / den_b| + a_V |V| |V / den_s|)."""
    m = _mesh(name)
    B, C = m.B, m.C
    w = np.array([0.5, 1.0, 2.0]) if mode == "sum+w" else None
    agg = mr.MAX if mode == "max" else mr.SUM
    ref = dr.term_autograd(m.x, m.E, m.I, m.fix, m.Fy, m.wy, m.hp, tr.objective(), w, agg)
    assert dr.well_separated(ref.P)      # (the 4-fold loads: the worst case is clear)
    o = run_term(m, m.p, aggregate="max" if agg == mr.MAX else "sum", weights=w)
    assert int(o.keep[0].status.abs().sum()) == 0 and int(o.keep[3].abs().sum()) == 0
    assert torch.equal(o.I_rows.reshape(B, C, -1)[:, 0].cpu(), torch.as_tensor(m.I))
    gI, L, P = o.gI.cpu().numpy(), o.sample_loss.cpu().numpy(), o.case_penalty.cpu().numpy()
    assert np.array_equal(o.governing.cpu().numpy(), ref.governing if agg == mr.MAX else np.argmax((np.ones(C) if w is None else w) * ref.P, axis=1))
    tol, fwd = max(1e-8, 4e-16 * m.kappa), max(1e-10, 4e-16 * m.kappa)
    for b in range(B):
        wb = np.eye(C)[ref.governing[b]] if agg == mr.MAX else (np.ones(C) if w is None else w)
        err, bound = np.linalg.norm(gI[b] - ref.grad[b]), tol * float((np.abs(wb) * m.scale[b]).sum())
        print(f"{name} {mode} sample {b}: |gI - autograd| {err:.3e} (bound {bound:.3e}), L {L[b]:.9e} vs {ref.loss[b]:.9e}")
        assert err < bound
        den_b, den_s = 2.0 * m.hp.E * m.I[b] + m.hp.bend_eps, m.hp.G * m.hp.area_coef * np.sqrt(m.I[b])
        move = np.array([2.0 * fwd * (m.hp.alpha_moment * np.linalg.norm(r.outs[3]) * np.linalg.norm(r.outs[3] / den_b)
                                      + m.hp.alpha_shear * np.linalg.norm(r.outs[2]) * np.linalg.norm(r.outs[2] / den_s)) for r in m.rows[b]])
        assert (np.abs(P[b] - ref.P[b]) <= move + 1e-14 * np.abs(ref.P[b])).all()
        assert abs(L[b] - ref.loss[b]) <= float((np.abs(wb) * move).sum()) + 1e-14 * abs(ref.loss[b])


def test_one_load_case_collapses_to_the_gradient_row(lib):
    """C = 1, the sum, no weights, a unit scaler, weight = B, ref NULL, float32 predictions: gI is ops_beam_sizing_grad_f64's row bit
    for bit and dpreds its float32 rounding -- without and with the deflection term, whose value reaches the objective."""
    import openpystruct_amd as oa
    from openpystruct_amd import sizing
    m = _mesh("bridge")
    B, Ne = m.B, m.I.shape[1]
    unit = types.SimpleNamespace(**{**m.__dict__, "sI": Scaler(np.ones(Ne, dtype=np.float32), np.zeros(Ne, dtype=np.float32))})
    p = torch.as_tensor(m.I).float()
    Fy1 = m.Fy[:, :1].copy()
    x, fix, Id, Fy = _dev(m.x), _dev(m.fix, torch.uint8), p.double().to(DEV), _dev(Fy1[:, 0])
    sol = oa.beam_solve(x, _dev(np.float64(m.E)), Id, fix, Fy, _dev(np.float64(m.wy)), tiling=sizing.sizing_tiling(Ne + 1))
    vlim = float(sol.v.abs().median())
    for kw in ({}, {"alpha_deflection": 100.0, "deflection_limit": vlim}):
        grad, extra, status = oa.beam_sizing_gradient(x, m.E, Id, fix, m.wy, sol, m.hp, **kw)
        o = run_term(unit, p, weight=float(B), Fy=Fy1, **kw)
        assert int(status.abs().sum()) == 0
        assert torch.equal(o.gI, grad) and torch.equal(o.dpreds, grad.float())
        if kw:
            assert bool((extra > 0).any())
            free = run_term(unit, p, weight=float(B), Fy=Fy1)
            # (the term enters the float64 sum last: the difference of the two objectives is it, up to the roundings of the sums)
            assert bool(((o.sample_loss - free.sample_loss - extra).abs() <= 4 * 2.0 ** -53 * o.sample_loss.abs()).all())
        got = oa.design_objective(Id, x, m.E, fix, torch.as_tensor(Fy1).to(DEV), m.wy, m.hp, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got.value, o.sample_loss) and torch.equal(got.grad, o.gI) and int(got.status.abs().sum()) == 0
        assert tuple(got.case_penalty.shape) == (B, 1) and got.governing.dtype == torch.int32


def test_a_sample_does_not_depend_on_its_launch(lib):
    """Sample 0 and the last sample alone (B = 1, weight 1) equal themselves in the B = 4 launch (weight 4: the same weight / B), in
    every bit; `rows` picks their load cases."""
    m = _mesh("mesh13")
    p = torch.cat([m.p, m.p[:1] * 0.9])
    rows4 = torch.tensor([0, 1, 2, 1], device=DEV)
    refG = _dev(np.array([3.0, 5.0, 7.0]))
    for mode in ("sum", "max"):
        full = run_term(m, p, aggregate=mode, weight=4.0, rows=rows4, ref=refG)
        for b in (0, 3):
            one = run_term(m, p[b:b + 1], aggregate=mode, weight=1.0, rows=rows4[b:b + 1].contiguous(), ref=refG)
            for k in ("sample_loss", "gI", "case_penalty", "governing", "dpreds"):
                assert torch.equal(getattr(full, k)[b:b + 1], getattr(one, k)), (mode, b, k)


def test_nan_predictions_and_clamped_ones(lib):
    m = _mesh("mesh13")
    clean = run_term(m, m.p)
    p = m.p.clone()
    p[1, 4] = float("nan")
    hit = run_term(m, p)
    for k in ("sample_loss", "gI", "dpreds"):
        assert bool(torch.isnan(getattr(hit, k)[1]).all()), k
        assert torch.equal(getattr(hit, k)[[0, 2]], getattr(clean, k)[[0, 2]]), k
    assert bool(torch.isnan(hit.value)) and bool(torch.isfinite(clean.value))
    # far below the floor: the inertia is the floor and the prediction gets exactly no gradient
    p = m.p.clone()
    p[0, 3] = p[2, 7] = -1e4
    low = run_term(m, p)
    assert int(low.keep[0].status.abs().sum()) == 0 and bool(torch.isfinite(low.value))
    assert float(low.I_rows[0, 3]) == float(np.float32(1e-8)) and float(low.dpreds[0, 3]) == 0.0 and float(low.dpreds[2, 7]) == 0.0
    assert float(low.gI[0, 3]) != 0.0 and int((low.dpreds == 0).sum()) == 2


def test_strides_the_running_sum_and_autograd(lib):
    from openpystruct_amd import design_loss
    m = _mesh("mesh13")
    B, Ne = m.p.shape
    for dtype in (torch.float32, torch.bfloat16):
        dense = m.p.to(dtype)
        want = run_term(m, dense)
        big = torch.randn((B, Ne + 7)).to(dtype)
        big[:, :Ne] = dense
        view = big.to(DEV)[:, :Ne + 3]              # row stride Ne + 7, three columns the term does not read
        got = run_term(m, view)
        assert got.dpreds.stride() == view.stride() and got.dpreds.dtype == dtype
        assert torch.equal(got.dpreds[:, :Ne], want.dpreds) and bool((got.dpreds[:, Ne:] == 0).all())
        assert torch.equal(got.value, want.value) and torch.equal(got.gI, want.gI)
    # the autograd Function: the value, `acc`, the stored gradient whatever comes in from above
    acc = torch.zeros((), dtype=torch.float32, device=DEV)
    p = m.p.to(DEV).requires_grad_(True)
    args = (m.I.shape[1], m.sI, None, torch.as_tensor(m.Fy).to(DEV), _dev(m.x), m.E, _dev(m.fix, torch.uint8), m.wy, m.hp, 0.5)
    v = design_loss.design_objective_term(p, *args, acc=acc)
    want = run_term(m, m.p, weight=0.5)
    assert torch.equal(v.detach(), want.value) and float(acc) == float(v.detach())
    (3.0 * v).backward()
    assert torch.equal(p.grad, want.dpreds)
    design_loss.design_objective_term(p.detach(), *args, acc=acc)
    assert float(acc) == float(np.float32(2.0) * np.float32(float(v.detach())))
    with pytest.raises(ValueError, match="rows"):
        design_loss.design_objective_term(p, *args[:2], torch.zeros(1, dtype=torch.int64, device=DEV), *args[3:])
    with pytest.raises(ValueError, match="Fy_cases"):
        design_loss.design_objective_term(p, *args[:3], args[3][:2], *args[4:])


def test_ten_plain_gradient_steps_lower_the_value(lib):
    from openpystruct_amd import design_loss
    m = _mesh("mesh13")
    p = m.p.to(DEV).requires_grad_(True)
    args = (m.I.shape[1], m.sI, None, torch.as_tensor(m.Fy).to(DEV), _dev(m.x), m.E, _dev(m.fix, torch.uint8), m.wy, m.hp, 1.0)
    values = []
    for _ in range(11):
        v = design_loss.design_objective_term(p, *args, aggregate="max")
        values.append(float(v))
        (g,) = torch.autograd.grad(v, p)
        with torch.no_grad():
            p -= 0.02 * g / g.abs().max()
    print("values over ten plain gradient steps:", values)
    assert values[-1] < values[0] and all(np.isfinite(values))


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _designs():
    from openpystruct_amd import multicase, sizing
    cfg = sizing.SizingConfig(max_e=40)
    rec = multicase.generate_multicase_dataset(48, 3, cfg, "cuda", seed=11)
    assert int(rec["status"].abs().sum()) == 0
    fix = sizing.make_cases(1, cfg, seed=11, device="cpu").fix[0]
    return cfg, rec, fix


def _term(cfg, rec, fix, **kw):
    from openpystruct_amd import train
    return train.DesignTerm(weight=0.5, x=rec["node_positions"][0].double().cpu(), E=cfg.E, fix=fix, wy=cfg.uniform_udl, hp=cfg, **kw)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("kind", ["tfd", "fnn"])
def test_training_with_the_design_term(lib, kind, use_graph):
    from openpystruct_amd import dataprep, train
    cfg, rec, fix = _designs()
    d = dataprep.prepare(rec, kind=kind, n_cases=3, seed=0, device="cuda")
    assert tuple(d.Fy_cases_train.shape) == (38, 3, 101) and d.Fy_train is None
    tcfg = {"tfd": train.TfdConfig, "fnn": train.FnnConfig}[kind](n_cases=3, batch_size=16)
    said = []
    out = train.train_surrogate(kind, d, tcfg, device="cuda", max_epochs=2, seed=3, use_graph=use_graph, log=said.append,
                                physics=_term(cfg, rec, fix, aggregate="max"))
    assert not any("capture" in line and "failed" in line for line in said), said      # the captured step was captured
    assert out["epochs"] == 2 and np.isfinite(out["history"]["train"]).all() and np.isfinite(out["history"]["val"]).all()
    assert np.isfinite(out["design_term_sum"]) and out["design_term_sum"] > 0.0
    gap = out["design_gap_val"]
    assert set(gap) >= {"mean", "median", "max", "failed"} and gap["failed"] == 0
    assert all(np.isfinite(gap[k]) for k in ("mean", "median", "max")) and gap["max"] >= gap["median"]
    print(f"{kind} {'captured' if use_graph else 'eager'}: design_gap_val {gap}, term sum {out['design_term_sum']:.4f}")
    with pytest.raises(ValueError, match="n_cases == 1"):       # the FE-residual term on grouped data: refused as before
        train.train_surrogate(kind, d, tcfg, device="cuda", max_epochs=1,
                              physics=train.PhysicsTerm(weight=0.1, x=rec["node_positions"][0].double(), E=cfg.E, fix=fix, wy=cfg.uniform_udl))


def test_the_design_term_refuses_random_bridges(lib):
    from openpystruct_amd import dataprep, multicase, sizing, train
    cfg = sizing.SizingConfig(max_e=5, random_bridge=1)
    rec = multicase.generate_multicase_dataset(10, 3, cfg, "cuda", seed=2)
    d = dataprep.prepare(rec, kind="fnn", n_cases=3, seed=0, device="cuda")
    fix = sizing.make_cases(1, cfg, seed=2, device="cpu").fix[0]
    with pytest.raises(ValueError, match="ONE (geometry|support set)"):
        train.train_surrogate("fnn", d, train.FnnConfig(n_cases=3, batch_size=4), device="cuda", max_epochs=1, physics=_term(cfg, rec, fix))
