"""Multi-load-case frame sizing, what needs no GPU: the extension header and its place in the binding and the build,
the package's exports, the refusals the C entries decide before any HIP call, the argument checks of the Python entries (shape and
dtype: ValueError; then anything but a GPU tensor: RuntimeError), and on the CPU the aggregation identity the design step relies
on: the per-case gradients, aggregated as the kernel aggregates them, are autograd of the design objective with ONE leaf I."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "openpystruct_amd_frame_designs.h"
ENTRIES = {"ops_frame_design_rhs_f64", "ops_frame_design_step_f32", "ops_frame_design_max_cases"}


def test_header_is_an_extension_and_changes_no_version():
    from openpystruct_amd import _cabi, build
    names = [os.path.basename(p) for p in _cabi.EXTENSION_HEADER_PATHS]
    assert HEADER in names
    ext = _cabi._extensions[_cabi.EXTENSION_HEADER_PATHS[names.index(HEADER)]]
    assert set(ext.functions) == ENTRIES and not ext.structs and not ext.defines
    assert ENTRIES <= set(_cabi.EXTENSION_EXPORTS) and not ENTRIES & set(_cabi.EXPORTS)
    i, p = ctypes.c_int, ctypes.c_void_p
    hp, obj = ctypes.POINTER(_cabi.SizingParams), ctypes.POINTER(_cabi.FrameSizingObjective)
    assert ext.functions["ops_frame_design_max_cases"] == (i, [])
    restype, argtypes = ext.functions["ops_frame_design_rhs_f64"]
    assert restype is i and argtypes == [i] * 4 + [p] * 9 + [hp, obj] + [p] * 4
    # the rows entry it mirrors, with C behind G
    rows = _cabi._extensions[_cabi.EXTENSION_HEADER_PATHS[names.index("openpystruct_amd_frame_sizing.h")]].functions["ops_frame_sizing_rhs_f64"]
    assert argtypes == rows[1][:1] + [i] + rows[1][1:]
    restype, argtypes = ext.functions["ops_frame_design_step_f32"]
    assert restype is i and argtypes == [i] * 4 + [p] * 13 + [i] + [p] * 10 + [hp, p, p]
    deps = {os.path.relpath(q, ROOT) for s in build.SOURCES for q in build._deps(s)}      # every file the build watches
    assert os.path.join("include", HEADER) in deps and os.path.join("openpystruct_amd", "csrc", "frame_designs_math.hpp") in deps
    src = os.path.join(ROOT, "openpystruct_amd", "csrc", "frame_designs.hip")
    assert src in build.SOURCES
    scanned = build._deps(src)
    for name in ("frame_designs_math.hpp", "frame_sizing_math.hpp", "sizing_multicase_math.hpp", "frame_stream.hpp"):
        assert os.path.normpath(os.path.join(ROOT, "openpystruct_amd", "csrc", name)) in scanned, name
    assert os.path.normpath(os.path.join(ROOT, "include", HEADER)) in scanned


def test_package_exports():
    import openpystruct_amd as oa
    from openpystruct_amd import frame_designs
    for name in ("FrameDesigns", "optimize_frame_designs", "frame_design_gradient", "generate_frame_design_dataset"):
        assert getattr(oa, name) is getattr(frame_designs, name) and name in oa.__all__
    assert frame_designs.FrameDesigns._fields == ("I", "solution", "epochs", "governing", "case_penalty")


def test_refusals_are_decided_before_any_device_call():
    """No GPU here: an entry that returns its refusal has not made a HIP call.  Every pointer is one host buffer that no refusal
    may read or write (the parameters and the objective apart: real structs)."""
    from openpystruct_amd import _cabi, frames
    lib = _cabi.load()
    assert lib.ops_frame_design_max_cases() == 64
    buf = ctypes.create_string_buffer(b"\xa5" * 256, 256)
    p = ctypes.addressof(buf)
    hp = frames._sizing_params(frames.FrameConfig())
    free = _cabi.FrameSizingObjective(alpha_sway=0.0, sway_limit=0.0, alpha_deflection=0.0, deflection_limit=0.0)
    hinge = _cabi.FrameSizingObjective(alpha_sway=1.0, sway_limit=1e-3, alpha_deflection=0.0, deflection_limit=0.0)

    def rhs(G=5, C=3, Nn=4, Ne=3, objective=free, **null):
        a = dict(geo=p, EA=p, E=p, ptr=p, idx=p, I64=p, disp=p, V=p, M=p, hp=ctypes.byref(hp), obj=ctypes.byref(objective), active=p, rhs=p, extra=p)
        a.update({k: None for k in null})
        return lib.ops_frame_design_rhs_f64(G, C, Nn, Ne, *a.values(), None)

    def step(G=5, C=3, Nn=4, Ne=3, aggregate=0, weights=None, **null):
        a = dict(geo=p, E=p, conn=p, I=p, I64=p, disp=p, V=p, M=p, lam=p, extra=p, st_fwd=p, st_adj=p, weights=weights, aggregate=aggregate,
                 exp_avg=p, exp_avg_sq=p, best=p, cnt=p, epochs=p, active=p, last=p, penalty=p, governing=p, grad_out=p,
                 hp=ctypes.byref(hp), schedule=p)
        a.update({k: None for k in null})
        return lib.ops_frame_design_step_f32(G, C, Nn, Ne, *a.values(), None)

    for call in (rhs, step):
        for kw in (dict(G=-1), dict(C=0), dict(C=-2), dict(Nn=1), dict(Nn=-4), dict(Ne=0), dict(Ne=-3)):
            assert call(**kw) == _cabi.ERR_INVALID_ARG, (call.__name__, kw)
        assert call(Ne=513) == _cabi.ERR_UNSUPPORTED and call(C=65) == _cabi.ERR_UNSUPPORTED and call(Ne=512, C=64, G=0) == _cabi.OK
        assert call(G=0) == _cabi.OK and call(G=0, geo=True) == _cabi.OK
    for k in ("geo", "EA", "E", "ptr", "idx", "I64", "disp", "V", "M", "hp", "obj", "rhs"):
        assert rhs(**{k: True}) == _cabi.ERR_INVALID_ARG, k
    assert rhs(objective=hinge, extra=True) == _cabi.ERR_INVALID_ARG          # a hinge needs loss_extra
    for bad in (dict(alpha_sway=1.0, sway_limit=0.0), dict(alpha_sway=-1.0, sway_limit=1e-3), dict(alpha_deflection=2.0, deflection_limit=-1.0),
                dict(alpha_deflection=float("nan"), deflection_limit=1e-3)):
        o = _cabi.FrameSizingObjective(**{**dict(alpha_sway=0.0, sway_limit=0.0, alpha_deflection=0.0, deflection_limit=0.0), **bad})
        assert rhs(objective=o) == _cabi.ERR_INVALID_ARG, bad
    for k in ("geo", "E", "conn", "I", "I64", "disp", "V", "M", "lam", "exp_avg", "exp_avg_sq", "best", "cnt", "epochs", "active", "last", "hp"):
        assert step(**{k: True}) == _cabi.ERR_INVALID_ARG, k
    assert step(aggregate=2) == _cabi.ERR_INVALID_ARG and step(aggregate=-1) == _cabi.ERR_INVALID_ARG
    assert step(aggregate=1, weights=p) == _cabi.ERR_INVALID_ARG        # the worst case takes no weights
    assert buf.raw == b"\xa5" * 256                                     # nothing written


def test_python_entries_check_shapes_then_devices():
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    topo = frames.grid_frame(1, 1, device="cpu")
    G, C = 2, 3
    f64 = dict(dtype=torch.float64)
    loads, w = torch.zeros((G, C, topo.Nn, 3), **f64), torch.zeros((G, C, topo.Ne, 2), **f64)
    I0 = torch.full((G, topo.Ne), 5e-4)
    # shapes and dtypes first, on CPU tensors
    for bad in (loads[..., :2], loads.float(), loads[0, 0], loads.numpy()):
        with pytest.raises(ValueError, match="loads must be"):
            oa.optimize_frame_designs(topo, bad, n_designs=G)
    with pytest.raises(ValueError, match="n_designs or I0"):
        oa.optimize_frame_designs(topo, loads[0])
    with pytest.raises(ValueError, match="n_designs"):
        oa.optimize_frame_designs(topo, loads, n_designs=G + 1)
    for bad in (w[:, :2], w[:1], w.float(), w[..., :1]):
        with pytest.raises(ValueError, match="element_loads"):
            oa.optimize_frame_designs(topo, loads, bad)
    with pytest.raises(ValueError, match="I0 must be"):
        oa.optimize_frame_designs(topo, loads, I0=I0[:, :-1])
    for kw in (dict(weights=(1.0, 1.0)), dict(weights=(1.0, -1.0, 1.0)), dict(weights=(1.0, float("nan"), 1.0)),
               dict(aggregate="max", weights=(1.0, 1.0, 1.0)), dict(aggregate="mean"), dict(alpha_sway=1.0), dict(alpha_deflection=-1.0),
               dict(alpha_sway=1.0, sway_limit=0.0)):
        with pytest.raises(ValueError):
            oa.optimize_frame_designs(topo, loads, **kw)
    with pytest.raises(ValueError, match="load cases"):
        oa.optimize_frame_designs(topo, torch.zeros((1, 65, topo.Nn, 3), **f64))
    big = frames.grid_frame(16, 16, device="cpu", numbering="node")
    assert big.Ne == 528
    with pytest.raises(ValueError, match="512"):
        oa.optimize_frame_designs(big, torch.zeros((1, 2, big.Nn, 3), **f64))
    wide = frames.grid_frame(17, 2, device="cpu", numbering="node")
    assert wide.kd == 56
    with pytest.raises(ValueError, match="frame_factor does not serve.*half bandwidth <= 55"):
        oa.optimize_frame_designs(wide, torch.zeros((1, 2, wide.Nn, 3), **f64))
    # then where the tensors live
    for args in ((loads,), (loads, w), (loads[0], w[0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            oa.optimize_frame_designs(topo, *args, n_designs=G)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.optimize_frame_designs(topo, loads, I0=I0, aggregate="max")

    # frame_design_gradient on a factor as frame_factor would have made it, on the CPU: only the checks can run
    I = torch.full((G, topo.Ne), 5e-4, **f64)
    sol0 = frames.FrameSolution(torch.zeros((G, topo.Nn, 3), **f64), torch.zeros((G, topo.Ne, 6), **f64), torch.zeros((G, topo.Ne), **f64),
                                torch.zeros((G, topo.Ne), **f64), torch.zeros((G,), dtype=torch.int32))
    fac = frames.FrameFactor(topo, I, torch.zeros(16, dtype=torch.uint8), sol0)
    case = frames.FrameCaseSolution(torch.zeros((G, C, topo.Nn, 3), **f64), torch.zeros((G, C, topo.Ne, 6), **f64),
                                    torch.zeros((G, C, topo.Ne), **f64), torch.zeros((G, C, topo.Ne), **f64),
                                    torch.zeros((G, C), dtype=torch.int32))
    cfg = frames.FrameConfig()
    for bad in (case._replace(disp=case.disp[:, :2]), case._replace(V=case.V.float()), case._replace(M=case.M[:1]),
                case._replace(status=case.status[:, :2]), case._replace(disp=case.disp[..., :2])):
        with pytest.raises(ValueError, match="sol\\."):
            oa.frame_design_gradient(fac, bad, cfg)
    for kw in (dict(weights=(1.0, 2.0)), dict(aggregate="max", weights=(1.0, 1.0, 1.0)), dict(aggregate="worst"), dict(alpha_deflection=1.0)):
        with pytest.raises(ValueError):
            oa.frame_design_gradient(fac, case, cfg, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_design_gradient(fac, case, cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_design_gradient(fac, case, cfg, aggregate="max", alpha_sway=1.0, sway_limit=1e-3)


@pytest.mark.parametrize("hinges", [False, True])
@pytest.mark.parametrize("frame", ["1x1", "2x3"])
def test_aggregated_case_gradients_are_the_gradient_of_the_design_objective(frame, hinges):
    """What ops_frame_design_step_f32 steps on: sum_c w_c grad_c - (sum_c w_c - 1), and grad_c* for "max", with grad_c = 1 + dP_c/dI
    of every (design, case) row taken on its own (the rows gradient of §9h), against autograd of the design objective with ONE leaf
    I per design; C = 3, to 1e-9 relative to the size of the terms the gradient is a sum of (`grad_scale` of the rows)."""
    from openpystruct_amd import frames
    from tests import frame_dense as fd
    from tests import frame_designs_ref as dr
    from tests import frame_sizing_total_ref as ft
    from tests import sizing_multicase_ref as mr
    bays, stories = (int(v) for v in frame.split("x"))
    topo = frames.grid_frame(bays, stories, device="cpu")
    case = fd.case_of(topo)
    G, C = 4, 3
    rng = np.random.default_rng(31 + bays)
    I = fd.random_inertias(rng, G, topo.Ne)
    H, q = rng.uniform(0.5e4, 2e4, size=G), rng.uniform(-2e4, -0.5e4, size=G)
    loads, w = frames.grid_load_cases(topo, np.stack([H, -H, 0 * H], 1).reshape(-1), np.stack([q, q, 1.5 * q], 1).reshape(-1))
    loads, w = loads.numpy().reshape(G, C, topo.Nn, 3), w.numpy().reshape(G, C, topo.Ne, 2)
    hp = ft.frame_hp()
    I_rows = np.repeat(I, C, axis=0)
    free = dr.rows_gradient(case, I_rows, loads.reshape(G * C, topo.Nn, 3), w.reshape(G * C, topo.Ne, 2), hp, ft.objective())
    obj = ft.objective()
    if hinges:        # half the forward's own largest |ux| and |uy|: both hinges active on some nodes and inactive on others
        obj = ft.objective(3.0, 0.5 * np.abs(free.outs[0][..., 0]).max(), 2.0, 0.5 * np.abs(free.outs[0][..., 1]).max())
    rows = dr.rows_gradient(case, I_rows, loads.reshape(G * C, topo.Nn, 3), w.reshape(G * C, topo.Ne, 2), hp, obj)
    assert not hinges or (rows.loss_extra > 0).sum() >= G * C - 2      # (the limits are the batch's: a row may stay below both)
    scale = ft.grad_scale(case, rows, rows.lam)
    grad_rows = rows.grad.reshape(G, C, topo.Ne)
    for aggregate, weights in ((dr.SUM, None), (dr.SUM, (1.0, 1.0, 0.5)), (dr.SUM, (0.25, 0.0, 2.0)), (dr.MAX, None)):
        want = dr.design_gradient(case, I, loads, w, hp, obj, aggregate, weights)
        got = mr.group_gradient(grad_rows, weights, aggregate, want.governing)
        err = float(np.linalg.norm(got - want.grad) / max(np.linalg.norm(want.grad), scale))
        print(f"{frame} hinges {hinges} aggregate {aggregate} weights {weights}: {err:.3e}")
        assert err <= 1e-9, (aggregate, weights, err)
        if aggregate == dr.MAX:      # the governing case is no matter of round-off here, and not the same for every design or case 0 alone
            s = np.sort(want.P, axis=1)
            assert ((s[:, -1] - s[:, -2]) / s[:, -1]).min() > 1e-6
