"""Several load cases per frame on one kept factorisation, what needs no GPU: the extension header and its place
in the binding and the build, the refusals the C entries decide before any HIP call, the package's exports, and the argument checks
of the Python entries (shape and dtype: ValueError; anything but a GPU tensor: RuntimeError)."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "openpystruct_amd_frame_cases.h"
ENTRIES = {"ops_frame_factor_workspace_bytes", "ops_frame_factor_solve_f64", "ops_frame_resolve_f64"}


def test_header_is_an_extension_and_changes_no_version():
    from openpystruct_amd import _cabi, build
    names = [os.path.basename(p) for p in _cabi.EXTENSION_HEADER_PATHS]
    assert HEADER in names
    ext = _cabi._extensions[_cabi.EXTENSION_HEADER_PATHS[names.index(HEADER)]]
    assert set(ext.functions) == ENTRIES and not ext.structs and not ext.defines
    assert ENTRIES <= set(_cabi.EXTENSION_EXPORTS) and not ENTRIES & set(_cabi.EXPORTS)
    restype, argtypes = ext.functions["ops_frame_factor_workspace_bytes"]
    assert restype is ctypes.c_size_t and argtypes == [ctypes.c_int] * 3
    restype, argtypes = ext.functions["ops_frame_factor_solve_f64"]
    assert restype is ctypes.c_int and argtypes == _cabi._abi.functions["ops_frame_solve_batched_f64"][1]
    restype, argtypes = ext.functions["ops_frame_resolve_f64"]
    assert restype is ctypes.c_int and len(argtypes) == 23 and argtypes[:6] == [ctypes.c_int] * 6 and argtypes[13] is ctypes.c_long
    assert argtypes[21] is ctypes.c_size_t
    deps = {os.path.relpath(p, ROOT) for s in build.SOURCES for p in build._deps(s)}      # every file the build watches
    assert os.path.join("include", HEADER) in deps and os.path.join("openpystruct_amd", "csrc", "frame_resolve.hpp") in deps
    assert os.path.normpath(os.path.join(ROOT, "openpystruct_amd", "csrc", "frame_resolve.hpp")) in build._deps(
        os.path.join(ROOT, "openpystruct_amd", "csrc", "frame_solve.hip"))


def test_package_exports():
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    for name in ("FrameFactor", "FrameCaseSolution", "frame_factor", "frame_resolve", "frame_solve_cases", "frame_solve_cases_vjp"):
        assert getattr(oa, name) is getattr(frames, name) and name in oa.__all__
    assert frames.FrameCaseSolution._fields == frames.FrameSolution._fields


def test_refusals_are_decided_before_any_device_call():
    """No GPU here: an entry that returns its refusal has not made a HIP call."""
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    assert lib.ops_frame_factor_workspace_bytes(5, 66, 35) > 0
    per_frame = lib.ops_frame_factor_workspace_bytes(6, 66, 35) - lib.ops_frame_factor_workspace_bytes(5, 66, 35)
    assert per_frame == (66 + 4) * 36 * 8                                      # (n_eq + 4) columns of W = 36 doubles
    assert lib.ops_frame_factor_workspace_bytes(6, 78, 41) - lib.ops_frame_factor_workspace_bytes(5, 78, 41) == (78 + 4) * 52 * 8
    assert lib.ops_frame_factor_workspace_bytes(6, 102, 53) - lib.ops_frame_factor_workspace_bytes(5, 102, 53) == (102 + 4) * 56 * 8
    assert lib.ops_frame_factor_workspace_bytes(5, 108, 56) == 0 and lib.ops_frame_factor_workspace_bytes(5, 108, 55) > 0
    assert lib.ops_frame_factor_workspace_bytes(5, 6000, 35) == 0              # four waves' LDS beyond 160 KB
    assert lib.ops_frame_factor_workspace_bytes(0, 66, 35) == 0 and lib.ops_frame_factor_workspace_bytes(-1, 66, 35) == 0
    p = ctypes.addressof(ctypes.create_string_buffer(64))                      # non-NULL; never dereferenced by a refusal

    def factor(B=5, Nn=33, Ne=42, n_eq=66, kd=35, lbs=0, nbytes=1 << 40, ptr=p, last=p):
        return lib.ops_frame_factor_solve_f64(B, Nn, Ne, n_eq, kd, ptr, p, p, p, p, p, p, p, lbs, p, p, p, p, p, last, nbytes, None)

    def resolve(B=5, C=3, Nn=33, Ne=42, n_eq=66, kd=35, rbs=0, nbytes=1 << 40, ptr=p, last=p):
        return lib.ops_frame_resolve_f64(B, C, Nn, Ne, n_eq, kd, ptr, p, p, p, p, p, p, rbs, p, p, p, p, p, p, last, nbytes, None)

    for call in (factor, resolve):
        assert call(kd=56) == _cabi.ERR_UNSUPPORTED and call(n_eq=6000, Ne=4000, Nn=2100) == _cabi.ERR_UNSUPPORTED
        assert call(B=-1) == _cabi.ERR_INVALID_ARG and call(Nn=1) == _cabi.ERR_INVALID_ARG and call(Ne=0) == _cabi.ERR_INVALID_ARG
        assert call(n_eq=0) == _cabi.ERR_INVALID_ARG and call(kd=-1) == _cabi.ERR_INVALID_ARG
        assert call(ptr=None) == _cabi.ERR_INVALID_ARG and call(last=None) == _cabi.ERR_INVALID_ARG
        assert call(nbytes=1024) == _cabi.ERR_INVALID_ARG and call(Ne=4 * 66 + 65) == _cabi.ERR_INVALID_ARG
        assert call(B=0) == _cabi.OK and call(B=0, ptr=None) == _cabi.OK
    assert factor(lbs=5) == _cabi.ERR_INVALID_ARG
    assert resolve(C=-1) == _cabi.ERR_INVALID_ARG and resolve(rbs=33 * 3) == _cabi.ERR_INVALID_ARG and resolve(rbs=-1) == _cabi.ERR_INVALID_ARG
    assert resolve(C=0) == _cabi.OK and resolve(C=0, ptr=None) == _cabi.OK and resolve(kd=56, C=0) == _cabi.OK


def test_python_entries_check_shapes_then_devices():
    from openpystruct_amd import frames
    topo = frames.grid_frame(1, 1, device="cpu")
    B, C = 2, 3
    f64 = dict(dtype=torch.float64)
    I = torch.full((B, topo.Ne), 5e-4, **f64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.frame_factor(topo, I)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.frame_factor(topo, I.numpy())
    for bad in (I.float(), I[:, :-1], I[0]):
        with pytest.raises(ValueError, match="I must be"):
            frames.frame_factor(topo, bad)
    wide = frames.grid_frame(17, 2, device="cpu", numbering="node")
    assert wide.kd == 56
    with pytest.raises(ValueError, match="half bandwidth <= 55.*frame_solve"):
        frames.frame_factor(wide, _FakeGpu.of(torch.zeros((1, wide.Ne), **f64)))
    # a factor as frame_factor would have made it, on the CPU: only the checks can run
    sol0 = frames.FrameSolution(torch.zeros((B, topo.Nn, 3), **f64), torch.zeros((B, topo.Ne, 6), **f64), torch.zeros((B, topo.Ne), **f64),
                                torch.zeros((B, topo.Ne), **f64), torch.zeros((B,), dtype=torch.int32))
    fac = frames.FrameFactor(topo, I, torch.zeros(16, dtype=torch.uint8), sol0)
    assert fac.status is sol0.status and fac.I is I
    loads, w = torch.zeros((B, C, topo.Nn, 3), **f64), torch.zeros((B, C, topo.Ne, 2), **f64)
    for args in ((loads,), (loads[0],), (loads, w), (loads[0], w[0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            frames.frame_resolve(fac, *args)
    for bad in (loads[:1], loads[..., :2], loads.float(), loads[0, 0], loads.numpy()):
        with pytest.raises(ValueError, match="loads must be"):
            frames.frame_resolve(fac, bad)
    for bad in (w[:, :2], w[:1], w.float(), w[..., :1]):
        with pytest.raises(ValueError, match="element_loads"):
            frames.frame_resolve(fac, loads, bad)
    case = frames.FrameCaseSolution(torch.zeros((B, C, topo.Nn, 3), **f64), torch.zeros((B, C, topo.Ne, 6), **f64),
                                    torch.zeros((B, C, topo.Ne), **f64), torch.zeros((B, C, topo.Ne), **f64),
                                    torch.zeros((B, C), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.frame_solve_cases_vjp(fac, case)
    for kw in (dict(g_disp=case.disp[:, :2]), dict(g_forces=case.forces[..., :5]), dict(gV=case.V.float()), dict(gM=case.M[:1])):
        with pytest.raises(ValueError):
            frames.frame_solve_cases_vjp(fac, case, **kw)
    with pytest.raises(ValueError, match="sol.status"):
        frames.frame_solve_cases_vjp(fac, case._replace(status=case.status[:, :2]))
    assert np.array_equal(frames.FrameCaseSolution._fields, ("disp", "forces", "V", "M", "status"))


class _FakeGpu:
    """A CPU tensor that says it is on the GPU: lets `frame_factor` reach its shape limit without a device."""

    @staticmethod
    def of(t):
        class T(torch.Tensor):
            @property
            def is_cuda(self):
                return True
        return t.as_subclass(T)
