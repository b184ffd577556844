"""The design-objective term without a GPU: the extension header, the exported symbols, the package's exports and
every refusal of the two entry points -- all decided on the host, before any HIP call, with nothing written -- and the host-side
checks of openpystruct_amd/design_loss.py."""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import sizing_step_cases as sc  # noqa: E402

HEADER = "openpystruct_amd_design_loss.h"
FUNCTIONS = {"ops_design_loss_prep", "ops_design_loss_finish", "ops_design_loss_max_cases", "ops_design_loss_part_doubles"}


@pytest.fixture(scope="module")
def lib():
    from openpystruct_amd import _cabi
    return _cabi.load()


def test_header_is_an_extension_and_not_the_last():
    from openpystruct_amd import _cabi
    names = [os.path.basename(p) for p in _cabi.EXTENSION_HEADER_PATHS]
    assert HEADER in names[:-1] and names[-1] == "openpystruct_amd_sizing_grad.h"
    assert FUNCTIONS <= set(_cabi.EXTENSION_EXPORTS)
    ext = _cabi._extensions[_cabi.EXTENSION_HEADER_PATHS[names.index(HEADER)]]
    assert set(ext.functions) == FUNCTIONS
    assert set(ext.structs) == {"ops_design_loss_args"} and not ext.defines
    restype, argtypes = ext.functions["ops_design_loss_finish"]
    assert restype is ctypes.c_int and len(argtypes) == 3
    assert argtypes[0] == ctypes.POINTER(_cabi.DesignLossArgs) and argtypes[1] == ctypes.POINTER(_cabi.SizingParams)
    fields = dict(_cabi.DesignLossArgs._fields_)
    assert fields["B"] is ctypes.c_int and fields["ldp"] is ctypes.c_long and fields["weight"] is ctypes.c_float
    assert fields["alpha_deflection"] is ctypes.c_double and fields["dpreds"] is ctypes.c_void_p


def test_the_symbols_are_exported_and_bound(lib):
    assert lib.ops_design_loss_prep.restype is ctypes.c_int and len(lib.ops_design_loss_prep.argtypes) == 2
    assert lib.ops_design_loss_finish.restype is ctypes.c_int and len(lib.ops_design_loss_finish.argtypes) == 3
    assert lib.ops_design_loss_max_cases.argtypes == [] and lib.ops_design_loss_max_cases() >= 64
    assert lib.ops_design_loss_part_doubles(0) == 0 and lib.ops_design_loss_part_doubles(7) >= 1


def test_package_exports():
    import openpystruct_amd as oa
    from openpystruct_amd import design_loss
    for name in ("DesignObjective", "design_objective", "design_objective_term", "design_gap"):
        assert getattr(oa, name) is getattr(design_loss, name) and name in oa.__all__
    from openpystruct_amd import train
    assert {"weight", "x", "E", "fix", "wy", "hp", "aggregate", "weights", "alpha_deflection", "deflection_limit", "normalise"} \
        == set(train.DesignTerm.__dataclass_fields__)
    assert train.DesignTerm.__dataclass_fields__["normalise"].default is True


PREP_REQUIRED = ("preds", "I_scale", "I_mean", "I_rows", "Fy_src", "Fy_rows")
FINISH_REQUIRED = ("I_rows", "V", "M", "grad")


def _host_args(**override):
    """An argument struct whose pointers are host addresses of a guard buffer: a refusal never reads or writes through them."""
    from openpystruct_amd import _cabi
    guard = (ctypes.c_ubyte * 64)(*([0xA5] * 64))
    p = ctypes.addressof(guard)
    a = dict(B=2, C=3, Ne=5, G=2, aggregate=0, preds_bf16=0, ldp=5, preds=p, I_scale=p, I_mean=p, I_min=1e-8, weight=1.0,
             alpha_deflection=0.0, deflection_limit=0.0, rows=None, Fy_src=p, ref=None, weights=None, I_rows=p, Fy_rows=p, V=p, M=p,
             grad=p, loss_extra=None, status_solve=p, status_grad=p, sample_loss=p, gI=p, case_penalty=p, governing=p, dpreds=p,
             part=p, value=p, value_sum=None)
    a.update(override)
    return guard, _cabi.DesignLossArgs(**a)


def test_every_refusal_is_decided_on_the_host(lib):
    from openpystruct_amd import _cabi
    hp = sc.beam_hp()
    p = ctypes.addressof((ctypes.c_ubyte * 8)())
    INV, UNS = _cabi.ERR_INVALID_ARG, _cabi.ERR_UNSUPPORTED
    both = [({"B": -1}, INV), ({"C": 0}, INV), ({"C": -2}, INV), ({"Ne": 0}, INV), ({"Ne": -1}, INV), ({"G": -1}, INV),
            ({"aggregate": 2}, INV), ({"aggregate": -1}, INV), ({"aggregate": 1, "weights": p}, INV),
            ({"Ne": 513, "ldp": 513}, UNS), ({"Ne": 514, "ldp": 514}, UNS), ({"C": lib.ops_design_loss_max_cases() + 1}, UNS),
            ({"ldp": 4}, INV), ({"G": 1}, INV), ({"G": 0, "rows": p}, INV)]
    prep = both + [({k: None}, INV) for k in PREP_REQUIRED]
    finish = both + [({k: None}, INV) for k in FINISH_REQUIRED] + [
        ({"alpha_deflection": 1.0}, INV), ({"alpha_deflection": 1.0, "deflection_limit": 0.1}, INV),        # no loss_extra
        ({"alpha_deflection": 1.0, "deflection_limit": 0.0, "loss_extra": p}, INV), ({"alpha_deflection": -1.0}, INV),
        ({"preds": None}, INV), ({"I_scale": None}, INV), ({"part": None}, INV), ({"value": None, "value_sum": p}, INV)]
    for override, want in prep:
        guard, a = _host_args(**override)
        assert lib.ops_design_loss_prep(ctypes.byref(a), None) == want, override
        assert bytes(guard) == b"\xa5" * 64, override
    for override, want in finish:
        guard, a = _host_args(**override)
        assert lib.ops_design_loss_finish(ctypes.byref(a), ctypes.byref(hp), None) == want, override
        assert bytes(guard) == b"\xa5" * 64, override
    guard, a = _host_args()
    assert lib.ops_design_loss_finish(ctypes.byref(a), None, None) == INV and bytes(guard) == b"\xa5" * 64
    assert lib.ops_design_loss_prep(None, None) == INV and lib.ops_design_loss_finish(None, ctypes.byref(hp), None) == INV
    # B == 0: OK, whatever the pointers, nothing enqueued
    guard, a = _host_args(B=0, G=0, preds=None, I_rows=None, V=None)
    assert lib.ops_design_loss_prep(ctypes.byref(a), None) == _cabi.OK
    assert lib.ops_design_loss_finish(ctypes.byref(a), ctypes.byref(hp), None) == _cabi.OK and bytes(guard) == b"\xa5" * 64


def test_the_python_entries_refuse_cpu_tensors_and_bad_settings():
    from openpystruct_amd import design_loss, sizing
    cfg = sizing.SizingConfig(num_nodes=6)
    I = torch.full((2, 5), 0.5, dtype=torch.float64)
    x, fix, Fy = torch.linspace(0, 5, 6, dtype=torch.float64), torch.zeros(6, dtype=torch.uint8), torch.zeros((2, 1, 6), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        design_loss.design_objective(I, x, cfg.E, fix, Fy, -1000.0, cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        design_loss.design_objective_term(torch.zeros((2, 5)), 5, None, None, Fy, x, cfg.E, fix, -1000.0, cfg, 1.0)
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="aggregate"):
        design_loss._checked("mean", None, 2, 0.0, None, dev)
    with pytest.raises(ValueError, match="no weights"):
        design_loss._checked("max", [1.0, 1.0], 2, 0.0, None, dev)
    with pytest.raises(ValueError, match="deflection_limit"):
        design_loss._checked("sum", None, 2, 1.0, None, dev)
    with pytest.raises(ValueError, match="n_load_cases"):
        design_loss._checked("sum", None, 65, 0.0, None, dev)
    with pytest.raises(ValueError, match="weights"):
        design_loss._checked("sum", [1.0, -1.0], 2, 0.0, None, dev)
    assert design_loss._checked("max", None, 2, 0.5, 0.01, dev) == (1, None, 0.5, 0.01)
    with pytest.raises(ValueError, match="shared by the batch"):
        design_loss._shared(x.repeat(2, 1), fix, cfg.E, -1000.0, 5, dev)
