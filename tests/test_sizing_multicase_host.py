"""The multi-load-case sizing mode without a GPU: the extension header and the two entry points' refusals (all decided
on the host, before any HIP call), the host logic of openpystruct_amd/multicase.py, the numpy reference of the design step against
the single-case one, the group-gradient identity against autograd of the design objective, and what `dataprep.prepare` makes of
grouped records."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import sizing_multicase_ref as mr  # noqa: E402
from tests import sizing_step_cases as sc  # noqa: E402
from tests import sizing_total_ref as tr  # noqa: E402
from tests.beam_dense import random_case  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from openpystruct_amd import _cabi
    return _cabi.load()


# ---------------------------------------------------------------------------------------------------------------------
# header and library
# ---------------------------------------------------------------------------------------------------------------------
def test_header_is_an_extension_and_not_the_last():
    from openpystruct_amd import _cabi
    names = [os.path.basename(p) for p in _cabi.EXTENSION_HEADER_PATHS]
    assert "openpystruct_amd_sizing_multicase.h" in names[:-1]
    assert {"ops_beam_sizing_step_multicase_f32", "ops_beam_sizing_multicase_max_cases"} <= set(_cabi.EXTENSION_EXPORTS)
    ext = _cabi._extensions[_cabi.EXTENSION_HEADER_PATHS[names.index("openpystruct_amd_sizing_multicase.h")]]
    assert set(ext.functions) == {"ops_beam_sizing_step_multicase_f32", "ops_beam_sizing_multicase_max_cases"}
    assert not ext.structs and not ext.defines
    restype, argtypes = ext.functions["ops_beam_sizing_step_multicase_f32"]
    assert restype is ctypes.c_int and len(argtypes) == 24
    assert argtypes[:3] == [ctypes.c_int] * 3 and argtypes[10] is ctypes.c_int


def test_both_symbols_are_exported_and_bound(lib):
    step = lib.ops_beam_sizing_step_multicase_f32
    assert step.restype is ctypes.c_int and len(step.argtypes) == 24
    assert lib.ops_beam_sizing_multicase_max_cases.argtypes == []
    assert lib.ops_beam_sizing_multicase_max_cases() >= 16


def test_package_exports():
    import openpystruct_amd as oa
    from openpystruct_amd import multicase
    assert oa.optimize_designs is multicase.optimize_designs and oa.generate_multicase_dataset is multicase.generate_multicase_dataset
    assert {"optimize_designs", "generate_multicase_dataset"} <= set(oa.__all__)


# argument positions of ops_beam_sizing_step_multicase_f32
ARGS = ("G", "C", "Ne", "I", "I64_rows", "V", "M", "grad", "loss_extra", "weights", "aggregate", "exp_avg", "exp_avg_sq", "best_loss",
        "patience_cnt", "epochs_run", "active", "active_rows", "last_loss", "case_penalty", "governing", "hp", "schedule", "stream")
REQUIRED = ("I", "I64_rows", "V", "M", "grad", "exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active",
            "active_rows", "last_loss", "hp")


def _host_args(params, **override):
    """An argument list whose pointers are host addresses of a guard buffer: a refusal never reads or writes through them."""
    guard = (ctypes.c_ubyte * 64)(*([0xA5] * 64))
    p = ctypes.addressof(guard)
    a = dict(G=2, C=3, Ne=5, I=p, I64_rows=p, V=p, M=p, grad=p, loss_extra=None, weights=None, aggregate=0, exp_avg=p, exp_avg_sq=p,
             best_loss=p, patience_cnt=p, epochs_run=p, active=p, active_rows=p, last_loss=p, case_penalty=None, governing=None,
             hp=ctypes.byref(params), schedule=None, stream=None)
    assert tuple(a) == ARGS
    a.update(override)
    return guard, list(a.values())


def test_every_refusal_is_decided_on_the_host(lib):
    from openpystruct_amd import _cabi
    hp = sc.beam_hp()
    p = ctypes.addressof((ctypes.c_ubyte * 8)())
    refusals = [({k: None}, _cabi.ERR_INVALID_ARG) for k in REQUIRED]
    refusals += [({"G": -1}, _cabi.ERR_INVALID_ARG), ({"C": 0}, _cabi.ERR_INVALID_ARG), ({"C": -2}, _cabi.ERR_INVALID_ARG),
                 ({"Ne": 0}, _cabi.ERR_INVALID_ARG), ({"Ne": -1}, _cabi.ERR_INVALID_ARG),
                 ({"aggregate": 2}, _cabi.ERR_INVALID_ARG), ({"aggregate": -1}, _cabi.ERR_INVALID_ARG),
                 ({"aggregate": 1, "weights": p}, _cabi.ERR_INVALID_ARG),
                 ({"Ne": 513}, _cabi.ERR_UNSUPPORTED), ({"C": lib.ops_beam_sizing_multicase_max_cases() + 1}, _cabi.ERR_UNSUPPORTED)]
    for override, want in refusals:
        guard, args = _host_args(hp, **override)
        assert lib.ops_beam_sizing_step_multicase_f32(*args) == want, override
        assert bytes(guard) == b"\xa5" * 64, override
    # G == 0: OK, whatever the pointers
    guard, args = _host_args(hp, G=0)
    assert lib.ops_beam_sizing_step_multicase_f32(*args) == _cabi.OK
    guard, args = _host_args(hp, G=0, I=None, grad=None)
    assert lib.ops_beam_sizing_step_multicase_f32(*args) == _cabi.OK and bytes(guard) == b"\xa5" * 64


# ---------------------------------------------------------------------------------------------------------------------
# host logic
# ---------------------------------------------------------------------------------------------------------------------
def _cases(n, **cfg_kw):
    from openpystruct_amd import sizing
    cfg = sizing.SizingConfig(num_nodes=21, roller_nodes=(7, 14, 21), max_e=5, **cfg_kw)
    return cfg, sizing.make_cases(n, cfg, seed=3, device="cpu")


def test_check_design_groups():
    from openpystruct_amd import multicase, sizing
    cfg, cases = _cases(6)
    assert multicase.check_design_groups(cases, 3) == 2 and multicase.check_design_groups(cases, 1) == 6
    with pytest.raises(ValueError, match="design 1 "):            # ragged: 6 = 1 * 4 + 2
        multicase.check_design_groups(cases, 4)
    with pytest.raises(ValueError):
        multicase.check_design_groups(cases, 0)
    fix = cases.fix.clone()
    fix[4, 3] = 1                                                 # row 4 = case 1 of design 1
    other = sizing.Cases(*(fix if t is cases.fix else t for t in cases.tensors()))
    with pytest.raises(ValueError, match="design 1: .* fix"):
        multicase.check_design_groups(other, 3)
    assert multicase.check_design_groups(other, 1) == 6           # every row its own design: nothing to share
    xs = cases.node_positions.clone()
    xs[2, 5] += 0.25
    other = sizing.Cases(*(xs if t is cases.node_positions else t for t in cases.tensors()))
    with pytest.raises(ValueError, match="design 0: .* node_positions"):
        multicase.check_design_groups(other, 3)


def test_make_design_cases_shares_the_first_rows_bridge():
    from openpystruct_amd import multicase, sizing
    cfg = sizing.SizingConfig(num_nodes=21, random_bridge=1, max_e=5)
    plain = sizing.make_cases(8, cfg, seed=5, device="cpu")
    cases = multicase.make_design_cases(2, 4, cfg, seed=5, device="cpu")
    assert multicase.check_design_groups(cases, 4) == 2
    for g in range(2):
        for c in range(4):
            r = 4 * g + c
            for name in ("node_positions", "L", "roller_nodes_t", "n_rollers", "fix"):
                assert torch.equal(getattr(cases, name)[r], getattr(plain, name)[4 * g]), (name, r)
            for name in ("force_nodes_t", "n_forces", "force_values_t", "Fy"):        # the draws stay in the record
                assert torch.equal(getattr(cases, name)[r], getattr(plain, name)[r]), (name, r)
    fixed = sizing.SizingConfig(num_nodes=21, roller_nodes=(7, 14, 21))
    a, b = multicase.make_design_cases(2, 3, fixed, seed=5), sizing.make_cases(6, fixed, seed=5)
    assert all(torch.equal(s, t) for s, t in zip(a.tensors(), b.tensors()))


def test_optimize_designs_refusals():
    from openpystruct_amd import multicase
    cfg, cases = _cases(6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        multicase.optimize_designs(cases, cfg, "cpu", 3)
    with pytest.raises(ValueError, match="weights"):
        multicase.optimize_designs(cases, cfg, "cpu", 3, aggregate="max", weights=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="aggregate"):
        multicase.optimize_designs(cases, cfg, "cpu", 3, aggregate="mean")
    with pytest.raises(ValueError, match="deflection_limit"):
        multicase.optimize_designs(cases, cfg, "cpu", 3, alpha_deflection=100.0)
    with pytest.raises(ValueError, match="deflection_limit"):
        multicase.optimize_designs(cases, cfg, "cpu", 3, alpha_deflection=100.0, deflection_limit=0.0)
    with pytest.raises(ValueError, match="alpha_deflection"):
        multicase.optimize_designs(cases, cfg, "cpu", 3, alpha_deflection=-1.0, deflection_limit=0.01)


# ---------------------------------------------------------------------------------------------------------------------
# the numpy reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("G,Ne", [(1, 1), (5, 65), (9, 100)])
def test_reference_with_one_case_is_the_single_case_reference(G, Ne, with_extra):
    hp = sc.beam_hp()
    I, m, v, V, M, grad, extra = mr.design_inputs(G, 1, Ne, 0)
    extra = extra if with_extra else None
    rng = np.random.default_rng(G)
    t, cnt = rng.integers(0, 20, size=G), rng.integers(0, 4, size=G)
    best = rng.uniform(10.0, 1e4, size=G).astype(np.float32)
    got = mr.design_step_reference(I, m, v, V, M, grad, extra, None, mr.SUM, t, best, cnt, hp)
    want = tr.step_grad_reference(I, m, v, V[:, 0], M[:, 0], grad[:, 0], None if extra is None else extra[:, 0], t, best, cnt, hp)
    for k, a in want.items():
        assert np.array_equal(got[k], a), k
    assert (got["governing"] == 0).all() and got["case_penalty"].shape == (G, 1)
    one = mr.design_step_reference(I, m, v, V, M, grad, extra, np.ones(1), mr.SUM, t, best, cnt, hp)
    for k, a in want.items():
        assert np.array_equal(one[k], a), k


def test_reference_worst_case_picks_the_lowest_index_of_a_tie():
    hp = sc.beam_hp()
    I, m, v, V, M, grad, _ = mr.design_inputs(2, 3, 7, 1)
    V[:, 2], M[:, 2] = V[:, 0], M[:, 0]                  # cases 0 and 2 tie exactly
    V[:, 1], M[:, 1] = 0.5 * V[:, 0], 0.5 * M[:, 0]
    z = np.zeros(2, dtype=np.int64)
    r = mr.design_step_reference(I, m, v, V, M, grad, None, None, mr.MAX, z, np.full(2, np.inf), z, hp)
    assert (r["governing"] == 0).all() and np.array_equal(r["case_penalty"][:, 0], r["case_penalty"][:, 2])
    assert np.array_equal(r["mag"], np.abs(grad[:, 0].astype(np.float32).astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------------
# the group gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deflection", [False, True])
@pytest.mark.parametrize("mode", ["sum", "sum+weights", "max"])
def test_group_gradient_is_autograd_of_the_design_objective(mode, deflection):
    """Ne = 13, C = 3: the identity the kernel uses -- sum_c w_c grad_c - (sum_c w_c - 1), or the governing row -- from the per-row
    total gradients (each row its own leaf, as the gradient kernel sees them) against autograd of the design objective with ONE
    leaf shared by the three rows; float64 against float64, 1e-12 of the gradient's largest entry."""
    Ne, C = 13, 3
    hp = sc.beam_hp()
    rng = np.random.default_rng([Ne, C, 20250307])
    x, fix, I, Fy = random_case(rng, C, Ne)
    I = np.repeat(I[:1], C, axis=0)
    E, wy = 2e11, -750.0
    obj = tr.objective()
    if deflection:
        free = tr.total_gradient_ref(x, E, I, fix, Fy, wy, hp, obj)
        obj = tr.objective(100.0, 0.5 * float(np.abs(free.outs[0]).max(-1).min()))     # binding in every case
    rows = tr.total_gradient_ref(x, E, I, fix, Fy, wy, hp, obj)
    if deflection:
        assert (rows.loss_extra > 0).all()
    weights = np.array([0.5, 2.0, 1.25]) if mode == "sum+weights" else None
    aggregate = mr.MAX if mode == "max" else mr.SUM
    want = mr.design_autograd(x, E, I[0], fix, Fy, wy, hp, obj, weights, aggregate)
    P = rows.loss - I.sum(-1)
    assert np.allclose(P, want.P, rtol=1e-13, atol=0.0)
    got = mr.group_gradient(rows.grad, weights, aggregate, np.argmax(P))
    assert got.shape == (Ne,)
    err = float(np.abs(got - want.grad).max() / np.abs(want.grad).max())
    print(mode, deflection, "group gradient against autograd:", err)
    assert err <= 1e-12, err
    if aggregate == mr.MAX:
        assert int(np.argmax(P)) == want.governing
        second = np.sort(P)[-2]
        assert P.max() > 1.001 * second                     # no tie: the subgradient is the governing row's gradient


# ---------------------------------------------------------------------------------------------------------------------
# dataprep on grouped records
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pinn", "tfd"])
def test_dataprep_labels_grouped_records_with_the_design(kind):
    """Rows of a group share I_values: `unify_label_with_c` (mean + 0.5 std over the group) then IS the design.  The mean of C equal
    float32 numbers is off by at most C / 2 eps32 (relative), the population std by as much, and the standardisation round trip by a
    few eps32 of |mean| + |scale|: 32 eps32 of the largest inertia bounds them all for C = 6."""
    from openpystruct_amd import dataprep
    G, C, Ne, N = 10, 6, 12, 13
    rng = np.random.default_rng(4)
    I = np.exp(rng.uniform(np.log(1e-3), np.log(0.75), size=(G, Ne))).astype(np.float32)
    rec = {"roller_x_locations": torch.as_tensor(rng.uniform(0, 200, size=(G * C, 3))),
           "force_x_locations": torch.as_tensor(rng.uniform(0, 200, size=(G * C, 4))),
           "force_values": torch.as_tensor(rng.uniform(-3e5, -3e4, size=(G * C, 4))),
           "node_positions": torch.linspace(0, 200, N, dtype=torch.float64).expand(G * C, -1).contiguous(),
           "I_values": torch.as_tensor(np.repeat(I, C, axis=0)),
           "deflections": torch.as_tensor(rng.standard_normal((G * C, N))), "rotations": torch.as_tensor(rng.standard_normal((G * C, N))),
           "num_nodes": N}
    perm = torch.arange(G)
    d = dataprep.prepare(rec, kind=kind, n_cases=C, perm=perm, train_split=0.8)
    sy = d.scalers_Y["I"]
    labels = torch.cat([sy.inverse_transform(d.Y_train[:, :Ne]), sy.inverse_transform(d.Y_val[:, :Ne])]).numpy()
    assert labels.shape == (G, Ne)
    assert np.abs(labels.astype(np.float64) - I).max() <= 32 * sc.EPS32 * float(I.max())
    # the heuristic it replaces, on separately sized cases, is NOT any one of their designs
    apart = torch.as_tensor(rng.uniform(0.1, 0.5, size=(1, C, Ne)))
    assert not any(torch.allclose(dataprep.unify_label_with_c(apart)[0], apart[0, c]) for c in range(C))
