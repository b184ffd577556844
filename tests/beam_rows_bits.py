"""The cases behind tests/golden/beam_rows_parent_bits.npz (test code only): seeded inputs and one function that runs them on
the GPU and returns every output as raw bits.  tests/golden/make_beam_rows_parent_bits.py records them, and
tests/test_gpu_beam_rows_bits.py compares a later build with the record: trimming the rows kernel's instruction stream
(empty sides of the top reduction level, broadcasts, flags that multiply by exactly 1) must not move a bit of any beam whose
status is 0.

  a  9 x 100   the bench's bridge (rollers at nodes 10, 30, 70, 85, 100) and "trajectory" inertias; the third wave holds one beam
  b  5 x 37    one node with a fixed rotation (the RZ instantiation), odd Ne
  c  4 x 100   beam 2 has zero inertia on two adjacent elements: its factorisation fails, status 1, rows NaN; the other three share its wave
  d  9 x 100   the inputs of (a) through tiling 16 (beam_solve_kernel<16, 7>) and 8 | ROWS (beam_rows_kernel<8, 13, 2, false>)
  e  9 x 100   one fused sizing epoch (ops_beam_sizing_epoch_f32 -> beam_rows_sizing_kernel<16, 7, 3>) on the loads of (a)
"""
import ctypes

import numpy as np

SEED = 20261019
ROWS = 0x200                       # OPS_AMD_TILING_ROWS
ROLLERS = (10, 30, 70, 85, 100)    # 1-based nodes, as bench.py's bridge
KERNELS = {"a": "beam_rows_kernel<16, 7, 3, false>", "b": "beam_rows_kernel<16, 7, 3, false>",
           "c": "beam_rows_kernel<16, 7, 3, false>", "d16": "beam_solve_kernel<16, 7, true, true>", "d8r": "beam_rows_kernel<8, 13, 2, false>"}
TILINGS = {"a": 16 | ROWS, "b": 16 | ROWS, "c": 16 | ROWS, "d16": 16, "d8r": 8 | ROWS}
FAILED_BEAM = 2                    # case c


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _loads(rng, B, N, free):
    Fy = np.zeros((B, N))
    for b in range(B):
        nodes = rng.choice(free, size=int(rng.integers(1, 5)), replace=False)
        Fy[b, nodes] = rng.uniform(-355857.0, -35585.7, size=nodes.size)
    return Fy


def bridge(B, seed):
    """B beams of the bench's bridge: 100 elements over 200 m, rollers fixed in u_y, 1-4 point loads, log-uniform inertias."""
    rng = np.random.default_rng([SEED, seed])
    Ne, N = 100, 101
    fix = np.zeros(N, dtype=np.uint8)
    fix[0] = 1
    fix[[r - 1 for r in ROLLERS]] = 1
    Fy = _loads(rng, B, N, np.flatnonzero(fix[1:] == 0) + 1)
    I = np.exp(rng.uniform(np.log(3e-3), np.log(0.75), size=(B, Ne)))
    return dict(x=np.linspace(0.0, 200.0, N), E=np.float64(200e9), I=I, fix=fix, Fy=Fy, wy=np.float64(-1000.0))


def inputs():
    a = bridge(9, 1)
    rng = np.random.default_rng([SEED, 2])
    Ne, N = 37, 38
    fix = np.zeros(N, dtype=np.uint8)
    fix[[0, 12, 25, 37]] = 1
    fix[20] = 2                    # a free node whose rotation is fixed
    b = dict(x=np.concatenate([[0.0], np.cumsum(rng.uniform(1.5, 2.5, size=Ne))]), E=np.float64(200e9),
             I=np.exp(rng.uniform(np.log(3e-3), np.log(0.75), size=(5, Ne))), fix=fix,
             Fy=_loads(rng, 5, N, np.flatnonzero(fix[1:] == 0) + 1), wy=np.float64(-1000.0))
    c = bridge(4, 3)
    c["I"][FAILED_BEAM, 43:45] = 0.0   # node 44 (interior of lane 6's segment) keeps no stiffness at all: a zero pivot
    # (ONE zero element only cuts the beam into two well-supported halves, which solve)
    return {"a": a, "b": b, "c": c, "d16": a, "d8r": a}


def _solve(oa, torch, case, tiling):
    dev = torch.device("cuda")
    t = lambda z, dt=torch.float64: torch.as_tensor(z, dtype=dt, device=dev)   # noqa: E731
    B, Ne = case["I"].shape
    out = oa.BeamSolution(*(torch.full((B, n), float("nan"), dtype=torch.float64, device=dev) for n in (Ne + 1, Ne + 1, Ne, Ne)),
                          torch.full((B,), -77, dtype=torch.int32, device=dev))
    oa.beam_solve(t(case["x"]), t(case["E"]), t(case["I"]), t(case["fix"], torch.uint8), t(case["Fy"]), t(case["wy"]),
                  tiling=tiling, out=out)
    torch.cuda.synchronize()
    return {k: bits(getattr(out, k).cpu().numpy()) for k in ("v", "theta", "V", "M", "status")}


EPOCH_STATE = ("I", "I_last", "exp_avg", "exp_avg_sq", "best_loss", "patience_cnt", "epochs_run", "active", "last_loss", "status")


def epoch_state(a):
    """Optimiser state of case (e) before the epoch: float32 inertias of (a), seeded Adam moments, every third case on another
    epoch, case 5 finished (inactive; it shares its wave with three live ones)."""
    rng = np.random.default_rng([SEED, 5])
    B, Ne = a["I"].shape
    m = rng.standard_normal((B, Ne)).astype(np.float32)
    st = dict(I=a["I"].astype(np.float32), I_last=np.full((B, Ne), -12345.678, dtype=np.float32), exp_avg=m,
              exp_avg_sq=(rng.uniform(0.5, 2.0, size=(B, Ne)) * m.astype(np.float64) ** 2).astype(np.float32),
              best_loss=np.full(B, np.inf, dtype=np.float32), patience_cnt=np.zeros(B, dtype=np.int32),
              epochs_run=np.array([(0, 1, 17)[b % 3] for b in range(B)], dtype=np.int32), active=np.ones(B, dtype=np.uint8),
              last_loss=np.full(B, -12345.678, dtype=np.float32), status=np.full(B, -77, dtype=np.int32))
    st["active"][5] = 0
    return st


def _epoch(lib, torch, a):
    from openpystruct_amd import sizing
    dev = torch.device("cuda")
    hp = sizing.SizingConfig().c_params()
    tab = np.zeros((hp.max_epochs, 2), dtype=np.float32)
    lib.ops_sizing_schedule_f32(ctypes.byref(hp), tab.ctypes.data)
    t = lambda z, dt=None: torch.as_tensor(np.ascontiguousarray(z), dtype=dt).to(dev)   # noqa: E731
    pre = epoch_state(a)
    s = {k: t(z) for k, z in pre.items()}
    B, Ne = a["I"].shape
    dx, dE, dfix, dFy, dwy, sched = t(a["x"]), t(a["E"]), t(a["fix"], torch.uint8), t(a["Fy"]), t(a["wy"]), t(tab)
    rc = lib.ops_beam_sizing_epoch_f32(
        B, Ne, dx.data_ptr(), 0, dE.data_ptr(), 0, dfix.data_ptr(), 0, dFy.data_ptr(), Ne + 1, dwy.data_ptr(), 0,
        *(s[k].data_ptr() for k in EPOCH_STATE[:-1]), ctypes.byref(hp), sched.data_ptr(), s["status"].data_ptr(), 0,
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {"pre_" + k: bits(z) for k, z in pre.items()}
    out.update({"post_" + k: bits(s[k].cpu().numpy()) for k in EPOCH_STATE})
    return out


def run_all():
    """Every case on the GPU: {case: {array: raw bits}}."""
    import torch

    import openpystruct_amd as oa
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    cases = inputs()
    got = {}
    for name, case in cases.items():
        B, Ne = case["I"].shape
        assert oa.kernel_name(B, Ne, TILINGS[name]) == KERNELS[name], (name, oa.kernel_name(B, Ne, TILINGS[name]))
        got[name] = _solve(oa, torch, case, TILINGS[name])
    got["e"] = _epoch(lib, torch, cases["a"])
    return got
