"""The beam-solve VJP's per-lane arithmetic (openpystruct_amd/csrc/beam_adjoint.hpp over beam_math.hpp) run lane by lane
on the CPU (tests/csrc/emul_beam_vjp.cpp) against autograd of a dense float64 model, for every tiling the VJP kernel is
compiled for.  Covers the adjoint mathematics without a GPU; tests/test_gpu_beam_grad.py runs the kernel itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.beam_dense import cond_free, dense_solve, gI_term_scale, random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VJP_TILINGS = [(16, 7), (32, 4), (64, 4), (64, 8), (64, 16)]   # csrc/beam_vjp.hip kVjpTilings
_emul = None


def emul_lib():
    """g++ build of tests/csrc/emul_beam_vjp.cpp (same recipe as tests/helpers.py::emul_lib)."""
    global _emul
    if _emul is None:
        src = os.path.join(ROOT, "tests", "csrc", "emul_beam_vjp.cpp")
        hdrs = [os.path.join(ROOT, "openpystruct_amd", "csrc", h) for h in ("beam_math.hpp", "beam_adjoint.hpp")]
        so = os.path.join(ROOT, "tests", "csrc", "libemul_beam_vjp.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
        _emul = ctypes.CDLL(so)
        f = _emul.emul_beam_solve_vjp_f64
        f.restype = ctypes.c_int
        vp, lg = ctypes.c_void_p, ctypes.c_long
        f.argtypes = [ctypes.c_int] * 4 + [vp, lg] * 4 + [vp] * 10
    return _emul


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


def emul_vjp(P, M, x, E, I, fix, v, th, gv, gt, gV, gM):
    B, Ne = I.shape
    N = Ne + 1
    keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (x, I, v, th, gv, gt, gV, gM)]
    x, I, v, th, gv, gt, gV, gM = keep
    E = np.ascontiguousarray(np.atleast_1d(np.asarray(E, dtype=np.float64)))
    fix = np.ascontiguousarray(fix, dtype=np.uint8)
    gI = np.empty((B, Ne)); gF = np.empty((B, N)); gw = np.empty((B, Ne)); st = np.empty(B, dtype=np.int32)
    rc = emul_lib().emul_beam_solve_vjp_f64(
        P, M, B, Ne, _p(x), N if x.ndim == 2 else 0, _p(E), Ne if E.ndim == 2 else 0, _p(I), Ne, _p(fix),
        N if fix.ndim == 2 else 0, _p(v), _p(th), _p(gv), _p(gt), _p(gV), _p(gM), _p(gI), _p(gF), _p(gw), _p(st))
    assert rc == 0, rc
    return gI, gF, gw, st


def nrel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def dense_reference(x, E, I, fix, Fy, wy, cot):
    """The dense model's outputs (v, theta, V, M) and autograd of sum(cot . outputs) w.r.t. I, Fy, wy."""
    It = torch.tensor(I, requires_grad=True)
    Ft = torch.tensor(Fy, requires_grad=True)
    wt = torch.tensor(wy, dtype=torch.float64, requires_grad=True)
    outs = dense_solve(torch.as_tensor(x), E, It, fix, Ft, wt)
    loss = sum((o * torch.as_tensor(c)).sum() for o, c in zip(outs, cot) if c is not None)
    gI, gF, gw = torch.autograd.grad(loss, (It, Ft, wt))
    return [o.detach().numpy() for o in outs], gI.numpy(), gF.numpy(), gw.numpy()


@pytest.mark.parametrize("P,M", VJP_TILINGS)
@pytest.mark.parametrize("Ne", [1, 2, 5, 13, 100, 255, 1023])
@pytest.mark.parametrize("per_beam", [False, True])
def test_emulated_vjp_vs_dense_autograd(P, M, Ne, per_beam):
    if P * M < Ne + 1:
        pytest.skip("tiling too small for this Ne")
    if Ne > 100 and P * M > 4 * (Ne + 1):
        pytest.skip("covered by a tighter tiling")
    rng = np.random.default_rng(1000 * Ne + P + M + per_beam)
    B = 1 if Ne > 255 else 3
    x, fix, I, Fy = random_case(rng, B, Ne, per_beam=per_beam)
    N = Ne + 1
    E = 2.0e11
    wy = rng.uniform(-2e3, 0, size=(B, Ne)) if per_beam else np.float64(-750.0)
    cot = (rng.standard_normal((B, N)) * 1e3, rng.standard_normal((B, N)) * 1e3, rng.standard_normal((B, Ne)),
           rng.standard_normal((B, Ne)))
    outs, gI_r, gF_r, gw_r = dense_reference(x, E, I, fix, Fy, wy, cot)
    gI, gF, gw, st = emul_vjp(P, M, x, E, I, fix, outs[0], outs[1], *cot)
    assert (st == 0).all()
    xs = x if x.ndim == 1 else x[0]
    fs = fix if fix.ndim == 1 else fix[0]
    tol = max(1e-10, 4e-16 * cond_free(xs, E, I[0], fs))
    eI = np.linalg.norm(gI - gI_r) / max(np.linalg.norm(gI_r), gI_term_scale(x, I, wy, outs, cot))
    assert eI < tol, (eI, tol)
    assert nrel(gF, gF_r) < tol, (nrel(gF, gF_r), tol)
    if per_beam:
        assert nrel(gw, gw_r) < tol, (nrel(gw, gw_r), tol)
    else:   # a shared wy: the sum over every element of the batch
        assert abs(gw.sum() - gw_r) <= tol * np.abs(gw).sum()
    fixed_v = np.broadcast_to((fix & 1) != 0, (B, N))
    assert (gF[fixed_v] == 0).all()


@pytest.mark.parametrize("P,M", [(16, 7), (64, 4)])
def test_emulated_vjp_null_cotangents(P, M):
    """A NULL cotangent is a zero one."""
    rng = np.random.default_rng(7)
    B, Ne = 2, 20
    x, fix, I, Fy = random_case(rng, B, Ne)
    (v, th, _, _), *_ = dense_reference(x, 2e11, I, fix, Fy, -500.0, (np.ones((B, Ne + 1)), None, None, None))
    cot = [rng.standard_normal((B, Ne + 1)), rng.standard_normal((B, Ne + 1)), rng.standard_normal((B, Ne)),
           rng.standard_normal((B, Ne))]
    for drop in range(4):
        c_null, c_zero = list(cot), list(cot)
        c_null[drop] = None
        c_zero[drop] = np.zeros_like(cot[drop])
        a = emul_vjp(P, M, x, 2e11, I, fix, v, th, *c_null)
        b = emul_vjp(P, M, x, 2e11, I, fix, v, th, *c_zero)
        for p, q in zip(a, b):
            assert np.array_equal(p, q)


def test_emulated_vjp_singular_beam_is_nan():
    x = np.linspace(0, 10, 11)
    fix = np.zeros(11, dtype=np.uint8); fix[0] = fix[-1] = 1
    I = np.full((2, 10), 0.1); I[0, 4] = -0.1
    v = np.ones((2, 11)); th = np.ones((2, 11))
    gI, gF, gw, st = emul_vjp(16, 7, x, 2e11, I, fix, v, th, np.ones((2, 11)), None, None, None)
    assert st[0] != 0 and st[1] == 0
    assert np.isnan(gI[0]).all() and np.isnan(gF[0]).all() and np.isnan(gw[0]).all()
    assert np.isfinite(gI[1]).all() and np.isfinite(gF[1]).all()
