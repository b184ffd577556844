"""The design-objective kernels' arithmetic without a GPU: openpystruct_amd/csrc/design_loss_math.hpp run lane by
lane on the CPU (tests/csrc/emul_design_loss.cpp) against the numpy float64 reference (tests/design_loss_ref.py), and the
predictions' side bit for bit against the framework's expression.  tests/test_gpu_design_loss.py runs the kernels themselves."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import design_loss_ref as dr  # noqa: E402
from tests import sizing_multicase_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_emul = None
SHAPES = [(1, 1, 1), (1, 2, 2), (3, 3, 13), (5, 6, 100), (2, 64, 65), (2, 2, 512), (9, 1, 64), (9, 1, 65)]


def emul_lib():
    """g++ build of tests/csrc/emul_design_loss.cpp (the recipe of tests/test_sizing_grad_emulation.py::emul_lib)."""
    global _emul
    if _emul is None:
        src = os.path.join(ROOT, "tests", "csrc", "emul_design_loss.cpp")
        hdrs = [os.path.join(ROOT, "openpystruct_amd", "csrc", "design_loss_math.hpp")]
        so_path = os.path.join(ROOT, "tests", "csrc", "libemul_design_loss.so")
        if not os.path.exists(so_path) or os.path.getmtime(so_path) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so_path, src])
        _emul = ctypes.CDLL(so_path)
        vp, i, lg, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
        _emul.emul_design_prep.restype = ctypes.c_int
        _emul.emul_design_prep.argtypes = [i, i, vp, i, lg, vp, vp, fl, vp]
        _emul.emul_design_finish.restype = ctypes.c_int
        _emul.emul_design_finish.argtypes = [i] * 4 + [vp] * 9 + [i, lg, vp, vp, fl, fl] + [vp] * 7
    return _emul


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def consts(hp):
    return np.array([hp.alpha_moment, hp.alpha_shear, 2.0 * hp.E, hp.bend_eps, hp.G * hp.area_coef])


class Scaler:       # StandardScalerT's two fields and its inverse transform
    def __init__(self, scale, mean):
        self.scale_, self.mean_ = torch.as_tensor(scale), torch.as_tensor(mean)

    def inverse_transform(self, x):
        return x * self.scale_.to(x.device) + self.mean_.to(x.device)


def predictions(rng, B, Ne, ld, bf16):
    """Standardised predictions in a [B, ld] matrix, a scaler, and a few that land below the floor or exactly on it."""
    scale = rng.uniform(0.05, 0.3, size=Ne).astype(np.float32)
    mean = rng.uniform(0.2, 0.6, size=Ne).astype(np.float32)
    p = rng.standard_normal((B, ld)).astype(np.float32)
    p[:, ::3] -= 40.0                                 # far below the floor
    if Ne > 1:
        mean[1], p[0, 1] = np.float32(1e-8), 0.0      # exactly on it
    t = torch.as_tensor(p)
    if bf16:
        t = t.to(torch.bfloat16)
    return t, Scaler(scale, mean)


def as_host(t):
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("Ne", [1, 13, 100])
def test_prep_arithmetic_is_the_frameworks_bit_for_bit(Ne, bf16):
    rng = np.random.default_rng(100 + Ne + bf16)
    B, ld = 7, Ne + 3
    t, sI = predictions(rng, B, Ne, ld, bf16)
    want = dr.prep_reference(t[:, :Ne], sI).numpy()
    got = np.empty((B, Ne))
    host = as_host(t)
    assert emul_lib().emul_design_prep(B, Ne, _p(host), int(bf16), ld, _p(sI.scale_.numpy()), _p(sI.mean_.numpy()), 1e-8, _p(got)) == 0
    assert np.array_equal(got, want)
    assert (got == np.float64(np.float32(1e-8))).any()
    nan = torch.full((1, Ne), float("nan"))
    out = np.empty((1, Ne))
    emul_lib().emul_design_prep(1, Ne, _p(nan.numpy()), 0, Ne, _p(sI.scale_.numpy()), _p(sI.mean_.numpy()), 1e-8, _p(out))
    assert np.isnan(out).all()                       # clamp_min's semantics: a NaN stays NaN


def emul_finish(s, C, aggregate, weights, extra, t, sI, bf16, weight, ref, status=None):
    B, Ne = s.I.shape
    ld = t.shape[1]
    out = dict(sample_loss=np.empty(B), gI=np.empty((B, Ne)), case_penalty=np.empty((B, C)), governing=np.empty(B, dtype=np.int32),
               share=np.empty(B))
    dp = np.zeros((B, ld), dtype=np.int16 if bf16 else np.float32)
    host = as_host(t)
    V, M, g = (np.ascontiguousarray(a.reshape(B * C, Ne)) for a in (s.V, s.M, s.grad))
    ex = None if extra is None else np.ascontiguousarray(extra.reshape(-1))
    rc = emul_lib().emul_design_finish(B, C, Ne, aggregate, _p(consts(s.hp)), _p(s.I), _p(V), _p(M), _p(g), _p(ex), _p(weights), _p(status),
                                       _p(host), int(bf16), ld, _p(sI.scale_.numpy()), _p(sI.mean_.numpy()), 1e-8, weight, _p(ref),
                                       _p(out["sample_loss"]), _p(out["gI"]), _p(out["case_penalty"]), _p(out["governing"]), _p(dp),
                                       _p(out["share"]))
    assert rc == 0
    d = torch.as_tensor(dp)
    out["dpreds"] = (d.view(torch.bfloat16).float() if bf16 else d).numpy().astype(np.float64)
    return out


def check_against_reference(got, r, Ne, bf16, weight, B):
    """The bounds of tests/design_loss_ref.py on every output of one finish (emulated or on the GPU)."""
    assert np.array_equal(got["governing"], r.governing)
    assert (np.abs(got["case_penalty"] - r.case_penalty) <= r.tol_P).all()
    assert (np.abs(got["sample_loss"] - r.sample_loss) <= r.tol_L).all()
    assert (np.abs(got["gI"] - r.gI) <= r.tol_g).all()
    d = got["dpreds"][:, :Ne]
    if bf16:        # one bf16 ulp (8 significant bits: at most 2^-7 of the value)
        assert (np.abs(d - r.dpreds) <= 2.0 ** -7 * np.abs(r.dpreds) + r.tol_d).all()
    else:
        assert (np.abs(d - r.dpreds) <= 2.0 ** -24 * np.abs(r.dpreds) + r.tol_d).all()
    assert (got["dpreds"][:, Ne:] == 0).all()
    if "value" in got:
        assert abs(got["value"] - r.value) <= 2.0 ** -24 * abs(r.value) + r.tol_value
    else:
        value = weight * got["share"].sum() / B
        assert abs(value - r.value) <= r.tol_value + 8 * dr.U * abs(r.value)


def variants(C):
    w = np.linspace(0.5, 2.0, C)
    return [("sum", mr.SUM, None), ("sum+w", mr.SUM, w), ("max", mr.MAX, None)]


@pytest.mark.parametrize("B,C,Ne", SHAPES)
@pytest.mark.parametrize("with_extra", [False, True])
def test_emulated_finish_vs_the_float64_reference(B, C, Ne, with_extra):
    rng = np.random.default_rng([B, C, Ne, with_extra])
    s = dr.synthetic_rows(B, C, Ne, seed=1)
    extra = s.extra if with_extra else None
    for bf16, ref in ((False, None), (True, rng.uniform(0.5, 50.0, size=B))):
        t, sI = predictions(rng, B, Ne, Ne + 2, bf16)
        live = (dr.raw_reference(t[:, :Ne], sI) > 1e-8).numpy()
        for name, agg, w in variants(C):
            r = dr.finish_reference(s.I, s.V, s.M, s.grad, extra, w, agg, s.hp, live=live, scale=sI.scale_.numpy(), weight=float(np.float32(0.7)), ref=ref)
            assert dr.well_separated(r.case_penalty if agg == mr.MAX else (np.ones(C) if w is None else w) * r.case_penalty), name
            got = emul_finish(s, C, agg, w, extra, t, sI, bf16, np.float32(0.7), ref)
            check_against_reference(got, r, Ne, bf16, float(np.float32(0.7)), B)
            if agg == mr.MAX:
                assert np.array_equal(got["governing"], s.big)
                assert np.array_equal(got["gI"], s.grad[np.arange(B), s.big])


def test_emulated_ties_failures_and_the_single_case_collapse():
    rng = np.random.default_rng(5)
    B, C, Ne = 3, 4, 13
    s = dr.synthetic_rows(B, C, Ne, seed=2)
    t, sI = predictions(rng, B, Ne, Ne, False)
    # two bit-identical case rows that govern: the lower index
    for a in (s.V, s.M, s.grad):
        a[:, 1] = a[np.arange(B), s.big]
        a[:, 3] = a[:, 1]
    got = emul_finish(s, C, mr.MAX, None, None, t, sI, False, np.float32(1.0), None)
    assert (got["governing"] == np.where(s.big == 0, 0, 1)).all()
    # a failed row, a NaN inertia: NaN for that sample, every other sample bit-equal to a call without it
    clean = emul_finish(s, C, mr.SUM, None, None, t, sI, False, np.float32(1.0), None)
    status = np.zeros((B, C), dtype=np.int32)
    status[1, 2] = 7
    hit = emul_finish(s, C, mr.SUM, None, None, t, sI, False, np.float32(1.0), None, status=status)
    s.I[2, 5] = np.nan
    hit2 = emul_finish(s, C, mr.SUM, None, None, t, sI, False, np.float32(1.0), None, status=status)
    for k in ("sample_loss", "gI", "dpreds"):
        assert np.isnan(hit[k][1]).all() and np.array_equal(hit[k][[0, 2]], clean[k][[0, 2]]), k
        assert np.isnan(hit2[k][1:]).all() and np.array_equal(hit2[k][0], clean[k][0]), k
    assert np.isnan(hit["share"].sum())
    # C == 1, the sum, no weights, unit scaler, weight = B, no ref: gI is the gradient row, dpreds its float32 rounding
    s1 = dr.synthetic_rows(5, 1, 100, seed=3)
    p = torch.as_tensor(rng.uniform(0.1, 1.0, size=(5, 100)).astype(np.float32))
    unit = Scaler(np.ones(100, dtype=np.float32), np.zeros(100, dtype=np.float32))
    got = emul_finish(s1, 1, mr.SUM, None, None, p, unit, False, np.float32(5.0), None)
    assert np.array_equal(got["gI"], s1.grad[:, 0])
    assert np.array_equal(got["dpreds"].astype(np.float32), s1.grad[:, 0].astype(np.float32))
