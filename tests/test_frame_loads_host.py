"""Per-frame element loads on the host (no GPU): (a) the dense torch model with the element loads as a tensor
(tests/frame_dense_w.py) against the 3-DOF oracle; (b) the per-node / per-element arithmetic of csrc/frame_loads.hpp -- the text the
HIP kernels of csrc/frame_loads.hip compile -- built with g++ and the address + undefined-behaviour sanitizers into a stand-alone
program: right-hand side, the oracle's solve WITHOUT element loads, force correction against the oracle's solve WITH them, and g_w
against autograd of the dense model; (c) `grid_load_cases`, the dataset's draws and the argument checks of the Python entries."""
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import beam_oracle as bo  # noqa: E402
from tests import frame_dense as fd  # noqa: E402
from tests import frame_dense_w as fw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpystruct_amd", "csrc")
HEADER = os.path.join(CSRC, "frame_loads.hpp")


def _topologies():
    from openpystruct_amd import frames
    return {"1x1": lambda: frames.grid_frame(1, 1, device="cpu"), "2x3": lambda: frames.grid_frame(2, 3, device="cpu"),
            "general": lambda: fd.custom_frame(2, 2, True, True, "cpu"), "hub": lambda: fd.hub_frame("cpu")}


CASES = ["1x1", "2x3", "general", "hub"]


def _nrel(a, b, scale=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), scale, 1e-300))


def _batch(name, B=3, seed=0):
    topo = _topologies()[name]()
    rng = np.random.default_rng(11 * len(name) + topo.Ne + seed)
    I = fd.random_inertias(rng, B, topo.Ne)
    loads = np.broadcast_to(topo.nodal_loads, (B, topo.Nn, 3)) * rng.uniform(0.5, 2.0, size=(B, 1, 1)) + rng.standard_normal((B, topo.Nn, 3)) * 1e3
    w = fw.random_element_loads(rng, B, topo.Ne, zero_frame=1)
    return topo, fd.case_of(topo), rng, I, loads, w


def _oracle(topo, I, loads, w):
    out = [bo.solve_model_3dof(topo.coords, topo.conn, topo.A, topo.E, I[b], topo.fix3, loads[b], wy=w[b, :, 0], wx=w[b, :, 1])
           for b in range(I.shape[0])]
    assert all(o[2] == 0 for o in out)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("name", CASES)
def test_dense_w_model_reproduces_the_oracle(name):
    topo, case, _, I, loads, w = _batch(name)
    disp, forces, V, M = (t.numpy() for t in fw.dense_frame_solve_w(case, torch.tensor(I), torch.tensor(loads), torch.tensor(w)))
    d_ref, f_ref = _oracle(topo, I, loads, w)
    for b in range(I.shape[0]):
        tol = max(1e-10, 4e-16 * fd.cond_free(case, I[b]))
        assert _nrel(disp[b], d_ref[b]) < tol and _nrel(forces[b], f_ref[b]) < tol
    np.testing.assert_array_equal(V, forces[..., 1])
    np.testing.assert_array_equal(M, forces[..., 2])


def test_dense_w_model_with_the_case_loads_is_the_dense_model():
    topo, case, _, I, loads, _ = _batch("general")
    w = np.stack([topo.wy, topo.wx], axis=1)
    a = fw.dense_frame_solve_w(case, torch.tensor(I), torch.tensor(loads), torch.tensor(w))
    b = fd.dense_frame_solve(case, torch.tensor(I), torch.tensor(loads))
    for p, q in zip(a, b):
        assert _nrel(p.numpy(), q.numpy()) < 1e-13


_PROGRAM = r"""
#include "frame_loads.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace opsamd;
template <class T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short file\n"); std::exit(2); }
  return v;
}
// <in> <out>.  in: int32 B, Nn, Ne, mode (0: rhs, 1: forces, 2: vjp), loads shared, w shared, mask (bit k: cotangent k of g_forces,
// gV, gM present); geo; conn, ptr, idx; loads; w; mode 1: forces, status (int32); mode 2: the cotangents present, lambda.
// out: rhs [B,Nn,3] | forces [B,Ne,6] | g_w [B,Ne,2].
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = rd<int32_t>(f, 7);
  const int B = h[0], Nn = h[1], Ne = h[2], mode = h[3], lshared = h[4], wshared = h[5], mask = h[6];
  const auto geo = rd<double>(f, 3 * (size_t)Ne);
  const auto conn = rd<int32_t>(f, 2 * (size_t)Ne), ptr = rd<int32_t>(f, Nn + 1), idx = rd<int32_t>(f, 2 * (size_t)Ne);
  const auto loads = rd<double>(f, (size_t)(lshared ? 1 : B) * Nn * 3), w = rd<double>(f, (size_t)(wshared ? 1 : B) * Ne * 2);
  const long lbs = lshared ? 0 : 3L * Nn, wbs = wshared ? 0 : 2L * Ne;
  auto forces = rd<double>(f, mode == 1 ? (size_t)B * Ne * 6 : 0);
  const auto status = rd<int32_t>(f, mode == 1 ? B : 0);
  const auto g_forces = rd<double>(f, mode == 2 && (mask & 1) ? (size_t)B * Ne * 6 : 0);
  const auto gV = rd<double>(f, mode == 2 && (mask & 2) ? (size_t)B * Ne : 0), gM = rd<double>(f, mode == 2 && (mask & 4) ? (size_t)B * Ne : 0);
  const auto lam = rd<double>(f, mode == 2 ? (size_t)B * Nn * 3 : 0);
  std::fclose(f);
  auto opt = [](const std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };
  std::vector<double> out;
  for (long b = 0; b < B; ++b) {
    if (mode == 0) {
      for (int n = 0; n < Nn; ++n) {
        double r[3];
        fl_node_rhs(Nn, geo.data(), ptr.data(), idx.data(), loads.data(), lbs, w.data(), wbs, b, n, r);
        out.insert(out.end(), r, r + 3);
      }
    } else if (mode == 1) {
      for (int e = 0; e < Ne; ++e) {
        double* fe = forces.data() + (b * Ne + e) * 6;
        if (status[b] == 0) fl_elem_forces(geo.data(), w.data(), wbs, b, e, fe);
        out.insert(out.end(), fe, fe + 6);
      }
    } else {
      for (int e = 0; e < Ne; ++e) {
        double gw[2];
        fl_elem_gw(Nn, Ne, geo.data(), conn.data(), lam.data(), opt(g_forces), opt(gV), opt(gM), b, e, gw);
        out.insert(out.end(), gw, gw + 2);
      }
    }
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) return 2;
  std::fclose(o);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found: the host program cannot be built")
    assert os.path.exists(HEADER), "csrc/frame_loads.hpp is missing"
    d = tmp_path_factory.mktemp("frame_loads")
    src, exe = d / "frame_loads_host.cpp", d / "frame_loads_host"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _run(program, tmp_path, topo, mode, loads, w, forces=None, status=None, cot=(None, None, None), lam=None, B=None):
    from openpystruct_amd import frames
    adj = frames._adjoint_tables(topo)
    B = B if B is not None else max(a.shape[0] for a in (loads, w) if a.ndim == 3)
    mask = sum(1 << k for k, c in enumerate(cot) if c is not None)
    fin, fout = tmp_path / f"in{mode}.bin", tmp_path / f"out{mode}.bin"
    with open(fin, "wb") as f:
        np.array([B, topo.Nn, topo.Ne, mode, loads.ndim == 2, w.ndim == 2, mask], dtype=np.int32).tofile(f)
        topo.d_geo.numpy().astype(np.float64).tofile(f)
        for t in (adj.conn, adj.ptr, adj.idx):
            t.numpy().astype(np.int32).tofile(f)
        for a in (loads, w) + ((forces,) if mode == 1 else ()):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        if mode == 1:
            np.ascontiguousarray(status, dtype=np.int32).tofile(f)
        if mode == 2:
            for a in [c for c in cot if c is not None] + [lam]:
                np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    subprocess.check_call([program, str(fin), str(fout)])
    return np.fromfile(fout, dtype=np.float64).reshape({0: (B, topo.Nn, 3), 1: (B, topo.Ne, 6), 2: (B, topo.Ne, 2)}[mode])


def _solve_without_element_loads(topo, I, rhs):
    out = [bo.solve_model_3dof(topo.coords, topo.conn, topo.A, topo.E, I[b], topo.fix3, rhs[b]) for b in range(I.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("shared", ["none", "loads", "w"])
@pytest.mark.parametrize("name", CASES)
def test_host_forward_around_the_oracle_solve_matches_the_oracle_under_element_loads(program, tmp_path, name, shared):
    topo, case, _, I, loads, w = _batch(name)
    B = I.shape[0]
    loads_in, w_in = (loads[0] if shared == "loads" else loads), (w[0] if shared == "w" else w)
    loads_full, w_full = np.broadcast_to(loads_in, loads.shape), np.broadcast_to(w_in, w.shape)
    d_ref, f_ref = _oracle(topo, I, loads_full, w_full)
    rhs = _run(program, tmp_path, topo, 0, loads_in, w_in, B=B)
    disp, f0 = _solve_without_element_loads(topo, I, rhs)
    forces = _run(program, tmp_path, topo, 1, loads_in, w_in, forces=f0, status=np.zeros(B, dtype=np.int32), B=B)
    for b in range(B):
        tol = max(1e-10, 4e-16 * fd.cond_free(case, I[b]))
        assert _nrel(disp[b], d_ref[b]) < tol and _nrel(forces[b], f_ref[b]) < tol
    if shared != "w":
        np.testing.assert_array_equal(rhs[1], loads_full[1])          # the frame without element loads: its nodal loads, bit for bit
        np.testing.assert_array_equal(forces[1], f0[1])
    # a frame whose status is set keeps its rows, whatever they hold
    marked = np.array([0, 5, 0], dtype=np.int32)
    kept = _run(program, tmp_path, topo, 1, loads_in, w_in, forces=np.where(marked[:, None, None] != 0, np.nan, f0), status=marked, B=B)
    assert np.isnan(kept[1]).all()
    np.testing.assert_array_equal(kept[[0, 2]], forces[[0, 2]])


@pytest.mark.parametrize("mask", [7, 1, 6, 0])
@pytest.mark.parametrize("name", CASES)
def test_host_g_w_matches_dense_autograd(program, tmp_path, name, mask):
    """mask: which of (g_forces, gV, gM) are present; the cotangent of disp is always there (with mask 0: g_w = lambda . dpg/dw)."""
    topo, case, rng, I, loads, w = _batch(name, seed=mask)
    B = I.shape[0]
    g_disp = rng.standard_normal((B, topo.Nn, 3)) * 1e6
    cot = [c if (mask >> k) & 1 else None for k, c in
           enumerate([rng.standard_normal((B, topo.Ne, 6)), rng.standard_normal((B, topo.Ne)), rng.standard_normal((B, topo.Ne))])]
    It, Lt, Wt = (torch.tensor(a, requires_grad=True) for a in (I, loads, w))
    outs = fw.dense_frame_solve_w(case, It, Lt, Wt)
    loss = sum((o * torch.tensor(c)).sum() for o, c in zip(outs, [g_disp] + cot) if c is not None)
    lam, gw_ref = (g.numpy() for g in torch.autograd.grad(loss, [Lt, Wt]))
    gw = _run(program, tmp_path, topo, 2, loads, w, cot=cot, lam=lam)
    tol = max(1e-8, 4e-16 * max(fd.cond_free(case, I[b]) for b in range(B)))
    assert _nrel(gw, gw_ref) < tol


def test_grid_load_cases_reproduces_grid_frame():
    from openpystruct_amd import frames
    for bays, stories in ((1, 1), (2, 2), (4, 3)):
        cfg = frames.FrameConfig(lateral_load=1.3e4, vertical_load=-0.7e4)
        topo = frames.grid_frame(bays, stories, cfg, device="cpu")
        loads, w = frames.grid_load_cases(topo, [cfg.lateral_load, 2.0, 0.0], torch.tensor([cfg.vertical_load, -3.0, 0.0]))
        assert loads.shape == (3, topo.Nn, 3) and w.shape == (3, topo.Ne, 2) and loads.dtype == w.dtype == torch.float64
        np.testing.assert_array_equal(loads[0].numpy(), topo.nodal_loads)
        np.testing.assert_array_equal(w[0, :, 0].numpy(), topo.wy)
        np.testing.assert_array_equal(w[0, :, 1].numpy(), topo.wx)
        np.testing.assert_array_equal(loads[1].numpy(), topo.nodal_loads / cfg.lateral_load * 2.0)
        np.testing.assert_array_equal(w[1].numpy(), np.stack([topo.wy, topo.wx], 1) / cfg.vertical_load * -3.0)
        assert not loads[2].any() and not w[2].any()
    with pytest.raises(ValueError):
        frames.grid_load_cases(topo, [1.0, 2.0], [1.0])


def test_dataset_draws_are_reproducible_and_in_range():
    from openpystruct_amd import frames
    a, b = frames.frame_dataset_draws(64, seed=5), frames.frame_dataset_draws(64, seed=5)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    c = frames.frame_dataset_draws(64, seed=6)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    assert a[0].shape == a[1].shape == (64,) and a[0].dtype == a[1].dtype == np.float64
    assert (a[0] >= 0.5e4).all() and (a[0] < 2e4).all() and (a[1] >= -2e4).all() and (a[1] < -0.5e4).all()
    rng = np.random.default_rng(5)                                # the documented draw: np.random.default_rng(seed), uniform
    np.testing.assert_array_equal(a[0], rng.uniform(0.5e4, 2e4, size=64))
    np.testing.assert_array_equal(a[1], rng.uniform(-2e4, -0.5e4, size=64))
    lo = frames.frame_dataset_draws(8, (1.0, 2.0), (-4.0, -3.0), seed=1)
    assert (lo[0] >= 1.0).all() and (lo[0] < 2.0).all() and (lo[1] >= -4.0).all() and (lo[1] < -3.0).all()
    assert frames.frame_dataset_draws(0)[0].shape == (0,)
    with pytest.raises(ValueError):
        frames.frame_dataset_draws(-1)


def test_python_entries_need_gpu_tensors():
    """Without a GPU the entries refuse CPU tensors before they touch the library: there is no CPU path."""
    from openpystruct_amd import frames
    topo = frames.grid_frame(1, 1, device="cpu")
    I = torch.full((2, topo.Ne), 5e-4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.frame_solve(topo, I, element_loads=torch.zeros((topo.Ne, 2), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.frame_element_load_vjp(topo, torch.zeros((2, topo.Nn, 3), dtype=torch.float64))


def test_new_header_is_an_extension_and_not_the_last():
    from openpystruct_amd import _cabi
    names = [os.path.basename(p) for p in _cabi.EXTENSION_HEADER_PATHS]
    assert "openpystruct_amd_frame_loads.h" in names[:-1] and names[-1] == "openpystruct_amd_sizing_grad.h"
    assert {"ops_frame_load_rhs_f64", "ops_frame_load_forces_f64", "ops_frame_load_vjp_f64"} <= set(_cabi.EXTENSION_EXPORTS)
    assert _cabi.SizingObjective.__name__ == "SizingObjective" and _cabi.FrameSizingObjective.__name__ == "FrameSizingObjective"
