"""The frame solve's VJP on the host (no GPU): (a) the dense torch model (tests/frame_dense.py) against the 3-DOF oracle;
(b) the per-node / per-element arithmetic of csrc/frame_adjoint.hpp -- the text the HIP kernels of csrc/frame_vjp.hip compile --
built with g++ and the address + undefined-behaviour sanitizers into a stand-alone program, with the adjoint solve in between
done by the oracle, against autograd of the dense model."""
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import beam_oracle as bo  # noqa: E402
from tests import frame_dense as fd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "openpystruct_amd", "csrc", "frame_adjoint.hpp")


def _topologies():
    from openpystruct_amd import frames
    return {"1x1": lambda: frames.grid_frame(1, 1, device="cpu"), "2x3": lambda: frames.grid_frame(2, 3, device="cpu"),
            "4x2": lambda: frames.grid_frame(4, 2, device="cpu"), "general": lambda: fd.custom_frame(2, 2, True, True, "cpu"),
            "hub": lambda: fd.hub_frame("cpu")}


CASES = ["1x1", "2x3", "4x2", "general", "hub"]


def _nrel(a, b, scale=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), scale, 1e-300))


def _cotangents(rng, B, Nn, Ne):
    """Sizes that let every cotangent matter: displacements are ~1e-3, forces ~1e4."""
    return [rng.standard_normal((B, Nn, 3)) * 1e6, rng.standard_normal((B, Ne, 6)), rng.standard_normal((B, Ne)),
            rng.standard_normal((B, Ne))]


@pytest.mark.parametrize("name", CASES)
def test_dense_model_reproduces_the_oracle(name):
    topo = _topologies()[name]()
    case = fd.case_of(topo)
    rng = np.random.default_rng(len(name) + topo.Ne)
    B = 2
    I = fd.random_inertias(rng, B, topo.Ne)
    loads = np.broadcast_to(topo.nodal_loads, (B, topo.Nn, 3)) * rng.uniform(0.5, 2.0, size=(B, 1, 1))
    disp, forces, V, M = (t.numpy() for t in fd.dense_frame_solve(case, torch.tensor(I), torch.tensor(loads)))
    for b in range(B):
        d, f, st, _, _ = bo.solve_model_3dof(topo.coords, topo.conn, topo.A, topo.E, I[b], topo.fix3, loads[b], wy=topo.wy, wx=topo.wx)
        tol = max(1e-10, 4e-16 * fd.cond_free(case, I[b]))
        assert st == 0
        assert _nrel(disp[b], d) < tol and _nrel(forces[b], f) < tol
        np.testing.assert_array_equal(V[b], forces[b, :, 1])
        np.testing.assert_array_equal(M[b], forces[b, :, 2])


_PROGRAM = r"""
#include "frame_adjoint.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace opsamd;
template <class T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short file\n"); std::exit(2); }
  return v;
}
// <in> <out>.  in: int32 B, Nn, Ne, mask (bit k: cotangent k present), mode (0: rhs, 1: contraction); geo, EA, E; conn, ptr, idx; I;
// the cotangents present; mode 1: disp, lambda.  out: rhs [B,Nn,3] or gI [B,Ne].
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = rd<int32_t>(f, 5);
  const int B = h[0], Nn = h[1], Ne = h[2], mask = h[3], mode = h[4];
  const auto geo = rd<double>(f, 3 * (size_t)Ne), EA = rd<double>(f, Ne), E = rd<double>(f, Ne);
  const auto conn = rd<int32_t>(f, 2 * (size_t)Ne), ptr = rd<int32_t>(f, Nn + 1), idx = rd<int32_t>(f, 2 * (size_t)Ne);
  const auto I = rd<double>(f, (size_t)B * Ne);
  const auto g_disp = rd<double>(f, mask & 1 ? (size_t)B * Nn * 3 : 0), g_forces = rd<double>(f, mask & 2 ? (size_t)B * Ne * 6 : 0);
  const auto gV = rd<double>(f, mask & 4 ? (size_t)B * Ne : 0), gM = rd<double>(f, mask & 8 ? (size_t)B * Ne : 0);
  const auto disp = rd<double>(f, mode ? (size_t)B * Nn * 3 : 0), lam = rd<double>(f, mode ? (size_t)B * Nn * 3 : 0);
  std::fclose(f);
  auto opt = [](const std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };
  std::vector<double> out;
  for (long b = 0; b < B; ++b) {
    if (mode == 0) {
      for (int n = 0; n < Nn; ++n) {
        double r[3];
        fa_node_rhs(Nn, Ne, geo.data(), EA.data(), E.data(), ptr.data(), idx.data(), I.data(), opt(g_disp), opt(g_forces), opt(gV),
                    opt(gM), b, n, r);
        out.insert(out.end(), r, r + 3);
      }
    } else {
      for (int e = 0; e < Ne; ++e)
        out.push_back(fa_elem_gI(Nn, Ne, geo.data(), E.data(), conn.data(), disp.data(), lam.data(), opt(g_forces), opt(gV), opt(gM), b, e));
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
    assert os.path.exists(HEADER), "csrc/frame_adjoint.hpp is missing"
    d = tmp_path_factory.mktemp("frame_adjoint")
    src, exe = d / "frame_adjoint_host.cpp", d / "frame_adjoint_host"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-ffp-contract=off",
                           "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    return str(exe)


def _run(program, tmp_path, topo, I, cot, mode, disp=None, lam=None):
    from openpystruct_amd import frames
    adj = frames._adjoint_tables(topo)
    B = I.shape[0]
    mask = sum(1 << k for k, c in enumerate(cot) if c is not None)
    fin, fout = tmp_path / f"in{mode}.bin", tmp_path / f"out{mode}.bin"
    with open(fin, "wb") as f:
        np.array([B, topo.Nn, topo.Ne, mask, mode], dtype=np.int32).tofile(f)
        for t in (topo.d_geo, topo.d_EA, topo.d_E):
            t.numpy().astype(np.float64).tofile(f)
        for t in (adj.conn, adj.ptr, adj.idx):
            t.numpy().astype(np.int32).tofile(f)
        for a in [I] + [c for c in cot if c is not None] + ([disp, lam] if mode else []):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    subprocess.check_call([program, str(fin), str(fout)])
    return np.fromfile(fout, dtype=np.float64).reshape((B, topo.Nn, 3) if mode == 0 else (B, topo.Ne))


@pytest.mark.parametrize("mask", [15, 1, 6, 8])
@pytest.mark.parametrize("name", CASES)
def test_host_arithmetic_with_the_oracle_solve_matches_dense_autograd(program, tmp_path, name, mask):
    topo = _topologies()[name]()
    case = fd.case_of(topo)
    rng = np.random.default_rng(7 * len(name) + topo.Ne + mask)
    B = 2
    I = fd.random_inertias(rng, B, topo.Ne)
    loads = np.broadcast_to(topo.nodal_loads, (B, topo.Nn, 3)) * rng.uniform(0.5, 2.0, size=(B, 1, 1))
    cot = [c if (mask >> k) & 1 else None for k, c in enumerate(_cotangents(rng, B, topo.Nn, topo.Ne))]

    It, Lt = torch.tensor(I, requires_grad=True), torch.tensor(loads, requires_grad=True)
    outs = fd.dense_frame_solve(case, It, Lt)
    loss = sum((o * torch.tensor(c)).sum() for o, c in zip(outs, cot) if c is not None)
    gI_ref, gL_ref = (g.numpy() for g in torch.autograd.grad(loss, [It, Lt]))
    disp = outs[0].detach().numpy()

    rhs = _run(program, tmp_path, topo, I, cot, 0)
    lam = np.stack([bo.solve_model_3dof(topo.coords, topo.conn, topo.A, topo.E, I[b], topo.fix3, rhs[b])[0] for b in range(B)])
    gI = _run(program, tmp_path, topo, I, cot, 1, disp, lam)

    tol = max(1e-8, 4e-16 * max(fd.cond_free(case, I[b]) for b in range(B)))
    assert _nrel(lam, gL_ref) < tol
    assert _nrel(gI, gI_ref, fd.gI_term_scale(case, disp, gL_ref, fd.fold(B, topo.Ne, *cot[1:]))) < tol


def test_node_element_list_covers_every_end_once_with_any_degree():
    from openpystruct_amd import frames
    topo = fd.hub_frame("cpu")
    adj = frames._adjoint_tables(topo)
    ptr, idx = adj.ptr.numpy(), adj.idx.numpy()
    assert frames._adjoint_tables(topo) is adj                      # built once, kept on the topology
    assert ptr[0] == 0 and ptr[-1] == 2 * topo.Ne and (np.diff(ptr) >= 1).all() and np.diff(ptr).max() == 18
    assert sorted(idx.tolist()) == list(range(2 * topo.Ne))
    for n in range(topo.Nn):
        ends = idx[ptr[n]:ptr[n + 1]]
        assert (topo.conn.reshape(-1)[ends] == n).all() and (np.diff(ends) > 0).all()
