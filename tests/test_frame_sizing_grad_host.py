"""The exact-gradient frame sizing objective on the host (no GPU): (1) the decomposition the kernels compute --
explicit part + the solve's VJP of the objective's cotangents -- against autograd of L through the dense model
(tests/frame_dense.py), and that against central differences of L; (2) the per-node / per-element arithmetic of
csrc/frame_sizing_math.hpp -- the text the HIP kernels of csrc/frame_sizing_grad.hip compile -- built with g++ and the address +
undefined-behaviour sanitizers into a stand-alone program, with the adjoint solve in between done by the oracle, against the
dense reference; (3) the loop oracle against the committed fixture tests/golden/frame_sizing_total_reference.npz."""
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import beam_oracle as bo  # noqa: E402
from tests import frame_dense as fd  # noqa: E402
from tests import frame_sizing_total_ref as ft  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpystruct_amd", "csrc")
HEADER = os.path.join(CSRC, "frame_sizing_math.hpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_sizing_total_reference.npz")
CASES = ["2x3", "4x2", "general", "hub"]


def _topology(name):
    from openpystruct_amd import frames
    if name == "general":
        return fd.custom_frame(2, 2, True, True, "cpu")
    if name == "hub":
        return fd.hub_frame("cpu")
    bays, stories = (int(v) for v in name.split("x"))
    return frames.grid_frame(bays, stories, device="cpu")


def _nrel(a, b, scale=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), scale, 1e-300))


def _setup(name, B=2):
    """A topology, inertias and the objective whose limits are half the forward's own largest |ux| and |uy|: both hinges are
    active on some nodes and inactive on others."""
    topo = _topology(name)
    case = fd.case_of(topo)
    rng = np.random.default_rng(11 * len(name) + topo.Ne)
    I = fd.random_inertias(rng, B, topo.Ne)
    hp = ft.frame_hp()
    free = ft.total_gradient_ref(case, I, hp, ft.objective())
    ux, uy = np.abs(free.outs[0][..., 0]), np.abs(free.outs[0][..., 1])
    obj = ft.objective(3.0, 0.5 * ux.max(), 2.0, 0.5 * uy.max())
    for a, lim in ((ux, obj.sway_limit), (uy, obj.deflection_limit)):
        assert (a > lim).any() and (a < lim).any()
    return topo, case, I, hp, obj


@pytest.mark.parametrize("hinges", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_decomposition_matches_autograd_and_central_differences(name, hinges):
    topo, case, I, hp, obj = _setup(name)
    if not hinges:
        obj = ft.objective()
    r = ft.total_gradient_ref(case, I, hp, obj)
    dec, lam = ft.decomposed_gradient(case, I, hp, obj)
    tol = max(1e-10, 4e-16 * max(fd.cond_free(case, I[b]) for b in range(I.shape[0])))
    assert _nrel(dec, r.grad, ft.grad_scale(case, r, lam)) < tol
    assert (r.loss_extra > 0).all() == hinges
    np.testing.assert_allclose(r.loss_extra, ft.hinge_numpy(r.outs[0], obj), rtol=1e-13, atol=0)
    # autograd against central differences of L along relative directions (step and bound of tests/test_gpu_frame_grad.py)
    rng = np.random.default_rng(3)
    h = 1e-4
    for _ in range(3):
        d = rng.standard_normal(I.shape) * I
        quot = (ft.total_loss(case, I + h * d, hp, obj).sum() - ft.total_loss(case, I - h * d, hp, obj).sum()) / (2 * h)
        assert abs(quot - (r.grad * d).sum()) <= 2e-5 * abs(quot), (quot, (r.grad * d).sum())


_PROGRAM = r"""
#include "frame_sizing_math.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace opsamd;
template <class T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short file\n"); std::exit(2); }
  return v;
}
// <in> <out>.  in: int32 B, Nn, Ne, mode (0: rhs, 1: gradient); double[10] aM, aV, E, bend_eps, G, area_coef, aS, s_lim, aD, d_lim;
// geo, EA, E; conn, ptr, idx; I, disp, V, M; mode 1: lambda.  out: mode 0: rhs [B,Nn,3] then loss_extra [B]; mode 1: grad [B,Ne].
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = rd<int32_t>(f, 4);
  const int B = h[0], Nn = h[1], Ne = h[2], mode = h[3];
  const auto c = rd<double>(f, 10);
  const FrameSizingObj o = frame_sizing_obj(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]);
  const auto geo = rd<double>(f, 3 * (size_t)Ne), EA = rd<double>(f, Ne), E = rd<double>(f, Ne);
  const auto conn = rd<int32_t>(f, 2 * (size_t)Ne), ptr = rd<int32_t>(f, Nn + 1), idx = rd<int32_t>(f, 2 * (size_t)Ne);
  const auto I = rd<double>(f, (size_t)B * Ne), disp = rd<double>(f, (size_t)B * Nn * 3);
  const auto V = rd<double>(f, (size_t)B * Ne), M = rd<double>(f, (size_t)B * Ne);
  const auto lam = rd<double>(f, mode ? (size_t)B * Nn * 3 : 0);
  std::fclose(f);
  std::vector<double> out, extra;
  for (long b = 0; b < B; ++b) {
    if (mode == 0) {
      double hsum = 0.0;
      for (int n = 0; n < Nn; ++n) {
        double r[3];
        hsum += fs_node_rhs(o, Nn, Ne, geo.data(), EA.data(), E.data(), ptr.data(), idx.data(), I.data(), disp.data(), V.data(),
                            M.data(), b, n, r);
        out.insert(out.end(), r, r + 3);
      }
      extra.push_back(hsum);
    } else {
      for (int e = 0; e < Ne; ++e)
        out.push_back(fs_elem_grad(o, Nn, Ne, geo.data(), E.data(), conn.data(), I.data(), V.data(), M.data(), disp.data(), lam.data(), b, e));
    }
  }
  out.insert(out.end(), extra.begin(), extra.end());
  FILE* w = std::fopen(argv[2], "wb");
  if (!w || std::fwrite(out.data(), sizeof(double), out.size(), w) != out.size()) return 2;
  std::fclose(w);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found: the host program cannot be built")
    assert os.path.exists(HEADER), "csrc/frame_sizing_math.hpp is missing"
    d = tmp_path_factory.mktemp("frame_sizing")
    src, exe = d / "frame_sizing_host.cpp", d / "frame_sizing_host"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _run(program, tmp_path, topo, hp, obj, I, r, mode, lam=None):
    from openpystruct_amd import frames
    adj = frames._adjoint_tables(topo)
    B = I.shape[0]
    fin, fout = tmp_path / f"in{mode}.bin", tmp_path / f"out{mode}.bin"
    with open(fin, "wb") as f:
        np.array([B, topo.Nn, topo.Ne, mode], dtype=np.int32).tofile(f)
        np.array([hp.alpha_moment, hp.alpha_shear, hp.E, hp.bend_eps, hp.G, hp.area_coef, obj.alpha_sway, obj.sway_limit,
                  obj.alpha_deflection, obj.deflection_limit], dtype=np.float64).tofile(f)
        for t in (topo.d_geo, topo.d_EA, topo.d_E):
            t.numpy().astype(np.float64).tofile(f)
        for t in (adj.conn, adj.ptr, adj.idx):
            t.numpy().astype(np.int32).tofile(f)
        for a in [I, r.outs[0], r.outs[2], r.outs[3]] + ([lam] if mode else []):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    subprocess.check_call([program, str(fin), str(fout)])
    out = np.fromfile(fout, dtype=np.float64)
    if mode:
        return out.reshape(B, topo.Ne)
    return out[:B * topo.Nn * 3].reshape(B, topo.Nn, 3), out[B * topo.Nn * 3:]


@pytest.mark.parametrize("hinges", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_host_arithmetic_with_the_oracle_solve_matches_the_dense_reference(program, tmp_path, name, hinges):
    topo, case, I, hp, obj = _setup(name)
    if not hinges:
        obj = ft.objective()
    B = I.shape[0]
    r = ft.total_gradient_ref(case, I, hp, obj)
    _, lam_ref = ft.decomposed_gradient(case, I, hp, obj)
    rhs, extra = _run(program, tmp_path, topo, hp, obj, I, r, 0)
    lam = np.stack([bo.solve_model_3dof(topo.coords, topo.conn, topo.A, topo.E, I[b], topo.fix3, rhs[b])[0] for b in range(B)])
    grad = _run(program, tmp_path, topo, hp, obj, I, r, 1, lam)
    tol = max(1e-8, 4e-16 * max(fd.cond_free(case, I[b]) for b in range(B)))
    assert _nrel(lam, lam_ref) < tol
    assert _nrel(grad, r.grad, ft.grad_scale(case, r, lam_ref)) < tol
    want = ft.hinge_numpy(r.outs[0], obj)
    assert (np.abs(extra - want) <= 1e-12 * want).all(), (extra, want)
    assert (want > 0).all() == hinges


def test_a_nan_displacement_reaches_loss_extra(program, tmp_path):
    """The hinge's comparisons drop a NaN; the node function forwards it by hand (a frame whose forward failed)."""
    topo, case, I, hp, obj = _setup("2x3")
    r = ft.total_gradient_ref(case, I, hp, obj)
    disp = r.outs[0].copy()
    disp[1, 5, 1] = np.nan
    r.outs = (disp,) + r.outs[1:]
    _, extra = _run(program, tmp_path, topo, hp, obj, I, r, 0)
    assert np.isfinite(extra[0]) and np.isnan(extra[1])


def test_loop_oracle_reproduces_the_committed_fixture():
    """One run of each tag (the 2 x 3 frame: the fixture's generator runs all four) from the committed I0: the same epochs and the
    same float32 numbers -- the fixture is what tests/golden/make_frame_sizing_total_golden.py writes today."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_frame_sizing_total_golden", os.path.join(ROOT, "tests", "golden", "make_frame_sizing_total_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    z = np.load(GOLDEN)
    frame = "2x3"
    topo = _topology(frame)
    for tag, (cfg, obj, max_epochs) in mk.runs(frame).items():
        p = f"{tag}_{frame}_"
        assert int(z[p + "max_epochs"]) == max_epochs
        np.testing.assert_array_equal(z[p + "objective"], [obj.alpha_sway, obj.sway_limit, obj.alpha_deflection, obj.deflection_limit])
        r = ft.loop_oracle_frames(fd.case_of(topo), cfg, obj, z[f"I0_{frame}"][:2], max_epochs)
        np.testing.assert_array_equal(r.epochs, z[p + "epochs"][:2])
        np.testing.assert_allclose(r.loss, z[p + "loss"][:2], rtol=2e-6, atol=0, equal_nan=True)
        np.testing.assert_allclose(r.I, z[p + "I"][:2], rtol=0, atol=5e-6 * float(z[p + "I"].max()))
        if tag == "limit":      # both hinge branches run: the limits are exceeded at the stop (a penalty, not a constraint)
            assert (z[p + "umax"][:, 1] > obj.deflection_limit).all()
